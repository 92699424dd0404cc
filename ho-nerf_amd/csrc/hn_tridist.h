// The point-triangle arithmetic shared by the brute-force interaction queries (hn_interact.hip) and the culled closest-point query
// (hn_meshdist.hip): one definition, so that both give the same bits per pair.  Every translation unit that includes this header is
// compiled with -ffp-contract=off: the fmaf chains below are spelled out and nothing else may fuse.
#pragma once
#include <hip/hip_runtime.h>

namespace hn {

// Squared distance from the origin to triangle (a, b, c) (relative to the point) and the barycentric pair (v, w) of the closest point
// a + ab v + ac w: Ericson, Real-Time Collision Detection 5.1.5, the regions picked in his order by selects (lanes of a wave land in
// different regions).
__device__ inline float tri_dist2_bary(float4 a, float4 b, float4 c, float& v_out, float& w_out) {
    const float abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
    const float acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
    // p - a = -a, p - b = -b, p - c = -c
    const float d1 = -fmaf(abx, a.x, fmaf(aby, a.y, abz * a.z)), d2 = -fmaf(acx, a.x, fmaf(acy, a.y, acz * a.z));
    const float d3 = -fmaf(abx, b.x, fmaf(aby, b.y, abz * b.z)), d4 = -fmaf(acx, b.x, fmaf(acy, b.y, acz * b.z));
    const float d5 = -fmaf(abx, c.x, fmaf(aby, c.y, abz * c.z)), d6 = -fmaf(acx, c.x, fmaf(acy, c.y, acz * c.z));
    const float vc = fmaf(d1, d4, -d3 * d2), vb = fmaf(d5, d2, -d1 * d6), va = fmaf(d3, d6, -d5 * d4);
    // face region by default, then the edge and vertex regions override in reverse order of Ericson's tests
    const float den = va + vb + vc;
    const float inv = den > 0.f ? 1.f / den : 0.f;
    float v = vb * inv, w = vc * inv;
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {                      // edge BC
        w = e43 / (e43 + e56);
        v = 1.f - w;
    }
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {                        // edge AC
        v = 0.f;
        w = d2 / (d2 - d6);
    }
    if (d6 >= 0.f && d5 <= d6) v = 0.f, w = 1.f;                      // vertex C
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                        // edge AB
        v = d1 / (d1 - d3);
        w = 0.f;
    }
    if (d3 >= 0.f && d4 <= d3) v = 1.f, w = 0.f;                      // vertex B
    if (d1 <= 0.f && d2 <= 0.f) v = 0.f, w = 0.f;                     // vertex A
    const float qx = fmaf(abx, v, fmaf(acx, w, a.x)), qy = fmaf(aby, v, fmaf(acy, w, a.y)), qz = fmaf(abz, v, fmaf(acz, w, a.z));
    v_out = v, w_out = w;
    return fmaf(qx, qx, fmaf(qy, qy, qz * qz));
}

__device__ inline float tri_dist2(float4 a, float4 b, float4 c) {
    float v, w;
    return tri_dist2_bary(a, b, c, v, w);
}

// The closest point itself, relative to the query: a + ab v + ac w in tri_dist2's fmaf chain, for the (v, w) it returned.
__device__ inline void tri_point(float4 a, float4 b, float4 c, float v, float w, float& qx, float& qy, float& qz) {
    const float abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
    const float acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
    qx = fmaf(abx, v, fmaf(acx, w, a.x)), qy = fmaf(aby, v, fmaf(acy, w, a.y)), qz = fmaf(abz, v, fmaf(acz, w, a.z));
}

}  // namespace hn
