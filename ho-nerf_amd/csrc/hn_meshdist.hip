// Mesh-to-mesh surface distance on the device: the exact closest point on a triangle mesh per query point (distance, face, point,
// barycentrics), culled by the two-level boxes of the ray caster (hn_meshcast.hip), and a deterministic surface sampler.  DESIGN.md
// 3.27 is the contract; tests/mesh_distance_cases.py restates it in numpy, in float64.
//
// The query.  Per point p and triangle (a, b, c): d2 = tri_dist2(a - p, b - p, c - p) (hn_tridist.h: Ericson 5.1.5 by selects, the
// arithmetic of hn_interact.hip's brute force, bit for bit).  The winner is the smallest (d2, face) pair, face the index in the
// CALLER's triangle array: the answer depends neither on the order of the triangles in the workspace nor on what is culled.  A
// triangle with a coordinate that is not finite has d2 = NaN or inf and never wins (the brute force's fminf drops it likewise); a
// zero-area triangle is a segment or a point, has a distance and can win.
//
// Passes:
//   k_md_prepare  one lane per workspace slot: slot s holds triangle order[s] as three float4 (a | face bits, b, c); a wave is one
//                 block of 64 slots and reduces the bounds of its finite triangles (fminf / fmaxf shuffles) -> one box per block
//   k_md_groups   one wave per group of 32 blocks: the blocks' boxes reduced -> one box per group
//   k_md_inverse, k_md_verify   `order` is a permutation: inv[order[s]] = s by plain stores, then every slot finds itself again
//   k_meshdist    one lane per point, 256 points per workgroup.  Pass A seeds an upper bound per lane: the smallest squared distance
//                 to the FARTHEST corner of a group's box, then of a block's box in that group (every triangle of a box is at most
//                 that far).  Pass B, per group: the squared distance to the box is a lower bound; a group and then each of its
//                 blocks is skipped when lb > ub (1 + m) + m diag^2 (MD_MARGIN, DESIGN.md 3.27: three orders of magnitude beyond
//                 what fp32 rounding moves a tri_dist2) -> a 32-bit mask per lane, OR-ed over the workgroup; every block some lane
//                 wants is staged once in LDS and read by all lanes at the same address (a broadcast); a wave whose ballot for the
//                 block is empty skips it.  The bound tightens with every group: ub = min(ub, best d2 so far).
//   k_ms_faces    one lane per triangle: its area in fp64 from the fp32 vertices, its unit normal
//   k_ms_sample   one lane per sample: the stratified position, a bisection of the cumulative areas, the point and the normal
// Every loop's trip count is fixed by the triangle count alone: no traversal stack, no data-dependent loop, no atomics, nothing
// between workgroups.  `cull` on and off give the same bits.
#include "hn_common.h"
#include "hn_tridist.h"

namespace hn {
namespace {

constexpr int MD_THREADS = 256;                        // points per workgroup
constexpr int MD_BLOCK = 64;                           // triangles per block: one wave of k_md_prepare, one LDS tile of k_meshdist
constexpr int MD_GROUP = 32;                           // blocks per group: one bit each in a lane's mask
constexpr float MD_MARGIN = 1e-4f;                     // m of the skip test lb > ub (1 + m) + m diag^2

struct MdLayout {
    long long nb = 0, ng = 0;
    size_t tris = 0, bbox = 0, gbox = 0, inv = 0, bad = 0, bytes = 0;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int md_layout(long long n_tris, MdLayout& L) {
    HN_REQUIRE(n_tris >= 0 && n_tris < (1LL << 31) - MD_BLOCK - 1, "hn_meshdist: n_tris = %lld outside [0, 2^31 - 65)", n_tris);
    L.nb = (n_tris + MD_BLOCK - 1) / MD_BLOCK;
    L.ng = (L.nb + MD_GROUP - 1) / MD_GROUP;
    size_t at = 0;
    L.tris = at, at = align256(at + sizeof(float4) * 3 * MD_BLOCK * (size_t)L.nb);
    L.bbox = at, at = align256(at + sizeof(float4) * 2 * (size_t)L.nb);
    L.gbox = at, at = align256(at + sizeof(float4) * 2 * (size_t)L.ng);
    L.inv = at, at = align256(at + sizeof(int) * (size_t)n_tris);      // (prepare's permutation check; not read by the query)
    L.bad = at, at = align256(at + sizeof(int));
    L.bytes = at > 256 ? at : 256;
    return HN_OK;
}

__device__ inline float wave_min_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ inline float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ inline bool finite3(float x, float y, float z) { return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff(); }

// ---- prepare: the triangles in workspace order, a box per block, a box per group -------------------------------------------------
__global__ void __launch_bounds__(MD_THREADS) k_md_prepare(const float* __restrict__ verts, long long n_verts, const long long* __restrict__ tris,
                                                           int n_tris, const int* __restrict__ order, float4* __restrict__ out_tris,
                                                           float4* __restrict__ out_bbox, int nb) {
    const int s = blockIdx.x * MD_THREADS + threadIdx.x;
    const int blk = s >> 6;
    if (blk >= nb) return;                               // (whole waves: a block is a wave)
    const float qnan = __builtin_nanf("");
    const float inf = __builtin_inff();
    float a[3] = {qnan, qnan, qnan}, b[3] = {qnan, qnan, qnan}, c[3] = {qnan, qnan, qnan};
    int face = -1;
    if (s < n_tris) {
        const int f = order[s];
        if (f >= 0 && f < n_tris) {
            face = f;
            const long long i0 = tris[3LL * f], i1 = tris[3LL * f + 1], i2 = tris[3LL * f + 2];
            if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {   // an index outside is never dereferenced
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    a[u] = verts[3 * i0 + u];
                    b[u] = verts[3 * i1 + u];
                    c[u] = verts[3 * i2 + u];
                }
            }
        }
    }
    // a zero-area triangle is kept (it has a distance); one with a coordinate that is not finite stays as it is in the slot (its
    // tri_dist2 is NaN or inf: it never wins) and stays out of the box, which would otherwise promise a triangle that far
    const bool ok = finite3(a[0], a[1], a[2]) && finite3(b[0], b[1], b[2]) && finite3(c[0], c[1], c[2]);
    out_tris[3LL * s + 0] = make_float4(a[0], a[1], a[2], __int_as_float(face));
    out_tris[3LL * s + 1] = make_float4(b[0], b[1], b[2], 0.f);
    out_tris[3LL * s + 2] = make_float4(c[0], c[1], c[2], 0.f);
    float lo[3], hi[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        lo[u] = wave_min_f(ok ? fminf(a[u], fminf(b[u], c[u])) : inf);
        hi[u] = wave_max_f(ok ? fmaxf(a[u], fmaxf(b[u], c[u])) : -inf);
    }
    if ((threadIdx.x & 63) == 0) {                       // an empty block keeps lo = +inf > hi = -inf: never a bound, never wanted
        out_bbox[2LL * blk + 0] = make_float4(lo[0], lo[1], lo[2], 0.f);
        out_bbox[2LL * blk + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

__global__ void __launch_bounds__(MD_THREADS) k_md_groups(const float4* __restrict__ bbox, int nb, float4* __restrict__ gbox, int ng) {
    const int g = blockIdx.x * (MD_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= ng) return;
    const int lane = threadIdx.x & 63;
    const int blk = g * MD_GROUP + lane;
    const float inf = __builtin_inff();
    float4 lo = make_float4(inf, inf, inf, 0.f), hi = make_float4(-inf, -inf, -inf, 0.f);
    if (lane < MD_GROUP && blk < nb) {
        lo = bbox[2LL * blk];
        hi = bbox[2LL * blk + 1];
    }
    lo.x = wave_min_f(lo.x), lo.y = wave_min_f(lo.y), lo.z = wave_min_f(lo.z);
    hi.x = wave_max_f(hi.x), hi.y = wave_max_f(hi.y), hi.z = wave_max_f(hi.z);
    if (lane == 0) {
        gbox[2LL * g] = lo;
        gbox[2LL * g + 1] = hi;
    }
}

// `order` is a permutation of 0 .. n_tris - 1 exactly when every slot finds itself in the inverse: of two slots that name the same
// triangle one loses the plain store, and an entry outside the range finds nothing.
__global__ void __launch_bounds__(MD_THREADS) k_md_inverse(const int* __restrict__ order, int n_tris, int* __restrict__ inv) {
    const int s = blockIdx.x * MD_THREADS + threadIdx.x;
    if (s >= n_tris) return;
    const int f = order[s];
    if (f >= 0 && f < n_tris) inv[f] = s;
}

__global__ void __launch_bounds__(MD_THREADS) k_md_verify(const int* __restrict__ order, int n_tris, const int* __restrict__ inv, int* __restrict__ bad) {
    const int s = blockIdx.x * MD_THREADS + threadIdx.x;
    if (s >= n_tris) return;
    const int f = order[s];
    if (!(f >= 0 && f < n_tris && inv[f] == s)) bad[0] = 1;          // (every writer stores the same value)
}

// ---- the query -----------------------------------------------------------------------------------------------------------------
// squared distance from p to the farthest corner of a box: no point of the box is farther
__device__ inline float far2(float4 lo, float4 hi, float px, float py, float pz) {
    const float fx = fmaxf(fabsf(lo.x - px), fabsf(hi.x - px)), fy = fmaxf(fabsf(lo.y - py), fabsf(hi.y - py)), fz = fmaxf(fabsf(lo.z - pz), fabsf(hi.z - pz));
    return fmaf(fx, fx, fmaf(fy, fy, fz * fz));
}

// may the box hold a triangle as near as ub?  false only when lb > ub (1 + m) + m diag^2
__device__ inline bool box_wanted(float4 lo, float4 hi, float px, float py, float pz, float ub) {
    if (!(lo.x <= hi.x)) return false;                   // an empty box
    const float nx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f), ny = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f), nz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
    const float lb = fmaf(nx, nx, fmaf(ny, ny, nz * nz));
    const float ex = hi.x - lo.x, ey = hi.y - lo.y, ez = hi.z - lo.z;
    const float diag2 = fmaf(ex, ex, fmaf(ey, ey, ez * ez));
    return !(lb > fmaf(ub, 1.f + MD_MARGIN, MD_MARGIN * diag2));     // (a NaN point wants every box, as the brute force visits all)
}

__global__ void __launch_bounds__(MD_THREADS) k_meshdist(const float4* __restrict__ tris, const float4* __restrict__ bbox,
                                                         const float4* __restrict__ gbox, int nb, int ng, const float* __restrict__ points,
                                                         int n_points, int cull, float* __restrict__ dist_out, int* __restrict__ face_out,
                                                         float* __restrict__ point_out, float* __restrict__ bary_out) {
    __shared__ float4 tile[2][3 * MD_BLOCK];
    __shared__ unsigned wmask[2][MD_THREADS / 64];
    const int p = blockIdx.x * MD_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = p < n_points;
    const float inf = __builtin_inff();
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) px = points[3LL * p], py = points[3LL * p + 1], pz = points[3LL * p + 2];

    // pass A: an upper bound on the squared distance
    float ub = inf;
    if (cull && live) {
        int gbest = 0;
        for (int g = 0; g < ng; ++g) {
            const float4 lo = gbox[2LL * g], hi = gbox[2LL * g + 1];
            const float f2 = lo.x <= hi.x ? far2(lo, hi, px, py, pz) : inf;
            if (f2 < ub) ub = f2, gbest = g;
        }
        const int b0 = gbest * MD_GROUP;
        const int nbg = nb - b0 < MD_GROUP ? nb - b0 : MD_GROUP;
        for (int j = 0; j < nbg; ++j) {
            const float4 lo = bbox[2LL * (b0 + j)], hi = bbox[2LL * (b0 + j) + 1];
            const float f2 = lo.x <= hi.x ? far2(lo, hi, px, py, pz) : inf;
            ub = fminf(ub, f2);
        }
    }

    // pass B
    float bd = inf;
    int bf = 0x7fffffff, bslot = -1;
    int buf = 0;
    for (int g = 0; g < ng; ++g) {
        const int b0 = g * MD_GROUP;
        const int nbg = nb - b0 < MD_GROUP ? nb - b0 : MD_GROUP;
        const unsigned every = nbg == MD_GROUP ? 0xffffffffu : (1u << nbg) - 1u;
        unsigned mine = 0;
        if (live) {
            if (!cull) {
                mine = every;
            } else {
                const float u = fminf(ub, bd);
                if (box_wanted(gbox[2LL * g], gbox[2LL * g + 1], px, py, pz, u)) {
                    for (int j = 0; j < nbg; ++j) mine |= box_wanted(bbox[2LL * (b0 + j)], bbox[2LL * (b0 + j) + 1], px, py, pz, u) ? 1u << j : 0u;
                }
            }
        }
        unsigned wm = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wm |= __shfl_xor(wm, o, 64);
        if (lane == 0) wmask[g & 1][w] = wm;
        __syncthreads();                                 // (the slot of group g - 2 was read before the barrier of group g - 1)
        unsigned all = 0;
#pragma unroll
        for (int u = 0; u < MD_THREADS / 64; ++u) all |= wmask[g & 1][u];
        for (int j = 0; j < nbg; ++j) {
            if (!((all >> j) & 1u)) continue;            // the same decision in every lane of the workgroup
            const long long base = 3LL * MD_BLOCK * (b0 + j);
            if (threadIdx.x < 3 * MD_BLOCK) tile[buf][threadIdx.x] = tris[base + threadIdx.x];
            __syncthreads();                             // (two tiles: the one staged before this one may still be read)
            const bool want = (mine >> j) & 1u;
            if (__ballot(want) != 0ULL && want) {
                const float4* tl = tile[buf];
#pragma unroll 2
                for (int k = 0; k < MD_BLOCK; ++k) {
                    float4 a = tl[3 * k], b = tl[3 * k + 1], c = tl[3 * k + 2];
                    const int face = __float_as_int(a.w);
                    a.x -= px, a.y -= py, a.z -= pz;
                    b.x -= px, b.y -= py, b.z -= pz;
                    c.x -= px, c.y -= py, c.z -= pz;
                    const float d2 = tri_dist2(a, b, c);
                    if (d2 < bd || (d2 == bd && face < bf && face >= 0)) {       // (an empty slot is NaN: never here)
                        bd = d2, bf = face;
                        bslot = (b0 + j) * MD_BLOCK + k;
                    }
                }
            }
            buf ^= 1;
        }
    }
    if (!live) return;
    const bool found = bslot >= 0 && bd < inf;
    if (dist_out) dist_out[p] = sqrtf(bd);
    if (face_out) face_out[p] = found ? bf : -1;
    if (point_out || bary_out) {
        float v = 0.f, wq = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
        if (found) {
            float4 a = tris[3LL * bslot], b = tris[3LL * bslot + 1], c = tris[3LL * bslot + 2];
            a.x -= px, a.y -= py, a.z -= pz;
            b.x -= px, b.y -= py, b.z -= pz;
            c.x -= px, c.y -= py, c.z -= pz;
            tri_dist2_bary(a, b, c, v, wq);
            tri_point(a, b, c, v, wq, qx, qy, qz);
            qx = px + qx, qy = py + qy, qz = pz + qz;
        }
        if (point_out) point_out[3LL * p] = qx, point_out[3LL * p + 1] = qy, point_out[3LL * p + 2] = qz;
        if (bary_out) bary_out[2LL * p] = v, bary_out[2LL * p + 1] = wq;
    }
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------
struct Face64 {
    double a[3], b[3], c[3], n[3], len;                  // the corners, (b - a) x (c - a) and its length: plain fp64 products and sums
    bool ok;
};

__device__ inline Face64 load_face(const float* __restrict__ verts, long long n_verts, const long long* __restrict__ tris, long long f) {
    Face64 F;
    const long long i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
    F.ok = i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        F.a[u] = F.ok ? (double)verts[3 * i0 + u] : 0.0;
        F.b[u] = F.ok ? (double)verts[3 * i1 + u] : 0.0;
        F.c[u] = F.ok ? (double)verts[3 * i2 + u] : 0.0;
    }
    const double e1x = F.b[0] - F.a[0], e1y = F.b[1] - F.a[1], e1z = F.b[2] - F.a[2];
    const double e2x = F.c[0] - F.a[0], e2y = F.c[1] - F.a[1], e2z = F.c[2] - F.a[2];
    F.n[0] = e1y * e2z - e1z * e2y, F.n[1] = e1z * e2x - e1x * e2z, F.n[2] = e1x * e2y - e1y * e2x;
    F.len = sqrt((F.n[0] * F.n[0] + F.n[1] * F.n[1]) + F.n[2] * F.n[2]);
    return F;
}

__global__ void __launch_bounds__(MD_THREADS) k_ms_faces(const float* __restrict__ verts, long long n_verts, const long long* __restrict__ tris,
                                                         int n_tris, double* __restrict__ area, float* __restrict__ normal) {
    const int f = blockIdx.x * MD_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    const Face64 F = load_face(verts, n_verts, tris, f);
    const bool has = F.len > 0.0 && F.len < (double)__builtin_inff();         // (a NaN or infinite vertex: area 0, never drawn)
    if (area) area[f] = has ? 0.5 * F.len : 0.0;
    if (normal) {
#pragma unroll
        for (int u = 0; u < 3; ++u) normal[3LL * f + u] = has ? (float)(F.n[u] / F.len) : 0.f;
    }
}

__device__ inline unsigned long long mix64(unsigned long long z) {    // splitmix64's output function
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(MD_THREADS) k_ms_sample(const float* __restrict__ verts, long long n_verts, const long long* __restrict__ tris,
                                                          int n_tris, const double* __restrict__ cum, int n, unsigned seed,
                                                          float* __restrict__ points, int* __restrict__ face, float* __restrict__ normal) {
    const int i = blockIdx.x * MD_THREADS + threadIdx.x;
    if (i >= n) return;
    // three outputs of splitmix64 started at the counter (seed << 32) | i, the top 24 bits of each
    const unsigned long long ctr = ((unsigned long long)seed << 32) | (unsigned long long)(unsigned)i;
    const unsigned long long G = 0x9E3779B97F4A7C15ULL;
    const double r0 = ((double)(mix64(ctr + G) >> 40) + 0.5) / 16777216.0;
    const double r1 = ((double)(mix64(ctr + 2 * G) >> 40) + 0.5) / 16777216.0;
    const double r2 = ((double)(mix64(ctr + 3 * G) >> 40) + 0.5) / 16777216.0;
    const double total = cum[n_tris - 1];
    const double u = ((double)i + r0) / (double)n * total;
    // the first triangle whose inclusive cumulative area exceeds u (the last one if none does); log2(n_tris) steps whatever u is
    int base = 0, len = n_tris;
    while (len > 1) {
        const int half = len >> 1;
        if (cum[base + half - 1] <= u) base += half;
        len -= half;
    }
    const Face64 F = load_face(verts, n_verts, tris, base);
    const bool has = F.len > 0.0 && F.len < (double)__builtin_inff();
    const double s = sqrt(r1);
    const double w0 = 1.0 - s, w1 = s * (1.0 - r2), w2 = s * r2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (points) points[3LL * i + k] = (float)((w0 * F.a[k] + w1 * F.b[k]) + w2 * F.c[k]);
        if (normal) normal[3LL * i + k] = has ? (float)(F.n[k] / F.len) : 0.f;
    }
    if (face) face[i] = base;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_meshdist_workspace_bytes(long long n_tris) {
    MdLayout L;
    return md_layout(n_tris, L) == HN_OK ? L.bytes : 0;
}

int hn_meshdist_prepare(const float* vertices, long long n_verts, const long long* triangles, long long n_tris, const int* order, void* workspace,
                        size_t workspace_bytes, hn_stream_t stream) {
    MdLayout L;
    HN_TRY_RC(md_layout(n_tris, L));
    HN_REQUIRE(n_verts >= 0, "hn_meshdist_prepare: n_verts = %lld", n_verts);
    if (n_tris == 0) return HN_OK;
    HN_REQUIRE(vertices && triangles && order && workspace, "hn_meshdist_prepare: NULL vertices / triangles / order / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshdist_prepare: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshdist_prepare: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    // the permutation check first: nothing else is written for an order that is refused
    int* inv = (int*)(ws + L.inv);
    int* bad = (int*)(ws + L.bad);
    const unsigned nt = (unsigned)((n_tris + MD_THREADS - 1) / MD_THREADS);
    HN_CHECK_HIP(hipMemsetAsync(inv, 0xff, sizeof(int) * (size_t)n_tris, s));
    HN_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    k_md_inverse<<<nt, MD_THREADS, 0, s>>>(order, (int)n_tris, inv);
    HN_LAUNCH_CHECK();
    k_md_verify<<<nt, MD_THREADS, 0, s>>>(order, (int)n_tris, inv, bad);
    HN_LAUNCH_CHECK();
    int h_bad = 0;
    HN_CHECK_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HN_CHECK_HIP(hipStreamSynchronize(s));
    HN_REQUIRE(h_bad == 0, "hn_meshdist_prepare: order is not a permutation of 0 .. %lld", n_tris - 1);
    float4* bbox = (float4*)(ws + L.bbox);
    const int per = MD_THREADS / 64;
    k_md_prepare<<<(unsigned)((L.nb + per - 1) / per), MD_THREADS, 0, s>>>(vertices, n_verts, triangles, (int)n_tris, order, (float4*)(ws + L.tris), bbox,
                                                                           (int)L.nb);
    HN_LAUNCH_CHECK();
    k_md_groups<<<(unsigned)((L.ng + per - 1) / per), MD_THREADS, 0, s>>>(bbox, (int)L.nb, (float4*)(ws + L.gbox), (int)L.ng);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_meshdist_closest(const void* workspace, size_t workspace_bytes, long long n_tris, const float* points, long long n_points, int cull,
                        float* dist, int* face, float* point, float* bary, hn_stream_t stream) {
    MdLayout L;
    HN_TRY_RC(md_layout(n_tris, L));
    HN_REQUIRE(n_points >= 0 && n_points < (1LL << 31) - MD_BLOCK - 1, "hn_meshdist_closest: n_points = %lld outside [0, 2^31 - 65)", n_points);
    if (n_tris == 0 || n_points == 0) return HN_OK;      // nothing to launch: the caller fills the outputs
    HN_REQUIRE(workspace && points, "hn_meshdist_closest: NULL workspace / points");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshdist_closest: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshdist_closest: workspace not 16-byte aligned");
    const char* ws = (const char*)workspace;
    const unsigned grid = (unsigned)((n_points + MD_THREADS - 1) / MD_THREADS);
    k_meshdist<<<grid, MD_THREADS, 0, (hipStream_t)stream>>>((const float4*)(ws + L.tris), (const float4*)(ws + L.bbox), (const float4*)(ws + L.gbox),
                                                             (int)L.nb, (int)L.ng, points, (int)n_points, cull, dist, face, point, bary);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mesh_face_areas(const float* vertices, long long n_verts, const long long* triangles, long long n_tris, double* area, float* normal,
                       hn_stream_t stream) {
    HN_REQUIRE(n_tris >= 0 && n_tris < (1LL << 31) - MD_BLOCK - 1, "hn_mesh_face_areas: n_tris = %lld outside [0, 2^31 - 65)", n_tris);
    HN_REQUIRE(n_verts >= 0, "hn_mesh_face_areas: n_verts = %lld", n_verts);
    if (n_tris == 0) return HN_OK;
    HN_REQUIRE(vertices && triangles, "hn_mesh_face_areas: NULL vertices / triangles");
    k_ms_faces<<<(unsigned)((n_tris + MD_THREADS - 1) / MD_THREADS), MD_THREADS, 0, (hipStream_t)stream>>>(vertices, n_verts, triangles, (int)n_tris,
                                                                                                         area, normal);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mesh_sample(const float* vertices, long long n_verts, const long long* triangles, long long n_tris, const double* cum_area, long long n,
                   unsigned seed, float* points, int* face, float* normal, hn_stream_t stream) {
    HN_REQUIRE(n_tris >= 0 && n_tris < (1LL << 31) - MD_BLOCK - 1, "hn_mesh_sample: n_tris = %lld outside [0, 2^31 - 65)", n_tris);
    HN_REQUIRE(n >= 0 && n < (1LL << 31) - MD_BLOCK - 1, "hn_mesh_sample: n = %lld outside [0, 2^31 - 65)", n);
    HN_REQUIRE(n_verts >= 0, "hn_mesh_sample: n_verts = %lld", n_verts);
    if (n == 0) return HN_OK;
    HN_REQUIRE(n_tris > 0, "hn_mesh_sample: %lld samples of a mesh without triangles", n);
    HN_REQUIRE(vertices && triangles && cum_area, "hn_mesh_sample: NULL vertices / triangles / cum_area");
    k_ms_sample<<<(unsigned)((n + MD_THREADS - 1) / MD_THREADS), MD_THREADS, 0, (hipStream_t)stream>>>(vertices, n_verts, triangles, (int)n_tris, cum_area,
                                                                                                     (int)n, seed, points, face, normal);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
