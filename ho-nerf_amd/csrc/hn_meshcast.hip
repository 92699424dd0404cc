// Ray casting of triangle meshes on the device: the nearest triangle along each ray, for the rays of the volume render (hn_ray_gen), so
// that a mesh view and a field view are comparable pixel for pixel.  DESIGN.md 3.21 is the contract; tests/meshcast_cases.py restates it
// in numpy, in float64 (the reference) and in float32 in this file's operation order (the bits of this kernel).
//
// The intersection rule (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013), per ray o + t d and triangle (a, b, c):
//   kz = the axis of the largest |d_i| (lowest index on ties), kx, ky the next two cyclically, swapped when d[kz] < 0;
//   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];  A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz] (B, C likewise);
//   U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax in plain fp32 products and differences (the file is compiled with
//   -ffp-contract=off); if one of them is exactly 0 all three are formed again in double from the same fp32 Ax .. Cy and rounded to fp32;
//   a miss when one is negative while another is positive (two-sided: back faces hit), and when det = (U + V) + W is 0;
//   t = ((U Az + V Bz) + W Cz) / det with Az = Sz A[kz]; a hit needs near <= t <= far; the weights of b and c are V / det, W / det;
//   the nearest hit is the smallest (t, face) pair, face the index in the CALLER's triangle array: the answer depends neither on the
//   order of the triangles in the workspace nor on the rays around it;
//   the normal is the triangle's own normalize((b - a) x (c - a)), not turned toward the ray.
// A triangle with a vertex that is not finite, with a vertex index outside [0, V) or with (b - a) x (c - a) of squared length 0 or
// not finite is stored as NaN and never hits (every comparison of the rule is false on it); a ray with d[kz] = 0 never hits.
// An edge shared by two triangles gets its function from the same two sheared vertices in both, exactly antisymmetric, and the
// double form has the sign of the fp32 form wherever that is not 0: a ray cannot slip between two triangles that share an edge.
//
// Passes:
//   k_mc_prepare  one lane per workspace slot: slot s holds triangle order[s] as three float4 (a | face bits, b, c); a wave is one
//                 block of 64 slots and reduces its bounds (shuffles) -> one box per block
//   k_mc_groups   one wave per group of 32 blocks: the blocks' boxes reduced -> one box per group
//   k_meshcast    one lane per ray, 256 rays per workgroup.  For every group: a slab test against the group's box on
//                 [near, min(far, t_best)], in a surviving group one against each of its blocks' boxes -> a 32-bit mask per lane, OR-ed
//                 over the workgroup; every block some lane wants is staged once in LDS and read by all lanes at the same address
//                 (a broadcast, k_cd_partial's pattern); a wave whose ballot for the block is empty skips it.
// Every loop's trip count is fixed by the triangle count alone: no traversal stack, no data-dependent loop, no atomics, nothing
// between workgroups.  The boxes only remove work: a slab test is widened by 1e-4 of the ray origin's distance to the box's far
// corner, three orders of magnitude beyond what fp32 rounding moves a hit, so `cull` on and off give the same bits.
#include "hn_common.h"

namespace hn {
namespace {

constexpr int MC_THREADS = 256;                        // rays per workgroup
constexpr int MC_BLOCK = 64;                           // triangles per block: one wave of k_mc_prepare, one LDS tile of k_meshcast
constexpr int MC_GROUP = 32;                           // blocks per group: one bit each in a lane's mask
constexpr float MC_PAD = 1e-4f;                        // slab widening, relative to the distance from the ray origin

struct McLayout {
    long long nb = 0, ng = 0;
    size_t tris = 0, bbox = 0, gbox = 0, bytes = 0;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int mc_layout(long long n_tris, McLayout& L) {
    HN_REQUIRE(n_tris >= 0 && n_tris < (1LL << 31) - MC_BLOCK, "hn_meshcast: n_tris = %lld outside [0, 2^31 - 64)", n_tris);
    L.nb = (n_tris + MC_BLOCK - 1) / MC_BLOCK;
    L.ng = (L.nb + MC_GROUP - 1) / MC_GROUP;
    size_t at = 0;
    L.tris = at, at = align256(at + sizeof(float4) * 3 * MC_BLOCK * (size_t)L.nb);
    L.bbox = at, at = align256(at + sizeof(float4) * 2 * (size_t)L.nb);
    L.gbox = at, at = align256(at + sizeof(float4) * 2 * (size_t)L.ng);
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

// ---- prepare: the triangles in workspace order, a box per block ------------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS) k_mc_prepare(const float* __restrict__ verts, long long n_verts, const long long* __restrict__ tris,
                                                           int n_tris, const int* __restrict__ order, float4* __restrict__ out_tris,
                                                           float4* __restrict__ out_bbox, int nb) {
    const int s = blockIdx.x * MC_THREADS + threadIdx.x;
    const int blk = s >> 6;
    if (blk >= nb) return;                               // (whole waves: a block is a wave)
    const float qnan = __builtin_nanf("");
    const float inf = __builtin_inff();
    float a[3] = {qnan, qnan, qnan}, b[3] = {qnan, qnan, qnan}, c[3] = {qnan, qnan, qnan};
    int face = -1;
    bool ok = false;
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
                const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
                const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
                const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
                const float n2 = (nx * nx + ny * ny) + nz * nz;
                ok = finite3(a[0], a[1], a[2]) && finite3(b[0], b[1], b[2]) && finite3(c[0], c[1], c[2]) && n2 > 0.f && n2 < inf;
            }
        }
    }
    if (!ok) {
#pragma unroll
        for (int u = 0; u < 3; ++u) a[u] = b[u] = c[u] = qnan;
    }
    out_tris[3LL * s + 0] = make_float4(a[0], a[1], a[2], __int_as_float(face));
    out_tris[3LL * s + 1] = make_float4(b[0], b[1], b[2], 0.f);
    out_tris[3LL * s + 2] = make_float4(c[0], c[1], c[2], 0.f);
    float lo[3], hi[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        lo[u] = wave_min_f(ok ? fminf(a[u], fminf(b[u], c[u])) : inf);
        hi[u] = wave_max_f(ok ? fmaxf(a[u], fmaxf(b[u], c[u])) : -inf);
    }
    if ((threadIdx.x & 63) == 0) {                       // an empty block keeps lo = +inf > hi = -inf: no ray enters it
        out_bbox[2LL * blk + 0] = make_float4(lo[0], lo[1], lo[2], 0.f);
        out_bbox[2LL * blk + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_groups(const float4* __restrict__ bbox, int nb, float4* __restrict__ gbox, int ng) {
    const int g = blockIdx.x * (MC_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= ng) return;
    const int lane = threadIdx.x & 63;
    const int blk = g * MC_GROUP + lane;
    const float inf = __builtin_inff();
    float4 lo = make_float4(inf, inf, inf, 0.f), hi = make_float4(-inf, -inf, -inf, 0.f);
    if (lane < MC_GROUP && blk < nb) {
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

// ---- cast --------------------------------------------------------------------------------------------------------------------------
__device__ inline float pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

struct Slab {
    float ox, oy, oz, ix, iy, iz;                        // origin, 1 / d per axis (0 where d is 0)
    bool px, py, pz;                                     // d is 0 on that axis: the origin must lie between the planes
};

// One axis of the slab test: [t0, t1] cut down to where the ray lies between lo - pad and hi + pad.
__device__ inline void slab_axis(float lo, float hi, float o, float inv, bool par, float pad, float& t0, float& t1) {
    const float l = (lo - pad) - o, h = (hi + pad) - o;
    const float ta = l * inv, tb = h * inv;
    const float en = par ? (l <= 0.f && h >= 0.f ? -__builtin_inff() : __builtin_inff()) : fminf(ta, tb);
    const float ex = par ? __builtin_inff() : fmaxf(ta, tb);
    t0 = fmaxf(t0, en);
    t1 = fminf(t1, ex);
}

__device__ inline bool slab_hit(const Slab& r, float4 lo, float4 hi, float t0, float t1) {
    if (!(lo.x <= hi.x)) return false;                   // an empty box
    const float far_corner = fmaxf(fmaxf(fmaxf(fabsf(lo.x - r.ox), fabsf(hi.x - r.ox)), fmaxf(fabsf(lo.y - r.oy), fabsf(hi.y - r.oy))),
                                   fmaxf(fabsf(lo.z - r.oz), fabsf(hi.z - r.oz)));
    const float pad = MC_PAD * far_corner;
    slab_axis(lo.x, hi.x, r.ox, r.ix, r.px, pad, t0, t1);
    slab_axis(lo.y, hi.y, r.oy, r.iy, r.py, pad, t0, t1);
    slab_axis(lo.z, hi.z, r.oz, r.iz, r.pz, pad, t0, t1);
    return t0 <= t1;
}

__global__ void __launch_bounds__(MC_THREADS) k_meshcast(const float4* __restrict__ tris, const float4* __restrict__ bbox,
                                                         const float4* __restrict__ gbox, int nb, int ng, const float* __restrict__ rays_o,
                                                         const float* __restrict__ rays_d, int n_rays, float near, float far, int cull,
                                                         float* __restrict__ t_out, int* __restrict__ face_out, float* __restrict__ bary_out,
                                                         float* __restrict__ normal_out) {
    __shared__ float4 tile[2][3 * MC_BLOCK];
    __shared__ unsigned wmask[2][MC_THREADS / 64];
    const int r = blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool in_range = r < n_rays;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (in_range) {
        ox = rays_o[3LL * r], oy = rays_o[3LL * r + 1], oz = rays_o[3LL * r + 2];
        dx = rays_d[3LL * r], dy = rays_d[3LL * r + 1], dz = rays_d[3LL * r + 2];
    }
    // per-ray setup
    int kz = 0;
    float big = fabsf(dx);
    if (fabsf(dy) > big) kz = 1, big = fabsf(dy);
    if (fabsf(dz) > big) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dkz = pick(dx, dy, dz, kz);
    if (dkz < 0.f) {
        const int k = kx;
        kx = ky, ky = k;
    }
    const bool live = in_range && dkz != 0.f;
    const float Sx = pick(dx, dy, dz, kx) / dkz, Sy = pick(dx, dy, dz, ky) / dkz, Sz = 1.f / dkz;
    const float okx = pick(ox, oy, oz, kx), oky = pick(ox, oy, oz, ky), okz = pick(ox, oy, oz, kz);
    Slab sl;
    sl.ox = ox, sl.oy = oy, sl.oz = oz;
    sl.px = dx == 0.f, sl.py = dy == 0.f, sl.pz = dz == 0.f;
    sl.ix = sl.px ? 0.f : 1.f / dx, sl.iy = sl.py ? 0.f : 1.f / dy, sl.iz = sl.pz ? 0.f : 1.f / dz;

    float bt = __builtin_inff(), bV = 0.f, bW = 0.f, bDet = 1.f;
    int bf = 0x7fffffff, bslot = -1;
    int buf = 0;
    for (int g = 0; g < ng; ++g) {
        const int b0 = g * MC_GROUP;
        const int nbg = nb - b0 < MC_GROUP ? nb - b0 : MC_GROUP;
        const unsigned every = nbg == MC_GROUP ? 0xffffffffu : (1u << nbg) - 1u;
        unsigned mine = 0;
        if (live) {
            if (!cull) {
                mine = every;
            } else {
                const float t1 = fminf(far, bt);
                if (slab_hit(sl, gbox[2LL * g], gbox[2LL * g + 1], near, t1)) {
                    for (int j = 0; j < nbg; ++j) mine |= slab_hit(sl, bbox[2LL * (b0 + j)], bbox[2LL * (b0 + j) + 1], near, t1) ? 1u << j : 0u;
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
        for (int u = 0; u < MC_THREADS / 64; ++u) all |= wmask[g & 1][u];
        for (int j = 0; j < nbg; ++j) {
            if (!((all >> j) & 1u)) continue;            // the same decision in every lane of the workgroup
            const long long base = 3LL * MC_BLOCK * (b0 + j);
            if (threadIdx.x < 3 * MC_BLOCK) tile[buf][threadIdx.x] = tris[base + threadIdx.x];
            __syncthreads();                             // (two tiles: the one staged before this one may still be read)
            const bool want = (mine >> j) & 1u;
            if (__ballot(want) != 0ULL && want) {
                const float4* tl = tile[buf];
#pragma unroll 2
                for (int k = 0; k < MC_BLOCK; ++k) {
                    const float4 A4 = tl[3 * k], B4 = tl[3 * k + 1], C4 = tl[3 * k + 2];
                    const float Akz = pick(A4.x, A4.y, A4.z, kz) - okz, Bkz = pick(B4.x, B4.y, B4.z, kz) - okz, Ckz = pick(C4.x, C4.y, C4.z, kz) - okz;
                    const float Ax = (pick(A4.x, A4.y, A4.z, kx) - okx) - Sx * Akz, Ay = (pick(A4.x, A4.y, A4.z, ky) - oky) - Sy * Akz;
                    const float Bx = (pick(B4.x, B4.y, B4.z, kx) - okx) - Sx * Bkz, By = (pick(B4.x, B4.y, B4.z, ky) - oky) - Sy * Bkz;
                    const float Cx = (pick(C4.x, C4.y, C4.z, kx) - okx) - Sx * Ckz, Cy = (pick(C4.x, C4.y, C4.z, ky) - oky) - Sy * Ckz;
                    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
                    if (U == 0.f || V == 0.f || W == 0.f) {
                        U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
                        V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
                        W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
                    }
                    const bool mixed = (U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f);
                    const float det = (U + V) + W;
                    if (!mixed && det != 0.f) {
                        const float t = ((U * (Sz * Akz) + V * (Sz * Bkz)) + W * (Sz * Ckz)) / det;
                        const int face = __float_as_int(A4.w);
                        if (t >= near && t <= far && (t < bt || (t == bt && face < bf))) {
                            bt = t, bf = face, bV = V, bW = W, bDet = det;
                            bslot = (b0 + j) * MC_BLOCK + k;
                        }
                    }
                }
            }
            buf ^= 1;
        }
    }
    if (!in_range) return;
    const bool hit = bslot >= 0;
    if (t_out) t_out[r] = hit ? bt : 0.f;
    if (face_out) face_out[r] = hit ? bf : -1;
    if (bary_out) {
        bary_out[2LL * r] = hit ? bV / bDet : 0.f;
        bary_out[2LL * r + 1] = hit ? bW / bDet : 0.f;
    }
    if (normal_out) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (hit) {
            const float4 a = tris[3LL * bslot], b = tris[3LL * bslot + 1], c = tris[3LL * bslot + 2];
            const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
            const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
            nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
            nx = nx / len, ny = ny / len, nz = nz / len;
        }
        normal_out[3LL * r] = nx;
        normal_out[3LL * r + 1] = ny;
        normal_out[3LL * r + 2] = nz;
    }
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_meshcast_workspace_bytes(long long n_tris) {
    McLayout L;
    return mc_layout(n_tris, L) == HN_OK ? L.bytes : 0;
}

int hn_meshcast_prepare(const float* vertices, long long n_verts, const long long* triangles, long long n_tris, const int* order, void* workspace,
                        size_t workspace_bytes, hn_stream_t stream) {
    McLayout L;
    HN_TRY_RC(mc_layout(n_tris, L));
    HN_REQUIRE(n_verts >= 0, "hn_meshcast_prepare: n_verts = %lld", n_verts);
    if (n_tris == 0) return HN_OK;
    HN_REQUIRE(vertices && triangles && order && workspace, "hn_meshcast_prepare: NULL vertices / triangles / order / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshcast_prepare: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshcast_prepare: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    float4* bbox = (float4*)(ws + L.bbox);
    const int per = MC_THREADS / 64;
    k_mc_prepare<<<(unsigned)((L.nb + per - 1) / per), MC_THREADS, 0, s>>>(vertices, n_verts, triangles, (int)n_tris, order, (float4*)(ws + L.tris), bbox,
                                                                           (int)L.nb);
    HN_LAUNCH_CHECK();
    k_mc_groups<<<(unsigned)((L.ng + per - 1) / per), MC_THREADS, 0, s>>>(bbox, (int)L.nb, (float4*)(ws + L.gbox), (int)L.ng);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_meshcast(const void* workspace, size_t workspace_bytes, long long n_tris, const float* rays_o, const float* rays_d, long long n_rays, float near,
                float far, int cull, float* t, int* face, float* bary, float* normal, hn_stream_t stream) {
    McLayout L;
    HN_TRY_RC(mc_layout(n_tris, L));
    HN_REQUIRE(n_rays >= 0 && n_rays < (1LL << 31) - MC_THREADS, "hn_meshcast: n_rays = %lld outside [0, 2^31 - 256)", n_rays);
    if (n_tris == 0 || n_rays == 0) return HN_OK;        // nothing to launch: the caller fills the outputs
    HN_REQUIRE(workspace && rays_o && rays_d, "hn_meshcast: NULL workspace / rays_o / rays_d");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshcast: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshcast: workspace not 16-byte aligned");
    const char* ws = (const char*)workspace;
    const unsigned grid = (unsigned)((n_rays + MC_THREADS - 1) / MC_THREADS);
    k_meshcast<<<grid, MC_THREADS, 0, (hipStream_t)stream>>>((const float4*)(ws + L.tris), (const float4*)(ws + L.bbox), (const float4*)(ws + L.gbox),
                                                             (int)L.nb, (int)L.ng, rays_o, rays_d, (int)n_rays, near, far, cull, t, face, bary, normal);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
