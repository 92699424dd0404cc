// Hand-object interaction geometry on the device: what analys_results/analys_interaction.py asks trimesh for, on the meshes that
// extract_geometry(..., mesher='native') produces.  Meshes come in as one row of 9 coordinates per triangle (a, b, c; world metres).
//
// Three queries (tests/test_interaction_cpu.py restates them in float64 numpy; DESIGN.md 3.14 is the contract):
//   voxelize  trimesh's Trimesh.voxelized(pitch) (subdivide, max_iter = 10): a triangle with any edge length
//             sqrt((dx^2 + dy^2) + dz^2) > pitch / 2 is split 4-way at its edge midpoints (a + b) / 2, each child is judged again;
//             every vertex of every leaf is snapped to k = rint(v / pitch).  The cap is this project's choice: 10 rounds are
//             allowed and a triangle that needs an 11th is refused (trimesh's own loop may already refuse one that needs 10).
//             fp64 throughout, and the file is compiled with -ffp-contract=off so that the bits are those of the numpy restatement.
//   winding   trimesh's Trimesh.contains: inside <=> |w| > 1/2, w the generalized winding number, the sum over the triangles of the
//             Van Oosterom-Strackee solid angle 2 atan2(det, den) over 4 pi.  fp32.
//   distance  trimesh.proximity.closest_point's distance: the exact unsigned distance to the nearest triangle (Ericson's closest
//             point on a triangle, its seven regions picked by selects).  fp32.
//
// Passes:
//   k_vox_count   one thread per triangle: walks the leaves of its subdivision, writes 3 x leaves (0 for a refused triangle) and
//                 the workgroup's sums of keys and of refusals
//   k_vox_scan    one workgroup: exclusive scan of the workgroup sums -> key offsets and the totals {keys, too deep, out of range}
//   k_vox_emit    one thread per triangle: the same walk, writing the 3 packed keys of every leaf at its scanned offset
//   k_wn_partial  point-parallel (256 points per workgroup) x a range of the triangles (blockIdx.y): triangles staged through LDS
//                 in tiles of 256, every lane reads the same triangle (a broadcast); one partial sum per point and range, in a
//                 fixed triangle order
//   k_wn_combine  per point: the partial sums in range order -> inside flag (and w)
//   k_cd_partial  the same tiling with a running minimum of the squared distance
//   k_cd_combine  per point: minimum over the ranges -> distance
// There are no atomics: a repeated call gives the same bits.
#include "hn_common.h"
#include "hn_tridist.h"

namespace hn {
namespace {

constexpr int VOX_THREADS = 256;
constexpr int VOX_SCAN_THREADS = 1024;
constexpr int VOX_MAX_ROUNDS = 10;                     // the project's cap: 10 rounds allowed, an 11th refused (see above)
constexpr double VOX_KEY_LIMIT = 1048575.0;            // |v / pitch| below this: k + 2^20 fits 21 bits
constexpr int KEY_BIAS = 1 << 20;

constexpr int WN_THREADS = 256;                        // points per workgroup
constexpr int WN_TILE = 256;                           // triangles per LDS tile
constexpr long long WN_TARGET_BLOCKS = 2048;           // 256 CUs x 8 workgroups: split the triangles until the grid has about this many

// ---- voxelization: the subdivision walk ------------------------------------------------------------------------------------------
struct Tri64 {
    double v[9];
};

__device__ inline bool too_long(const Tri64& t, double max_edge) {
    bool r = false;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int a = e, b = e == 2 ? 0 : e + 1;
        const double dx = t.v[3 * b] - t.v[3 * a], dy = t.v[3 * b + 1] - t.v[3 * a + 1], dz = t.v[3 * b + 2] - t.v[3 * a + 2];
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        r = r || len > max_edge;
    }
    return r;
}

// child k of t, trimesh's order: (a, m01, m20), (m01, b, m12), (m20, m12, c), (m01, m12, m20)
__device__ inline Tri64 child(const Tri64& t, int k) {
    double m01[3], m12[3], m20[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        m01[d] = (t.v[d] + t.v[3 + d]) / 2.0;
        m12[d] = (t.v[3 + d] + t.v[6 + d]) / 2.0;
        m20[d] = (t.v[6 + d] + t.v[d]) / 2.0;
    }
    Tri64 c;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double p0 = k == 0 ? t.v[d] : k == 2 ? m20[d] : m01[d];
        const double p1 = k == 0 ? m01[d] : k == 1 ? t.v[3 + d] : m12[d];
        const double p2 = k == 0 ? m20[d] : k == 1 ? m12[d] : k == 2 ? t.v[6 + d] : m20[d];
        c.v[d] = p0;
        c.v[3 + d] = p1;
        c.v[6 + d] = p2;
    }
    return c;
}

__device__ inline long long pack_key(const double* v, double pitch) {
    const long long kx = (long long)rint(v[0] / pitch), ky = (long long)rint(v[1] / pitch), kz = (long long)rint(v[2] / pitch);
    return ((kx + KEY_BIAS) << 42) | ((ky + KEY_BIAS) << 21) | (kz + KEY_BIAS);
}

// Depth-first walk over the leaves without a stack: `path` holds the child index of every level (2 bits each), the node at the
// current path is rebuilt from the root (at most VOX_MAX_ROUNDS midpoint steps).  fn(leaf) per leaf, in a fixed order.
// Returns the number of leaves, or -1 when a node at depth VOX_MAX_ROUNDS is still too long.
template <class Fn>
__device__ inline long long walk_leaves(const Tri64& root, double max_edge, Fn fn) {
    unsigned path = 0;
    int depth = 0;
    long long leaves = 0;
    for (;;) {
        Tri64 t = root;
        for (int d = 0; d < depth; ++d) t = child(t, (path >> (2 * d)) & 3);
        while (too_long(t, max_edge)) {
            if (depth == VOX_MAX_ROUNDS) return -1;
            path &= ~(3u << (2 * depth));
            t = child(t, 0);
            ++depth;
        }
        fn(t);
        ++leaves;
        while (depth > 0 && ((path >> (2 * (depth - 1))) & 3) == 3) --depth;
        if (depth == 0) return leaves;
        path += 1u << (2 * (depth - 1));
    }
}

__device__ inline Tri64 load_tri64(const double* __restrict__ tv, long long t) {
    Tri64 r;
#pragma unroll
    for (int u = 0; u < 9; ++u) r.v[u] = tv[9 * t + u];
    return r;
}

__device__ inline bool keys_in_range(const Tri64& t, double pitch) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < 9; ++u) ok = ok && fabs(t.v[u] / pitch) < VOX_KEY_LIMIT;   // false for NaN / inf too
    return ok;
}

__device__ inline int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// exclusive scan of one value per thread over the workgroup (NT threads); total = the workgroup's sum
template <int NT, class I>
__device__ inline I block_excl_scan(I v, I* lds, I& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    I incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const I u = __shfl_up(incl, o, 64);
        incl += lane >= o ? u : 0;
    }
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    I before = 0;
    total = 0;
#pragma unroll
    for (int u = 0; u < NT / 64; ++u) {
        const I s = lds[u];
        before += u < w ? s : 0;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}

// ---- pass 1: leaf keys per triangle --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VOX_THREADS) k_vox_count(const double* __restrict__ tv, int n_tris, double pitch, int* __restrict__ cnt,
                                                           int* __restrict__ blk) {
    const int t = blockIdx.x * VOX_THREADS + threadIdx.x;
    int keys = 0, deep = 0, oor = 0;
    if (t < n_tris) {
        const Tri64 root = load_tri64(tv, t);
        if (!keys_in_range(root, pitch)) {
            oor = 1;
        } else {
            const long long leaves = walk_leaves(root, pitch / 2.0, [](const Tri64&) {});
            if (leaves < 0)
                deep = 1;
            else
                keys = (int)(3 * leaves);
        }
        cnt[t] = keys;
    }
    __shared__ int red[3][VOX_THREADS / 64];
    keys = wave_sum_i(keys);
    deep = wave_sum_i(deep);
    oor = wave_sum_i(oor);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w] = keys;
        red[1][w] = deep;
        red[2][w] = oor;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int s = 0;
#pragma unroll
        for (int u = 0; u < VOX_THREADS / 64; ++u) s += red[threadIdx.x][u];
        blk[3 * blockIdx.x + threadIdx.x] = s;
    }
}

// ---- pass 2: exclusive scan of the workgroup key sums (one workgroup, 64-bit); totals = {keys, too deep, out of range} --------
__global__ void __launch_bounds__(VOX_SCAN_THREADS) k_vox_scan(const int* __restrict__ blk, int nb, long long* __restrict__ off,
                                                               long long* __restrict__ totals) {
    __shared__ long long lds[VOX_SCAN_THREADS / 64];
    long long carry = 0, deep = 0, oor = 0;
    for (int base = 0; base < nb; base += VOX_SCAN_THREADS) {
        const int b = base + threadIdx.x;
        const long long v = b < nb ? blk[3 * b] : 0;
        long long tot, tot_d, tot_o;
        const long long e = block_excl_scan<VOX_SCAN_THREADS>(v, lds, tot);
        block_excl_scan<VOX_SCAN_THREADS>(b < nb ? (long long)blk[3 * b + 1] : 0LL, lds, tot_d);
        block_excl_scan<VOX_SCAN_THREADS>(b < nb ? (long long)blk[3 * b + 2] : 0LL, lds, tot_o);
        if (b < nb) off[b] = carry + e;
        carry += tot;
        deep += tot_d;
        oor += tot_o;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry;
        totals[1] = deep;
        totals[2] = oor;
    }
}

// ---- pass 3: the keys --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VOX_THREADS) k_vox_emit(const double* __restrict__ tv, int n_tris, double pitch, const int* __restrict__ cnt,
                                                          const long long* __restrict__ off, long long* __restrict__ keys, long long n_keys) {
    __shared__ int lds[VOX_THREADS / 64];
    const int t = blockIdx.x * VOX_THREADS + threadIdx.x;
    const int c = t < n_tris ? cnt[t] : 0;
    int total;
    const int excl = block_excl_scan<VOX_THREADS>(c, lds, total);   // at most 256 x 3 x 4^10 < 2^31
    if (c == 0) return;                                  // refused triangles were counted 0: they write nothing
    long long at = off[blockIdx.x] + excl;
    const long long end = at + c;
    walk_leaves(load_tri64(tv, t), pitch / 2.0, [&](const Tri64& leaf) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            if (at < end && at < n_keys) keys[at] = pack_key(leaf.v + 3 * u, pitch);
            ++at;
        }
    });
}

// ---- winding number and distance: point-parallel, triangles through LDS ---------------------------------------------------------
struct Split {
    int n_splits, tris_per_split;
};

__host__ __device__ inline Split split_of(long long n_points, long long n_tris) {
    const long long nb = (n_points + WN_THREADS - 1) / WN_THREADS;
    const long long tiles = (n_tris + WN_TILE - 1) / WN_TILE;
    long long s = nb > 0 ? (WN_TARGET_BLOCKS + nb - 1) / nb : 1;
    s = s < 1 ? 1 : s > tiles ? tiles : s;
    if (s < 1) s = 1;
    const long long tiles_per = (tiles + s - 1) / s;
    Split r;
    r.tris_per_split = (int)(tiles_per * WN_TILE > 0 ? tiles_per * WN_TILE : WN_TILE);
    r.n_splits = (int)((n_tris + r.tris_per_split - 1) / r.tris_per_split);
    if (r.n_splits < 1) r.n_splits = 1;
    return r;
}

__device__ inline bool in_box(float x, float y, float z, const float* bb) {
    return x >= bb[0] && y >= bb[1] && z >= bb[2] && x <= bb[3] && y <= bb[4] && z <= bb[5];
}

// stage triangles [base, base + n) of the row-of-9 array into tile (3 float4 per triangle: a, b, c; w unused)
__device__ inline void stage_tile(const float* __restrict__ tv, long long base, int n, float4* tile) {
    const int j = threadIdx.x;
    if (j < n) {
        const float* s = tv + 9 * (base + j);
        tile[3 * j + 0] = make_float4(s[0], s[1], s[2], 0.f);
        tile[3 * j + 1] = make_float4(s[3], s[4], s[5], 0.f);
        tile[3 * j + 2] = make_float4(s[6], s[7], s[8], 0.f);
    }
}

// half the Van Oosterom-Strackee solid angle of triangle (a, b, c) seen from the origin (a, b, c already relative to the point)
__device__ inline float half_solid_angle(float4 a, float4 b, float4 c) {
    const float la = __builtin_amdgcn_sqrtf(fmaf(a.x, a.x, fmaf(a.y, a.y, a.z * a.z)));
    const float lb = __builtin_amdgcn_sqrtf(fmaf(b.x, b.x, fmaf(b.y, b.y, b.z * b.z)));
    const float lc = __builtin_amdgcn_sqrtf(fmaf(c.x, c.x, fmaf(c.y, c.y, c.z * c.z)));
    const float cx = fmaf(b.y, c.z, -b.z * c.y), cy = fmaf(b.z, c.x, -b.x * c.z), cz = fmaf(b.x, c.y, -b.y * c.x);
    const float det = fmaf(a.x, cx, fmaf(a.y, cy, a.z * cz));
    const float ab = fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z));
    const float bc = fmaf(b.x, c.x, fmaf(b.y, c.y, b.z * c.z));
    const float ca = fmaf(c.x, a.x, fmaf(c.y, a.y, c.z * a.z));
    const float den = fmaf(la * lb, lc, fmaf(ab, lc, fmaf(bc, la, ca * lb)));
    return atan2f(det, den);
}

__global__ void __launch_bounds__(WN_THREADS) k_wn_partial(const float* __restrict__ pts, int n_points, const float* __restrict__ tv, int n_tris,
                                                           int tris_per_split, const float* __restrict__ bbox, float* __restrict__ partial) {
    __shared__ float4 tile[3 * WN_TILE];
    const int p = blockIdx.x * WN_THREADS + threadIdx.x;
    const long long t0 = (long long)blockIdx.y * tris_per_split;
    const long long t1 = t0 + tris_per_split < n_tris ? t0 + tris_per_split : n_tris;
    float px = 0.f, py = 0.f, pz = 0.f;
    bool live = false;
    if (p < n_points) {
        px = pts[3LL * p];
        py = pts[3LL * p + 1];
        pz = pts[3LL * p + 2];
        live = in_box(px, py, pz, bbox);
    }
    if (!__syncthreads_or(live)) return;                 // the AABB early-out, for the whole workgroup at once
    float acc = 0.f;
    for (long long base = t0; base < t1; base += WN_TILE) {
        const int n = t1 - base < WN_TILE ? (int)(t1 - base) : WN_TILE;
        __syncthreads();                                  // the previous tile is consumed
        stage_tile(tv, base, n, tile);
        __syncthreads();
        if (live) {
            const float4 o = make_float4(px, py, pz, 0.f);
#pragma unroll 2
            for (int j = 0; j < n; ++j) {
                float4 a = tile[3 * j], b = tile[3 * j + 1], c = tile[3 * j + 2];
                a.x -= o.x, a.y -= o.y, a.z -= o.z;
                b.x -= o.x, b.y -= o.y, b.z -= o.z;
                c.x -= o.x, c.y -= o.y, c.z -= o.z;
                acc += half_solid_angle(a, b, c);
            }
        }
    }
    if (live) partial[(long long)blockIdx.y * n_points + p] = acc;
}

__global__ void __launch_bounds__(WN_THREADS) k_wn_combine(const float* __restrict__ pts, int n_points, const float* __restrict__ bbox,
                                                           const float* __restrict__ partial, int n_splits, unsigned char* __restrict__ inside,
                                                           float* __restrict__ winding) {
    const int p = blockIdx.x * WN_THREADS + threadIdx.x;
    if (p >= n_points) return;
    float s = 0.f;
    if (in_box(pts[3LL * p], pts[3LL * p + 1], pts[3LL * p + 2], bbox)) {
        for (int k = 0; k < n_splits; ++k) s += partial[(long long)k * n_points + p];
    }
    const float w = s * (float)(0.5 / 3.14159265358979323846);   // sum of half solid angles / (2 pi) = sum of solid angles / (4 pi)
    inside[p] = fabsf(w) > 0.5f ? 1 : 0;
    if (winding) winding[p] = w;
}

// tri_dist2: the squared distance from the origin to a triangle given relative to the point (hn_tridist.h, shared with hn_meshdist.hip)

__global__ void __launch_bounds__(WN_THREADS) k_cd_partial(const float* __restrict__ pts, int n_points, const float* __restrict__ tv, int n_tris,
                                                           int tris_per_split, float* __restrict__ partial) {
    __shared__ float4 tile[3 * WN_TILE];
    const int p = blockIdx.x * WN_THREADS + threadIdx.x;
    const long long t0 = (long long)blockIdx.y * tris_per_split;
    const long long t1 = t0 + tris_per_split < n_tris ? t0 + tris_per_split : n_tris;
    const bool live = p < n_points;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) {
        px = pts[3LL * p];
        py = pts[3LL * p + 1];
        pz = pts[3LL * p + 2];
    }
    float best = __builtin_inff();
    for (long long base = t0; base < t1; base += WN_TILE) {
        const int n = t1 - base < WN_TILE ? (int)(t1 - base) : WN_TILE;
        __syncthreads();
        stage_tile(tv, base, n, tile);
        __syncthreads();
        if (live) {
#pragma unroll 2
            for (int j = 0; j < n; ++j) {
                float4 a = tile[3 * j], b = tile[3 * j + 1], c = tile[3 * j + 2];
                a.x -= px, a.y -= py, a.z -= pz;
                b.x -= px, b.y -= py, b.z -= pz;
                c.x -= px, c.y -= py, c.z -= pz;
                best = fminf(best, tri_dist2(a, b, c));
            }
        }
    }
    if (live) partial[(long long)blockIdx.y * n_points + p] = best;
}

__global__ void __launch_bounds__(WN_THREADS) k_cd_combine(int n_points, const float* __restrict__ partial, int n_splits, float* __restrict__ dist) {
    const int p = blockIdx.x * WN_THREADS + threadIdx.x;
    if (p >= n_points) return;
    float m = __builtin_inff();
    for (int k = 0; k < n_splits; ++k) m = fminf(m, partial[(long long)k * n_points + p]);
    dist[p] = sqrtf(m);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct VoxLayout {
    long long nb = 0;
    size_t cnt = 0, blk = 0, off = 0, totals = 0, bytes = 0;
};

int vox_layout(long long n_tris, VoxLayout& L) {
    HN_REQUIRE(n_tris >= 0 && n_tris < (1LL << 31) - VOX_THREADS, "hn_voxelize: n_tris = %lld outside [0, 2^31 - 256)", n_tris);
    L.nb = (n_tris + VOX_THREADS - 1) / VOX_THREADS;
    size_t at = 0;
    L.cnt = at, at = align256(at + sizeof(int) * n_tris);
    L.blk = at, at = align256(at + sizeof(int) * 3 * L.nb);
    L.off = at, at = align256(at + sizeof(long long) * L.nb);
    L.totals = at, at = align256(at + sizeof(long long) * 3);
    L.bytes = at;
    return HN_OK;
}

int interact_sizes(long long n_points, long long n_tris, Split& s, size_t& bytes) {
    HN_REQUIRE(n_points >= 0 && n_points < (1LL << 31) - WN_THREADS, "hn_interact: n_points = %lld outside [0, 2^31 - 256)", n_points);
    HN_REQUIRE(n_tris >= 0 && n_tris < (1LL << 31) - WN_TILE, "hn_interact: n_tris = %lld outside [0, 2^31 - 256)", n_tris);
    s = split_of(n_points, n_tris);
    bytes = align256(sizeof(float) * (size_t)s.n_splits * (size_t)n_points);
    if (bytes < 256) bytes = 256;
    return HN_OK;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_voxelize_workspace_bytes(long long n_tris) {
    VoxLayout L;
    return vox_layout(n_tris, L) == HN_OK ? (L.bytes > 256 ? L.bytes : 256) : 0;
}

int hn_voxelize_count(const double* tri_verts, long long n_tris, double pitch, long long* n_keys, void* workspace, size_t workspace_bytes,
                      hn_stream_t stream) {
    VoxLayout L;
    HN_TRY_RC(vox_layout(n_tris, L));
    HN_REQUIRE(n_keys, "hn_voxelize_count: NULL n_keys");
    HN_REQUIRE(pitch > 0.0 && pitch < 1e300, "hn_voxelize_count: pitch must be positive and finite, got %g", pitch);
    *n_keys = 0;
    if (n_tris == 0) return HN_OK;
    HN_REQUIRE(tri_verts && workspace, "hn_voxelize_count: NULL tri_verts / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_voxelize_count: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_voxelize_count: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int* blk = (int*)(ws + L.blk);
    long long* totals = (long long*)(ws + L.totals);
    k_vox_count<<<(unsigned)L.nb, VOX_THREADS, 0, s>>>(tri_verts, (int)n_tris, pitch, (int*)(ws + L.cnt), blk);
    HN_LAUNCH_CHECK();
    k_vox_scan<<<1, VOX_SCAN_THREADS, 0, s>>>(blk, (int)L.nb, (long long*)(ws + L.off), totals);
    HN_LAUNCH_CHECK();
    long long h[3] = {0, 0, 0};
    HN_CHECK_HIP(hipMemcpyAsync(h, totals, sizeof(h), hipMemcpyDeviceToHost, s));
    HN_CHECK_HIP(hipStreamSynchronize(s));
    HN_REQUIRE(h[1] == 0, "hn_voxelize_count: %lld triangle(s) still have an edge longer than pitch / 2 = %g after %d rounds of splitting "
               "(trimesh's max_iter)", h[1], pitch / 2.0, VOX_MAX_ROUNDS);
    HN_REQUIRE(h[2] == 0, "hn_voxelize_count: %lld triangle(s) have a vertex with |v / pitch| >= %.0f (or not finite): its key does not "
               "fit 21 bits", h[2], VOX_KEY_LIMIT);
    *n_keys = h[0];
    return HN_OK;
}

int hn_voxelize_emit(const double* tri_verts, long long n_tris, double pitch, void* workspace, size_t workspace_bytes, long long n_keys,
                     long long* keys, hn_stream_t stream) {
    VoxLayout L;
    HN_TRY_RC(vox_layout(n_tris, L));
    HN_REQUIRE(pitch > 0.0 && pitch < 1e300, "hn_voxelize_emit: pitch must be positive and finite, got %g", pitch);
    HN_REQUIRE(n_keys >= 0, "hn_voxelize_emit: n_keys = %lld", n_keys);
    if (n_tris == 0 || n_keys == 0) return HN_OK;
    HN_REQUIRE(tri_verts && workspace && keys, "hn_voxelize_emit: NULL tri_verts / workspace / keys");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_voxelize_emit: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    char* ws = (char*)workspace;
    k_vox_emit<<<(unsigned)L.nb, VOX_THREADS, 0, (hipStream_t)stream>>>(tri_verts, (int)n_tris, pitch, (const int*)(ws + L.cnt),
                                                                         (const long long*)(ws + L.off), keys, n_keys);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

size_t hn_interact_workspace_bytes(long long n_points, long long n_tris) {
    Split sp;
    size_t bytes = 0;
    return interact_sizes(n_points, n_tris, sp, bytes) == HN_OK ? bytes : 0;
}

int hn_winding_contains(const float* points, long long n_points, const float* tri_verts, long long n_tris, const float* bbox,
                        unsigned char* inside, float* winding, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    Split sp;
    size_t need = 0;
    HN_TRY_RC(interact_sizes(n_points, n_tris, sp, need));
    if (n_points == 0 || n_tris == 0) return HN_OK;      // nothing to launch: the caller fills the outputs
    HN_REQUIRE(points && tri_verts && bbox && inside && workspace, "hn_winding_contains: NULL points / tri_verts / bbox / inside / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_winding_contains: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n_points + WN_THREADS - 1) / WN_THREADS);
    float* partial = (float*)workspace;
    k_wn_partial<<<dim3(nb, (unsigned)sp.n_splits), WN_THREADS, 0, s>>>(points, (int)n_points, tri_verts, (int)n_tris, sp.tris_per_split, bbox,
                                                                        partial);
    HN_LAUNCH_CHECK();
    k_wn_combine<<<nb, WN_THREADS, 0, s>>>(points, (int)n_points, bbox, partial, sp.n_splits, inside, winding);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_closest_distance(const float* points, long long n_points, const float* tri_verts, long long n_tris, float* dist, void* workspace,
                        size_t workspace_bytes, hn_stream_t stream) {
    Split sp;
    size_t need = 0;
    HN_TRY_RC(interact_sizes(n_points, n_tris, sp, need));
    if (n_points == 0 || n_tris == 0) return HN_OK;
    HN_REQUIRE(points && tri_verts && dist && workspace, "hn_closest_distance: NULL points / tri_verts / dist / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_closest_distance: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n_points + WN_THREADS - 1) / WN_THREADS);
    float* partial = (float*)workspace;
    k_cd_partial<<<dim3(nb, (unsigned)sp.n_splits), WN_THREADS, 0, s>>>(points, (int)n_points, tri_verts, (int)n_tris, sp.tris_per_split,
                                                                        partial);
    HN_LAUNCH_CHECK();
    k_cd_combine<<<nb, WN_THREADS, 0, s>>>((int)n_points, partial, sp.n_splits, dist);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
