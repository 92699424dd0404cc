// Pose-accuracy metrics on the device: what analys_results/analys_hand_obj_pose.py and analys_results/analys_acc_err.py compute on
// the CPU, frame by frame, from the pose pickles of fitting_single.py (a scipy cKDTree per frame and method for ADD-S).
// tests/test_pose_metrics_cpu.py restates both scripts in float64 numpy; DESIGN.md 3.15 is the contract.
//
// Five calls, all on device pointers, outputs and workspace supplied by the caller, no synchronisation, no allocation, no atomics
// (every reduction combines its partials in a fixed order: a repeated call gives the same bits):
//   transform  model vertices [V, 3] pushed through F poses, R_f v + t_f - c_f, evaluated in fp64 and rounded ONCE to fp32.  With
//              c_f the ground-truth translation the stored coordinates are object-sized (0.1 m, ulp 7e-9 m) instead of
//              camera-sized (1 m, ulp 6e-8 m), and the fp32 differences the later passes take lose nothing that matters.
//   nearest    per frame, the distance from each query to its nearest target: brute force over F x Nq x Nt pairs, the squared
//              distance from coordinate differences fma(dz, dz, fma(dy, dy, dx * dx)) (never |q|^2 + |t|^2 - 2 q.t, which cancels),
//              one sqrt per query at the end.
//   paired     the row-wise |a - b| (ADD, the vertex error, the joint error); differences and norm in fp64, rounded once.
//   row_mean   [F, N] fp32 -> [F] fp64 means, accumulated in fp64 in a fixed tree.
//   accel      compute_error_accel: mean_j |(p[i] - 2 p[i+1] + p[i+2]) - (g[i] - 2 g[i+1] + g[i+2])| in fp64.
//
// Passes:
//   k_pm_transform    one thread per (frame, vertex)
//   k_pm_nn_partial   a workgroup owns PM_QPW queries of one frame (PM_QPT per lane, in registers) x a range of the targets
//                     (blockIdx.y); target tiles are staged in LDS as three float arrays, every lane reads the same four targets in
//                     the same instruction (a broadcast, no bank conflict); one running minimum per query and range.  A short last
//                     tile is padded with its own first target, which changes no minimum.
//   k_pm_nn_combine   per query: minimum over the ranges -> sqrt
//   k_pm_paired       one thread per (frame, point)
//   k_pm_row_mean     one workgroup per row: a per-thread strided fp64 sum, a shuffle tree per wave, the waves in order
//   k_pm_accel        one workgroup per entry i, the same reduction over j
#include "hn_common.h"

namespace hn {
namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_QPT = 4;                              // queries per lane
constexpr int PM_QPW = PM_THREADS * PM_QPT;            // queries per workgroup
constexpr int PM_TILE = 512;                           // targets per LDS tile (3 x 2 KB)
constexpr long long PM_TARGET_BLOCKS = 1024;           // 256 CUs x 4 workgroups: split the targets until the grid has about this many
constexpr long long PM_MAX = (1LL << 31) - PM_QPW;     // counts (and frames x count) below this: block and point indices fit an int

struct PmSplit {
    int n_splits, per_split;
    long long q_blocks;                                // query blocks per frame
};

PmSplit pm_split_of(long long n_frames, long long n_queries, long long n_targets) {
    PmSplit r;
    r.q_blocks = (n_queries + PM_QPW - 1) / PM_QPW;
    const long long nb = n_frames * r.q_blocks;
    const long long tiles = (n_targets + PM_TILE - 1) / PM_TILE;
    long long s = (PM_TARGET_BLOCKS + nb - 1) / nb;
    s = s < 1 ? 1 : s > tiles ? tiles : s;
    const long long tiles_per = (tiles + s - 1) / s;
    r.per_split = (int)(tiles_per * PM_TILE);
    r.n_splits = (int)((n_targets + r.per_split - 1) / r.per_split);
    return r;
}

int pm_sizes(const char* who, long long n_frames, long long n_queries, long long n_targets, PmSplit& s, size_t& bytes) {
    HN_REQUIRE(n_frames > 0 && n_queries > 0 && n_targets > 0, "%s: n_frames = %lld, n_queries = %lld, n_targets = %lld: all must be positive",
               who, n_frames, n_queries, n_targets);
    HN_REQUIRE(n_frames < PM_MAX && n_queries < PM_MAX && n_targets < PM_MAX && n_frames * n_queries < PM_MAX && n_frames * n_targets < PM_MAX,
               "%s: n_frames = %lld, n_queries = %lld, n_targets = %lld: frames x points must stay below 2^31 - %d", who, n_frames, n_queries,
               n_targets, PM_QPW);
    s = pm_split_of(n_frames, n_queries, n_targets);
    HN_REQUIRE(s.n_splits >= 1 && s.n_splits <= 65535, "%s: %d target ranges", who, s.n_splits);
    bytes = (sizeof(float) * (size_t)s.n_splits * (size_t)(n_frames * n_queries) + 255) & ~(size_t)255;
    return HN_OK;
}

int pm_flat(const char* who, long long n_rows, long long n_cols) {
    HN_REQUIRE(n_rows > 0 && n_cols > 0, "%s: %lld x %lld: both counts must be positive", who, n_rows, n_cols);
    HN_REQUIRE(n_rows < PM_MAX && n_cols < PM_MAX && n_rows * n_cols < PM_MAX, "%s: %lld x %lld: rows x points must stay below 2^31 - %d", who,
               n_rows, n_cols, PM_QPW);
    return HN_OK;
}

// ---- transform ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PM_THREADS) k_pm_transform(const float* __restrict__ verts, int n_verts, const float* __restrict__ R,
                                                             const float* __restrict__ t, const float* __restrict__ c, int n_frames,
                                                             float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= (long long)n_frames * n_verts) return;
    const int f = (int)(i / n_verts), v = (int)(i - (long long)f * n_verts);
    const double x = verts[3LL * v], y = verts[3LL * v + 1], z = verts[3LL * v + 2];
    const float* Rf = R + 9LL * f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double rv = ((double)Rf[3 * d] * x + (double)Rf[3 * d + 1] * y) + (double)Rf[3 * d + 2] * z;
        out[3 * i + d] = (float)(rv + ((double)t[3LL * f + d] - (double)c[3LL * f + d]));
    }
}

// ---- nearest -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PM_THREADS) k_pm_nn_partial(const float* __restrict__ q, int n_queries, const float* __restrict__ tg,
                                                              int n_targets, int q_blocks, int per_split, float* __restrict__ partial,
                                                              long long n_all) {
    __shared__ __attribute__((aligned(16))) float tx[PM_TILE], ty[PM_TILE], tz[PM_TILE];
    const int f = blockIdx.x / q_blocks, qb = blockIdx.x - f * q_blocks;
    const float* qf = q + 3LL * f * n_queries;
    const float* tf = tg + 3LL * f * n_targets;
    const long long t0 = (long long)blockIdx.y * per_split;
    const long long t1 = t0 + per_split < n_targets ? t0 + per_split : n_targets;
    float qx[PM_QPT], qy[PM_QPT], qz[PM_QPT], best[PM_QPT];
#pragma unroll
    for (int k = 0; k < PM_QPT; ++k) {
        const int p = qb * PM_QPW + k * PM_THREADS + threadIdx.x;
        const bool live = p < n_queries;
        qx[k] = live ? qf[3LL * p] : 0.f;
        qy[k] = live ? qf[3LL * p + 1] : 0.f;
        qz[k] = live ? qf[3LL * p + 2] : 0.f;
        best[k] = __builtin_inff();
    }
    for (long long base = t0; base < t1; base += PM_TILE) {
        const int n = t1 - base < PM_TILE ? (int)(t1 - base) : PM_TILE;
        const int n4 = (n + 3) & ~3;                      // <= PM_TILE
        __syncthreads();                                  // the previous tile is consumed
        for (int j = threadIdx.x; j < n4; j += PM_THREADS) {
            const float* s = tf + 3LL * (base + (j < n ? j : 0));    // the tail repeats the tile's first target
            tx[j] = s[0];
            ty[j] = s[1];
            tz[j] = s[2];
        }
        __syncthreads();
        for (int j = 0; j < n4; j += 4) {
            const float4 ax = *(const float4*)(tx + j), ay = *(const float4*)(ty + j), az = *(const float4*)(tz + j);
            const float sx[4] = {ax.x, ax.y, ax.z, ax.w}, sy[4] = {ay.x, ay.y, ay.z, ay.w}, sz[4] = {az.x, az.y, az.z, az.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int k = 0; k < PM_QPT; ++k) {
                    const float dx = qx[k] - sx[u], dy = qy[k] - sy[u], dz = qz[k] - sz[u];
                    best[k] = fminf(best[k], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PM_QPT; ++k) {
        const int p = qb * PM_QPW + k * PM_THREADS + threadIdx.x;
        if (p < n_queries) partial[(long long)blockIdx.y * n_all + (long long)f * n_queries + p] = best[k];
    }
}

__global__ void __launch_bounds__(PM_THREADS) k_pm_nn_combine(long long n_all, const float* __restrict__ partial, int n_splits,
                                                              float* __restrict__ dist) {
    const long long p = (long long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (p >= n_all) return;
    float m = __builtin_inff();
    for (int k = 0; k < n_splits; ++k) m = fminf(m, partial[(long long)k * n_all + p]);
    dist[p] = sqrtf(m);
}

// ---- paired ------------------------------------------------------------------------------------------------------------------------
__device__ inline double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ void __launch_bounds__(PM_THREADS) k_pm_paired(const float* __restrict__ a, const float* __restrict__ b, long long n_all,
                                                          float* __restrict__ dist) {
    const long long p = (long long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (p >= n_all) return;
    dist[p] = (float)norm3((double)a[3 * p] - (double)b[3 * p], (double)a[3 * p + 1] - (double)b[3 * p + 1],
                           (double)a[3 * p + 2] - (double)b[3 * p + 2]);
}

// ---- reductions --------------------------------------------------------------------------------------------------------------------
// the workgroup's sum of one fp64 per thread, in a fixed order: a butterfly per wave, then the waves 0 .. 3; valid in thread 0
__device__ inline double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < PM_THREADS / 64; ++w) s += red[w];
    return s;
}

__global__ void __launch_bounds__(PM_THREADS) k_pm_row_mean(const float* __restrict__ x, int n, double* __restrict__ mean) {
    __shared__ double red[PM_THREADS / 64];
    const float* row = x + (long long)blockIdx.x * n;
    double acc = 0.0;
    for (int j = threadIdx.x; j < n; j += PM_THREADS) acc += (double)row[j];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) mean[blockIdx.x] = s / (double)n;
}

__global__ void __launch_bounds__(PM_THREADS) k_pm_accel(const float* __restrict__ gt, const float* __restrict__ pred, int n_points,
                                                         double* __restrict__ out) {
    __shared__ double red[PM_THREADS / 64];
    const long long s0 = 3LL * blockIdx.x * n_points, s1 = s0 + 3LL * n_points, s2 = s1 + 3LL * n_points;    // frames i, i + 1, i + 2
    double acc = 0.0;
    for (int j = threadIdx.x; j < n_points; j += PM_THREADS) {
        double d[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const long long o = 3LL * j + u;
            const double ap = ((double)pred[s0 + o] - 2.0 * (double)pred[s1 + o]) + (double)pred[s2 + o];
            const double ag = ((double)gt[s0 + o] - 2.0 * (double)gt[s1 + o]) + (double)gt[s2 + o];
            d[u] = ap - ag;
        }
        acc += norm3(d[0], d[1], d[2]);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s / (double)n_points;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_pm_workspace_bytes(long long n_frames, long long n_queries, long long n_targets) {
    PmSplit sp;
    size_t bytes = 0;
    return pm_sizes("hn_pm_workspace_bytes", n_frames, n_queries, n_targets, sp, bytes) == HN_OK ? bytes : 0;
}

int hn_pm_transform(const float* verts, long long n_verts, const float* R, const float* t, const float* c, long long n_frames, float* out,
                    hn_stream_t stream) {
    HN_TRY_RC(pm_flat("hn_pm_transform", n_frames, n_verts));
    HN_REQUIRE(verts && R && t && c && out, "hn_pm_transform: NULL verts / R / t / c / out");
    const long long n_all = n_frames * n_verts;
    k_pm_transform<<<(unsigned)((n_all + PM_THREADS - 1) / PM_THREADS), PM_THREADS, 0, (hipStream_t)stream>>>(verts, (int)n_verts, R, t, c,
                                                                                                              (int)n_frames, out);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_pm_nearest(const float* queries, long long n_queries, const float* targets, long long n_targets, long long n_frames, float* dist,
                  void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    PmSplit sp;
    size_t need = 0;
    HN_TRY_RC(pm_sizes("hn_pm_nearest", n_frames, n_queries, n_targets, sp, need));
    HN_REQUIRE(queries && targets && dist && workspace, "hn_pm_nearest: NULL queries / targets / dist / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_pm_nearest: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 3) == 0, "hn_pm_nearest: workspace not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n_all = n_frames * n_queries;
    float* partial = (float*)workspace;
    k_pm_nn_partial<<<dim3((unsigned)(n_frames * sp.q_blocks), (unsigned)sp.n_splits), PM_THREADS, 0, s>>>(
        queries, (int)n_queries, targets, (int)n_targets, (int)sp.q_blocks, sp.per_split, partial, n_all);
    HN_LAUNCH_CHECK();
    k_pm_nn_combine<<<(unsigned)((n_all + PM_THREADS - 1) / PM_THREADS), PM_THREADS, 0, s>>>(n_all, partial, sp.n_splits, dist);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_pm_paired(const float* a, const float* b, long long n_frames, long long n_points, float* dist, hn_stream_t stream) {
    HN_TRY_RC(pm_flat("hn_pm_paired", n_frames, n_points));
    HN_REQUIRE(a && b && dist, "hn_pm_paired: NULL a / b / dist");
    const long long n_all = n_frames * n_points;
    k_pm_paired<<<(unsigned)((n_all + PM_THREADS - 1) / PM_THREADS), PM_THREADS, 0, (hipStream_t)stream>>>(a, b, n_all, dist);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_pm_row_mean(const float* x, long long n_rows, long long n_cols, double* mean, hn_stream_t stream) {
    HN_TRY_RC(pm_flat("hn_pm_row_mean", n_rows, n_cols));
    HN_REQUIRE(x && mean, "hn_pm_row_mean: NULL x / mean");
    k_pm_row_mean<<<(unsigned)n_rows, PM_THREADS, 0, (hipStream_t)stream>>>(x, (int)n_cols, mean);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_pm_accel(const float* gt, const float* pred, long long n_frames, long long n_points, double* accel, hn_stream_t stream) {
    HN_REQUIRE(n_frames >= 3, "hn_pm_accel: n_frames = %lld: the second difference needs at least 3 frames", n_frames);
    HN_TRY_RC(pm_flat("hn_pm_accel", n_frames, n_points));
    HN_REQUIRE(gt && pred && accel, "hn_pm_accel: NULL gt / pred / accel");
    k_pm_accel<<<(unsigned)(n_frames - 2), PM_THREADS, 0, (hipStream_t)stream>>>(gt, pred, (int)n_points, accel);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
