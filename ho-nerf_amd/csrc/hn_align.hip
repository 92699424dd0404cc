// Rigid and similarity alignment of paired point clouds on the device: the weighted moments of two clouds, the best proper rotation
// (and scale) from them, and the transform applied and composed.  What a caller otherwise leaves the device for (scipy's
// orthogonal_procrustes, trimesh.registration.procrustes / icp, open3d's registration).  tests/alignment_cases.py restates every call
// in float64 numpy, twice (SVD with the determinant correction, Horn's quaternion); DESIGN.md 3.28 is the contract.
//
// Four calls, all on device pointers, outputs and workspace supplied by the caller, no synchronisation, no allocation, no atomics:
//   moments   src, dst [F, N, 3] fp32, weight [F, N] fp32 or NULL (= 1) -> [F, 18] fp64: W, ca[3], cb[3], H[9], va, vb with
//             ca = sum w a / W, H = sum w (b - cb)(a - ca)^T, va = sum w |a - ca|^2.  Two passes, centroids first, then the centred second
//             moments from differences taken in fp64: a cloud a few centimetres across at camera distance loses nothing to
//             cancellation.  The summation tree is fixed by N alone: the points are cut into chunks of AL_CHUNK; a wave owns one chunk
//             of one frame, lane l adds the chunk's points l, l + 64, ... in that order, the 64 lane sums meet in an xor butterfly
//             (32, 16, ... 1), and a frame's chunk sums are added in chunk order.  Neither F, nor the grid, nor the frames that
//             share a launch enter: a frame alone and the same frame among others give the same bits, and so do weight = NULL and
//             explicit ones (1.0 * x is x).
//   solve     moments -> R [F, 3, 3], s [F], t [F, 3] fp64, rank [F] int32: Horn's closed form (JOSA A 4, 1987).  The unit quaternion
//             of the best rotation is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix that is LINEAR in H
//             (H^T H, which squares the condition number, is never formed), found by cyclic Jacobi rotations in fp64, at most
//             AL_SWEEPS sweeps.  The rotation is proper by construction: there is no determinant fix-up, and the gap between the two
//             largest eigenvalues, 2 (sigma_2 + det sign * sigma_3) in H's singular values, says how well it is determined.
//   apply     pts [F, N, 3] fp32 -> (float)(s (R p) + t), evaluated in fp64 and rounded once; one transform may serve every frame.
//   compose   (R2, s2, t2) o (R1, s1, t1) = (R2 R1, s2 s1, s2 R2 t1 + t2) in fp64.
//
// Passes:
//   k_align_moments   4 waves per workgroup, each wave its own (frame, chunk) item: no barrier, no LDS, and a launch over thousands of
//                     frames of 21 points idles at most 3 waves, in its last workgroup.  phase 0 (N <= AL_CHUNK: one chunk per frame)
//                     makes both passes and writes the 18 moments; phase 1 / 2 (more chunks) write the chunk sums of the first /
//                     second pass to the workspace
//   k_align_combine   one thread per frame adds the chunk sums in chunk order -> W, ca, cb (phase 1) or H, va, vb (phase 2)
//   k_align_solve     one thread per frame
//   k_align_apply     one thread per point
//   k_align_compose   one thread per frame
#include "hn_common.h"

namespace hn {
namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_WAVES = AL_THREADS / 64;
constexpr int AL_CHUNK = 1024;                         // points per wave: 16 per lane.  honerf_amd.alignment.CHUNK restates it
constexpr int AL_N1 = 7, AL_N2 = 11;                   // sums of the first pass (W, W ca, W cb) and of the second (H, va, vb)
constexpr int AL_SWEEPS = 24;                          // Jacobi converges quadratically: 6 to 8 sweeps in practice, the bound is never met
constexpr long long AL_MAX = (1LL << 31) - AL_CHUNK;   // frames x points below this: every index fits an int
constexpr double AL_RANK_TOL = 1e-10;

struct AlSplit {
    int n_chunks;
    long long n_items;                                 // frames x chunks
};

int al_sizes(const char* who, long long n_frames, long long n_points, AlSplit& s, size_t& bytes) {
    HN_REQUIRE(n_frames > 0 && n_points > 0, "%s: n_frames = %lld, n_points = %lld: both must be positive", who, n_frames, n_points);
    HN_REQUIRE(n_frames < AL_MAX && n_points < AL_MAX && n_frames * n_points < AL_MAX,
               "%s: n_frames = %lld, n_points = %lld: frames x points must stay below 2^31 - %d", who, n_frames, n_points, AL_CHUNK);
    s.n_chunks = (int)((n_points + AL_CHUNK - 1) / AL_CHUNK);
    s.n_items = n_frames * s.n_chunks;
    // the chunk sums of the two passes (one chunk: nothing is staged, the minimum is returned so that 0 keeps meaning "refused")
    bytes = s.n_chunks > 1 ? (sizeof(double) * (size_t)s.n_items * (AL_N1 + AL_N2) + 255) & ~(size_t)255 : 256;
    return HN_OK;
}

template <int K>
__device__ inline void wave_sum(double (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    }
}

// the centroids from the first pass's sums; a frame without weight has none: 0, and every centred moment is then 0 too
__device__ inline void al_centroids(const double (&s)[AL_N1], double (&ca)[3], double (&cb)[3]) {
    const bool has = s[0] > 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ca[d] = has ? s[1 + d] / s[0] : 0.0;
        cb[d] = has ? s[4 + d] / s[0] : 0.0;
    }
}

__global__ void __launch_bounds__(AL_THREADS) k_align_moments(const float* __restrict__ src, const float* __restrict__ dst,
                                                              const float* __restrict__ weight, int n_points, int n_chunks, long long n_items,
                                                              int phase, double* __restrict__ part1, double* __restrict__ part2,
                                                              double* __restrict__ moments) {
    const long long item = (long long)blockIdx.x * AL_WAVES + (threadIdx.x >> 6);      // the same for the whole wave
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const long long f = item / n_chunks;
    const int c = (int)(item - f * n_chunks);
    const int p0 = c * AL_CHUNK;
    const int n = n_points - p0 < AL_CHUNK ? n_points - p0 : AL_CHUNK;
    const long long base = f * n_points + p0;
    const float* a = src + 3 * base;
    const float* b = dst + 3 * base;
    const float* w = weight ? weight + base : nullptr;
    double ca[3], cb[3];
    double s1[AL_N1];
    if (phase != 2) {
#pragma unroll
        for (int k = 0; k < AL_N1; ++k) s1[k] = 0.0;
        for (int j = lane; j < n; j += 64) {
            const double wt = w ? (double)w[j] : 1.0;
            s1[0] += wt;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                s1[1 + d] += wt * (double)a[3 * j + d];
                s1[4 + d] += wt * (double)b[3 * j + d];
            }
        }
        wave_sum(s1);
        if (phase == 1) {
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < AL_N1; ++k) part1[item * AL_N1 + k] = s1[k];
            }
            return;
        }
        al_centroids(s1, ca, cb);
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            ca[d] = moments[f * 18 + 1 + d];
            cb[d] = moments[f * 18 + 4 + d];
        }
    }
    double s2[AL_N2];
#pragma unroll
    for (int k = 0; k < AL_N2; ++k) s2[k] = 0.0;
    for (int j = lane; j < n; j += 64) {
        const double wt = w ? (double)w[j] : 1.0;
        double da[3], db[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            da[d] = (double)a[3 * j + d] - ca[d];
            db[d] = (double)b[3 * j + d] - cb[d];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double wb = wt * db[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) s2[3 * i + k] += wb * da[k];
        }
        s2[9] += wt * ((da[0] * da[0] + da[1] * da[1]) + da[2] * da[2]);
        s2[10] += wt * ((db[0] * db[0] + db[1] * db[1]) + db[2] * db[2]);
    }
    wave_sum(s2);
    if (lane != 0) return;
    if (phase == 0) {
        double* m = moments + f * 18;
        m[0] = s1[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            m[1 + d] = ca[d];
            m[4 + d] = cb[d];
        }
#pragma unroll
        for (int k = 0; k < AL_N2; ++k) m[7 + k] = s2[k];
    } else {
#pragma unroll
        for (int k = 0; k < AL_N2; ++k) part2[item * AL_N2 + k] = s2[k];
    }
}

__global__ void __launch_bounds__(AL_THREADS) k_align_combine(int phase, int n_chunks, int n_frames, const double* __restrict__ part,
                                                              double* __restrict__ moments) {
    const int f = blockIdx.x * AL_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    double* m = moments + 18LL * f;
    if (phase == 1) {
        const double* p = part + (long long)f * n_chunks * AL_N1;
        double s[AL_N1], ca[3], cb[3];
#pragma unroll
        for (int k = 0; k < AL_N1; ++k) s[k] = p[k];
        for (int c = 1; c < n_chunks; ++c) {
#pragma unroll
            for (int k = 0; k < AL_N1; ++k) s[k] += p[(long long)c * AL_N1 + k];
        }
        al_centroids(s, ca, cb);
        m[0] = s[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            m[1 + d] = ca[d];
            m[4 + d] = cb[d];
        }
    } else {
        const double* p = part + (long long)f * n_chunks * AL_N2;
        double s[AL_N2];
#pragma unroll
        for (int k = 0; k < AL_N2; ++k) s[k] = p[k];
        for (int c = 1; c < n_chunks; ++c) {
#pragma unroll
            for (int k = 0; k < AL_N2; ++k) s[k] += p[(long long)c * AL_N2 + k];
        }
#pragma unroll
        for (int k = 0; k < AL_N2; ++k) m[7 + k] = s[k];
    }
}

// ---- solve -------------------------------------------------------------------------------------------------------------------------
// One Jacobi rotation of the symmetric A (and of the eigenvector columns V) that annihilates A[P][Q]; Rutishauser's update, as in
// Numerical Recipes' jacobi: t is the smaller root, and an entry that no longer changes its diagonals in fp64 is set to zero.
template <int P, int Q>
__device__ inline void al_rotate(double (&A)[4][4], double (&V)[4][4], double& off) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    if (fabs(A[P][P]) + g == fabs(A[P][P]) && fabs(A[Q][Q]) + g == fabs(A[Q][Q])) {
        A[P][Q] = A[Q][P] = 0.0;
        return;
    }
    off += fabs(apq);
    const double h = A[Q][Q] - A[P][P];
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double x = A[r][P], y = A[r][Q];
            A[r][P] = A[P][r] = x - s * (y + x * tau);
            A[r][Q] = A[Q][r] = y + s * (x - y * tau);
        }
        const double vx = V[r][P], vy = V[r][Q];
        V[r][P] = vx - s * (vy + vx * tau);
        V[r][Q] = vy + s * (vx - vy * tau);
    }
}

__global__ void __launch_bounds__(AL_THREADS) k_align_solve(const double* __restrict__ moments, int n_frames, int with_scale,
                                                            double* __restrict__ R_out, double* __restrict__ s_out, double* __restrict__ t_out,
                                                            int* __restrict__ rank_out) {
    const int f = blockIdx.x * AL_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const double* m = moments + 18LL * f;
    const double W = m[0], va = m[16], vb = m[17];
    const double* H = m + 7;                              // H[3 i + k] = sum w (b - cb)_i (a - ca)_k = Horn's S_{k i}
    const double Sxx = H[0], Sxy = H[3], Sxz = H[6], Syx = H[1], Syy = H[4], Syz = H[7], Szx = H[2], Szy = H[5], Szz = H[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < AL_SWEEPS; ++sweep) {
        double off = 0.0;
        al_rotate<0, 1>(A, V, off);
        al_rotate<0, 2>(A, V, off);
        al_rotate<0, 3>(A, V, off);
        al_rotate<1, 2>(A, V, off);
        al_rotate<1, 3>(A, V, off);
        al_rotate<2, 3>(A, V, off);
        if (off == 0.0) break;
    }
    // the two largest eigenvalues; among equal ones the smaller index
    const double lam[4] = {A[0][0], A[1][1], A[2][2], A[3][3]};
    int i1 = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (lam[k] > lam[i1]) i1 = k;
    int i2 = i1 == 0 ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k != i1 && k != i2 && lam[k] > lam[i2]) i2 = k;
    double q[4], q2[4], l1 = 0.0, l2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == i1) {
            l1 = lam[k];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = V[r][k];
        }
        if (k == i2) {
            l2 = lam[k];
#pragma unroll
            for (int r = 0; r < 4; ++r) q2[r] = V[r][k];
        }
    }
    const double size = sqrt(va * vb);                    // every singular value of H is at most this
    int rank = 3;
    if (!(W > 0.0) || !(size > 0.0) || !(size < __builtin_inf()) || !(l1 > AL_RANK_TOL * size)) {
        rank = 0;                                         // H = 0 as far as fp64 can tell: every rotation is as good; the identity
        q[0] = 1.0;
        q[1] = q[2] = q[3] = 0.0;
    } else if (!(l1 - l2 > AL_RANK_TOL * l1)) {
        rank = 1;                                         // a plane of optimal quaternions: the one nearest the identity (the smallest angle)
        const double w1 = q[0], w2 = q2[0];
        if (w1 * w1 + w2 * w2 > 1e-24) {
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = w1 * q[r] + w2 * q2[r];
        }
    }
    {
        const double nq = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
        double sign = 1.0;                                // q and -q are the same rotation: the first entry that is not 0 is made positive
        if (q[0] < 0.0 || (q[0] == 0.0 && (q[1] < 0.0 || (q[1] == 0.0 && (q[2] < 0.0 || (q[2] == 0.0 && q[3] < 0.0)))))) sign = -1.0;
        const double inv = nq > 0.0 ? sign / nq : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] *= inv;
        if (!(nq > 0.0)) q[0] = 1.0;
    }
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    double R[9];
    R[0] = (qw * qw + qx * qx) - (qy * qy + qz * qz);
    R[1] = 2.0 * (qx * qy - qw * qz);
    R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz);
    R[4] = (qw * qw + qy * qy) - (qx * qx + qz * qz);
    R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy);
    R[7] = 2.0 * (qy * qz + qw * qx);
    R[8] = (qw * qw + qz * qz) - (qx * qx + qy * qy);
    double s = 1.0;
    if (with_scale && va > 0.0 && W > 0.0 && va < __builtin_inf()) {
        double tr = 0.0;                                  // sum w (b - cb) . R (a - ca)
#pragma unroll
        for (int k = 0; k < 9; ++k) tr += R[k] * H[k];
        s = tr > 0.0 ? tr / va : 0.0;
        if (!(s < __builtin_inf())) s = 1.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R_out[9LL * f + k] = R[k];
    s_out[f] = s;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double rc = (R[3 * d] * m[1] + R[3 * d + 1] * m[2]) + R[3 * d + 2] * m[3];
        const double t = m[4 + d] - s * rc;
        t_out[3LL * f + d] = t == t && fabs(t) < __builtin_inf() ? t : 0.0;
    }
    rank_out[f] = rank;
}

// ---- apply, compose ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AL_THREADS) k_align_apply(const float* __restrict__ pts, int n_points, long long n_all, const double* __restrict__ R,
                                                            const double* __restrict__ s, const double* __restrict__ t, int broadcast,
                                                            float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= n_all) return;
    const long long f = broadcast ? 0 : i / n_points;
    const double* Rf = R + 9 * f;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2], sf = s[f];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double rv = (Rf[3 * d] * x + Rf[3 * d + 1] * y) + Rf[3 * d + 2] * z;
        out[3 * i + d] = (float)(sf * rv + t[3 * f + d]);
    }
}

// (no __restrict__: the outputs may be either input; a frame's thread reads everything before it writes)
__global__ void __launch_bounds__(AL_THREADS) k_align_compose(const double* R2, const double* s2, const double* t2, const double* R1, const double* s1,
                                                              const double* t1, int n_frames, double* R, double* s, double* t) {
    const int f = blockIdx.x * AL_THREADS + threadIdx.x;
    if (f >= n_frames) return;
    const double* A = R2 + 9LL * f;
    const double* B = R1 + 9LL * f;
    double C[9], u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) C[3 * i + k] = (A[3 * i] * B[k] + A[3 * i + 1] * B[3 + k]) + A[3 * i + 2] * B[6 + k];
        u[i] = s2[f] * ((A[3 * i] * t1[3LL * f] + A[3 * i + 1] * t1[3LL * f + 1]) + A[3 * i + 2] * t1[3LL * f + 2]) + t2[3LL * f + i];
    }
    const double sc = s2[f] * s1[f];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[9LL * f + k] = C[k];
    s[f] = sc;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[3LL * f + i] = u[i];
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_align_workspace_bytes(long long n_frames, long long n_points) {
    AlSplit sp;
    size_t bytes = 0;
    return al_sizes("hn_align_workspace_bytes", n_frames, n_points, sp, bytes) == HN_OK ? bytes : 0;
}

int hn_align_chunk(void) { return AL_CHUNK; }

int hn_align_moments(const float* src, const float* dst, const float* weight, long long n_frames, long long n_points, double* moments,
                     void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    AlSplit sp;
    size_t need = 0;
    HN_TRY_RC(al_sizes("hn_align_moments", n_frames, n_points, sp, need));
    HN_REQUIRE(src && dst && moments && workspace, "hn_align_moments: NULL src / dst / moments / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_align_moments: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)moments & 7) == 0, "hn_align_moments: workspace or moments not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((sp.n_items + AL_WAVES - 1) / AL_WAVES);
    if (sp.n_chunks == 1) {
        k_align_moments<<<blocks, AL_THREADS, 0, s>>>(src, dst, weight, (int)n_points, 1, sp.n_items, 0, nullptr, nullptr, moments);
        HN_LAUNCH_CHECK();
        return HN_OK;
    }
    double* part1 = (double*)workspace;
    double* part2 = part1 + sp.n_items * AL_N1;
    const unsigned fb = (unsigned)((n_frames + AL_THREADS - 1) / AL_THREADS);
    k_align_moments<<<blocks, AL_THREADS, 0, s>>>(src, dst, weight, (int)n_points, sp.n_chunks, sp.n_items, 1, part1, part2, moments);
    HN_LAUNCH_CHECK();
    k_align_combine<<<fb, AL_THREADS, 0, s>>>(1, sp.n_chunks, (int)n_frames, part1, moments);
    HN_LAUNCH_CHECK();
    k_align_moments<<<blocks, AL_THREADS, 0, s>>>(src, dst, weight, (int)n_points, sp.n_chunks, sp.n_items, 2, part1, part2, moments);
    HN_LAUNCH_CHECK();
    k_align_combine<<<fb, AL_THREADS, 0, s>>>(2, sp.n_chunks, (int)n_frames, part2, moments);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_align_solve(const double* moments, long long n_frames, int with_scale, double* R, double* s, double* t, int* rank, hn_stream_t stream) {
    HN_REQUIRE(n_frames > 0 && n_frames < AL_MAX, "hn_align_solve: n_frames = %lld outside (0, 2^31 - %d)", n_frames, AL_CHUNK);
    HN_REQUIRE(moments && R && s && t && rank, "hn_align_solve: NULL moments / R / s / t / rank");
    k_align_solve<<<(unsigned)((n_frames + AL_THREADS - 1) / AL_THREADS), AL_THREADS, 0, (hipStream_t)stream>>>(moments, (int)n_frames,
                                                                                                                 with_scale ? 1 : 0, R, s, t, rank);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_align_apply(const float* pts, long long n_frames, long long n_points, const double* R, const double* s, const double* t,
                   long long n_transforms, float* out, hn_stream_t stream) {
    AlSplit sp;
    size_t bytes = 0;
    HN_TRY_RC(al_sizes("hn_align_apply", n_frames, n_points, sp, bytes));
    HN_REQUIRE(n_transforms == n_frames || n_transforms == 1, "hn_align_apply: %lld transforms for %lld frames: one for all, or one each", n_transforms,
               n_frames);
    HN_REQUIRE(pts && R && s && t && out, "hn_align_apply: NULL pts / R / s / t / out");
    const long long n_all = n_frames * n_points;
    k_align_apply<<<(unsigned)((n_all + AL_THREADS - 1) / AL_THREADS), AL_THREADS, 0, (hipStream_t)stream>>>(
        pts, (int)n_points, n_all, R, s, t, n_transforms == 1 && n_frames > 1 ? 1 : 0, out);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_align_compose(const double* R2, const double* s2, const double* t2, const double* R1, const double* s1, const double* t1, long long n_frames,
                     double* R, double* s, double* t, hn_stream_t stream) {
    HN_REQUIRE(n_frames > 0 && n_frames < AL_MAX, "hn_align_compose: n_frames = %lld outside (0, 2^31 - %d)", n_frames, AL_CHUNK);
    HN_REQUIRE(R2 && s2 && t2 && R1 && s1 && t1 && R && s && t, "hn_align_compose: NULL argument");
    k_align_compose<<<(unsigned)((n_frames + AL_THREADS - 1) / AL_THREADS), AL_THREADS, 0, (hipStream_t)stream>>>(R2, s2, t2, R1, s1, t1, (int)n_frames,
                                                                                                                   R, s, t);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
