// Geometry buffers of a fitted field pair (or one field): per ray the opacity, the un-normalised expected depth and the composited
// field gradient of each field, from the per-sample sdf / gradient a render hands back and its depths.  SDF -> alpha
// (alpha_sample, hn_scan.h: k_alpha's arithmetic), the transmittance scan and the per-ray sums are one kernel: alpha and the
// weights stay in registers: 36 B per ray-sample with two fields (2 x (4 sdf + 12 gradient) + 4 depth), 20 B with one; DESIGN.md 3.20
// has the measured rate and what else bounds it (2 expf and 3 divisions per sample and field).
//
//   dist_k = z_{k+1} - z_k (the last one sample_dist), m_k = z_k + dist_k / 2
//   two fields: T_k = prod_{j<k} (1 - a^h_j + 1e-7)(1 - a^o_j + 1e-7)    (utils/renderer.py:512-520)
//   one field:  T_k = c_0 prod_{j<k} (1 - a_j + 1e-7)                     (utils/renderer.py:163-164, SURVEY B-3)
//   w^f_k = a^f_k T_k;  opacity^f = sum_k w^f_k,  depth^f = sum_k w^f_k m_k,  normal^f = sum_k w^f_k grad^f_k
// The object's gradient is taken in the object's frame p' = Ro (p - To): its sum goes back to the world frame as Ro^T n.
// The second half of the file is the adjoint of this stage (hn_gbuffer1_bwd / hn_gbuffer2_bwd).
#include "hn_scan.h"

namespace hn {

struct GbArgs {
    const float* sdf[2];
    const float* grad[2];
    const float* dir[2];
    float inv_s[2];
    const float* z;
    const float* Ro;        // [n_frames, 3, 3] or NULL (two fields only)
    int n_rays, rays_per_frame, S;
    float sample_dist;
    float *opacity, *depth, *normal;
};

// what a ray's group of lanes (or wave) has summed for one ray, written by one lane: [N, NF], [N, NF], [N, NF, 3]
template <int NF>
__device__ __forceinline__ void gb_store(const GbArgs& p, int ray, const float (&op)[NF], const float (&dp)[NF], float (&nr)[NF][3]) {
    if (NF == 2 && p.normal != nullptr && p.Ro != nullptr) {
        const float* R = p.Ro + 9 * (size_t)(ray / p.rays_per_frame);
        const float x = nr[1][0], y = nr[1][1], z = nr[1][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) nr[1][k] = R[k] * x + R[3 + k] * y + R[6 + k] * z;    // Ro^T n
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (p.opacity != nullptr) p.opacity[(size_t)ray * NF + f] = op[f];
        if (p.depth != nullptr) p.depth[(size_t)ray * NF + f] = dp[f];
        if (p.normal != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p.normal[((size_t)ray * NF + f) * 3 + k] = nr[f][k];
        }
    }
}

// ---- S = 16 CPS: 16 lanes per ray, lane l owns samples l CPS .. l CPS + CPS - 1 (k_composite2_rows' layout) ---------------------
// A wave takes 4 consecutive rays and reads 4 S consecutive floats of every per-sample array with 16-byte loads, all of them issued
// before the first use (9 CPS / 4 per lane with two fields), one group of rays ahead.  A lane's last section ends at the first depth
// of the next lane (DPP row_shl:1) or, in the last lane, is sample_dist.  The transmittance is a sequential product inside the lane
// and an exclusive product scan over the 16 lanes, the per-ray sums are DPP butterflies.
template <int CPS, int NF>
__global__ __launch_bounds__(256) void k_gbuffer_rows(const GbArgs p) {
    constexpr int S = 16 * CPS;
    const int lane = threadIdx.x & 63, l = lane & 15, row = lane >> 4;
    const bool want_depth = p.depth != nullptr, want_normal = p.normal != nullptr;
    // the loads of a wave's NEXT group of rays are issued before the arithmetic of the current one (2 expf and 3 divisions per sample
    // and field: about as long as the loads take), so that a wave always has loads in flight
    float z[CPS], s[NF][CPS], gr[NF][3 * CPS], d[NF][3];
    float zn[CPS], sn[NF][CPS], grn[NF][3 * CPS], dn[NF][3];
    auto load = [&](int g, float (&z_)[CPS], float (&s_)[NF][CPS], float (&gr_)[NF][3 * CPS], float (&d_)[NF][3]) {
        const int ray = g * 4 + row;
        const int r = ray < p.n_rays ? ray : p.n_rays - 1;
        const size_t base = (size_t)r * S + l * CPS;
        load_run<CPS>(p.z + base, z_);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            load_run<CPS>(p.sdf[f] + base, s_[f]);
            load_run<3 * CPS>(p.grad[f] + 3 * base, gr_[f]);
#pragma unroll
            for (int k = 0; k < 3; ++k) d_[f][k] = p.dir[f][3 * (size_t)r + k];
        }
    };
    int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g * 4 < p.n_rays) load(g, zn, sn, grn, dn);
    for (; g * 4 < p.n_rays; g += gridDim.x * 4) {
        const int ray = g * 4 + row;
        const bool ok = ray < p.n_rays;
#pragma unroll
        for (int i = 0; i < CPS; ++i) z[i] = zn[i];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
            for (int i = 0; i < CPS; ++i) s[f][i] = sn[f][i];
#pragma unroll
            for (int i = 0; i < 3 * CPS; ++i) gr[f][i] = grn[f][i];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[f][k] = dn[f][k];
        }
        if ((g + gridDim.x * 4) * 4 < p.n_rays) load(g + gridDim.x * 4, zn, sn, grn, dn);
        const float z_next = dpp<0x101>(0.f, z[0]);       // row_shl:1: the first depth of lane l + 1
        float dist[CPS];
#pragma unroll
        for (int i = 0; i + 1 < CPS; ++i) dist[i] = z[i + 1] - z[i];
        dist[CPS - 1] = l == 15 ? p.sample_dist : z_next - z[CPS - 1];
        float P = 1.f, c_first = 1.f;
#pragma unroll
        for (int i = 0; i < CPS; ++i) {
            float fac = 1.f;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                float c;
                s[f][i] = alpha_sample(d[f][0], d[f][1], d[f][2], gr[f][3 * i], gr[f][3 * i + 1], gr[f][3 * i + 2], s[f][i], dist[i],
                                       p.inv_s[f], c);      // the sdf's register holds alpha from here on
                if (NF == 1 && i == 0) c_first = c;
                fac *= 1.f - s[f][i] + 1e-7f;
            }
            P *= fac;
        }
        float T = group_excl_prod<16>(P, l);
        if (NF == 1) T *= __shfl(c_first, lane & 48, 64);   // SURVEY B-3: the seed is c_0, lane 0 of the group has it
        float op[NF], dp[NF], nr[NF][3];
#pragma unroll
        for (int f = 0; f < NF; ++f) op[f] = dp[f] = nr[f][0] = nr[f][1] = nr[f][2] = 0.f;
#pragma unroll
        for (int i = 0; i < CPS; ++i) {
            const float m = z[i] + dist[i] * 0.5f;
            float fac = 1.f;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float w = s[f][i] * T;
                fac *= 1.f - s[f][i] + 1e-7f;
                op[f] += w;
                if (want_depth) dp[f] += w * m;
                if (want_normal) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) nr[f][k] += w * gr[f][3 * i + k];
                }
            }
            T *= fac;
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            op[f] = group_sum<16>(op[f]);
            if (want_depth) dp[f] = group_sum<16>(dp[f]);
            if (want_normal) {
#pragma unroll
                for (int k = 0; k < 3; ++k) nr[f][k] = group_sum<16>(nr[f][k]);
            }
        }
        if (ok && l == 0) gb_store<NF>(p, ray, op, dp, nr);
    }
}

// ---- every other S: one wave per ray, sample e = lane + 64 m (k_composite2's layout) --------------------------------------------
template <int NF>
__global__ __launch_bounds__(256) void k_gbuffer(const GbArgs p) {
    const int lane = threadIdx.x & 63, S = p.S;
    const bool want_depth = p.depth != nullptr, want_normal = p.normal != nullptr;
    for (int ray = blockIdx.x * 4 + (threadIdx.x >> 6); ray < p.n_rays; ray += gridDim.x * 4) {
        const size_t base = (size_t)ray * S;
        float d[NF][3];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d[f][k] = p.dir[f][3 * (size_t)ray + k];
        }
        float carry = 1.f;
        float op[NF], dp[NF], nr[NF][3];
#pragma unroll
        for (int f = 0; f < NF; ++f) op[f] = dp[f] = nr[f][0] = nr[f][1] = nr[f][2] = 0.f;
        for (int m0 = 0; m0 < S; m0 += 64) {
            const int e = m0 + lane;
            const bool ok = e < S;
            const size_t i = base + (ok ? e : S - 1);
            const float z = p.z[i];
            const float dist = (ok && e + 1 < S) ? p.z[i + 1] - z : p.sample_dist;
            const float m = z + dist * 0.5f;
            float a[NF], g[NF][3], fac = 1.f, c_mine = 1.f;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
#pragma unroll
                for (int k = 0; k < 3; ++k) g[f][k] = p.grad[f][3 * i + k];
                float c;
                a[f] = alpha_sample(d[f][0], d[f][1], d[f][2], g[f][0], g[f][1], g[f][2], p.sdf[f][i], dist, p.inv_s[f], c);
                if (!ok) a[f] = 0.f;
                if (NF == 1) c_mine = c;
                fac *= ok ? (1.f - a[f] + 1e-7f) : 1.f;
            }
            if (NF == 1 && m0 == 0) carry = __shfl(c_mine, 0, 64);     // SURVEY B-3: the first factor is c_0, not 1
            const float incl = wave_incl_prod(fac, lane);
            float excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 1.f;
            const float T = carry * excl;
            carry *= __shfl(incl, 63, 64);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float w = a[f] * T;       // 0 in the lanes behind the last sample
                op[f] += w;
                if (want_depth) dp[f] += w * m;
                if (want_normal) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) nr[f][k] += w * g[f][k];
                }
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            op[f] = wave_sum(op[f]);
            if (want_depth) dp[f] = wave_sum(dp[f]);
            if (want_normal) {
#pragma unroll
                for (int k = 0; k < 3; ++k) nr[f][k] = wave_sum(nr[f][k]);
            }
        }
        if (lane == 0) gb_store<NF>(p, ray, op, dp, nr);
    }
}

static bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int NF>
static int gbuffer_launch(const GbArgs& p, hipStream_t s) {
    bool rows = p.S % 64 == 0 && aligned16(p.z);
    for (int f = 0; f < NF; ++f) rows = rows && aligned16(p.sdf[f]) && aligned16(p.grad[f]);
    const int groups = (p.n_rays + 3) / 4;      // 4 rays per wave, 4 waves per block
    const dim3 rgrid((groups + 3) / 4 < 2048 ? (groups + 3) / 4 : 2048);
    if (rows && p.S == 64)
        hipLaunchKernelGGL((k_gbuffer_rows<4, NF>), rgrid, dim3(256), 0, s, p);
    else if (rows && p.S == 128)
        hipLaunchKernelGGL((k_gbuffer_rows<8, NF>), rgrid, dim3(256), 0, s, p);
    else if (rows && p.S == 192)
        hipLaunchKernelGGL((k_gbuffer_rows<12, NF>), rgrid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((k_gbuffer<NF>), dim3(composite_grid(p.n_rays)), dim3(256), 0, s, p);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int gbuffer1(const float* sdf, const float* grad, const float* rays_d, const float* z_vals, int n_rays, int S, float sample_dist,
             float inv_s, float* opacity, float* depth, float* normal, hipStream_t s) {
    HN_REQUIRE(S >= 1, "hn_gbuffer1: S = %d, must be positive", S);
    HN_REQUIRE(n_rays >= 0, "hn_gbuffer1: n_rays = %d", n_rays);
    if (n_rays == 0) return HN_OK;
    HN_REQUIRE(sdf != nullptr && grad != nullptr && rays_d != nullptr && z_vals != nullptr, "hn_gbuffer1: a NULL input");
    if (opacity == nullptr && depth == nullptr && normal == nullptr) return HN_OK;
    GbArgs p = {};
    p.sdf[0] = sdf, p.grad[0] = grad, p.dir[0] = rays_d, p.inv_s[0] = inv_s;
    p.z = z_vals, p.Ro = nullptr, p.n_rays = n_rays, p.rays_per_frame = n_rays, p.S = S, p.sample_dist = sample_dist;
    p.opacity = opacity, p.depth = depth, p.normal = normal;
    return gbuffer_launch<1>(p, s);
}

int gbuffer2(const float* sdf_hand, const float* grad_hand, const float* rays_d_hand, float inv_s_hand, const float* sdf_obj,
             const float* grad_obj, const float* rays_d_obj, float inv_s_obj, const float* z_vals, int n_frames, int rays_per_frame,
             int S, float sample_dist, const float* Ro, float* opacity, float* depth, float* normal, hipStream_t s) {
    HN_REQUIRE(S >= 1, "hn_gbuffer2: S = %d, must be positive", S);
    HN_REQUIRE(n_frames >= 0 && rays_per_frame >= 0, "hn_gbuffer2: %d frames x %d rays", n_frames, rays_per_frame);
    const long long n = (long long)n_frames * rays_per_frame;
    HN_REQUIRE(n <= 0x7fffffffLL, "hn_gbuffer2: %d frames x %d rays do not fit an int", n_frames, rays_per_frame);
    if (n == 0) return HN_OK;
    HN_REQUIRE(sdf_hand != nullptr && grad_hand != nullptr && rays_d_hand != nullptr && sdf_obj != nullptr && grad_obj != nullptr &&
                   rays_d_obj != nullptr && z_vals != nullptr,
               "hn_gbuffer2: a NULL input");
    if (opacity == nullptr && depth == nullptr && normal == nullptr) return HN_OK;
    GbArgs p = {};
    p.sdf[0] = sdf_hand, p.grad[0] = grad_hand, p.dir[0] = rays_d_hand, p.inv_s[0] = inv_s_hand;
    p.sdf[1] = sdf_obj, p.grad[1] = grad_obj, p.dir[1] = rays_d_obj, p.inv_s[1] = inv_s_obj;
    p.z = z_vals, p.Ro = Ro, p.n_rays = (int)n, p.rays_per_frame = rays_per_frame, p.S = S, p.sample_dist = sample_dist;
    p.opacity = opacity, p.depth = depth, p.normal = normal;
    return gbuffer_launch<2>(p, s);
}

// ---- the adjoint: per-ray g_opacity, g_depth, g_normal -> per-sample g_sdf, g_grad and per-ray g_rays_d ------------------------------
// With q^f_k = g_opacity^f + g_depth^f m_k + g_normal^f . grad^f_k (what multiplies w^f_k in the caller's scalar) and the products
// written as in k_composite2_bwd, so that nothing divides by a factor that may be 1e-7:
//   P_k = sum_{j>k} (prod_{k<i<j} f_i) (a^h_j q^h_j + a^o_j q^o_j) = s_{k+1} + f_{k+1} P_{k+1},  f_k = (1 - a^h_k + 1e-7)(1 - a^o_k + 1e-7)
//   dL/da^h_k = T_k q^h_k - T_k P_k (1 - a^o_k + 1e-7)   (and the same with h and o exchanged; one field: T_k q_k - T_k P_k)
//   one field: dL/dc_0 = P_{-1} (T is linear in its seed), added to sample 0's c as hn_composite1_bwd's g_c column 0 is
// then alpha_sample_bwd (hn_scan.h) and g_grad^f_k += w^f_k g_normal^f.  The suffix recurrence is a scan of the affine maps
// x -> s + f x (k_composite2_bwd_wave).  The depths carry no gradient.  Alpha, the weights and the transmittance stay in
// registers: a two-field launch reads the forward's 36 B per ray-sample and writes 32 B.
struct GbBwdArgs {
    const float* sdf[2];
    const float* grad[2];
    const float* dir[2];
    float inv_s[2];
    const float* z;
    int n_rays, S;
    float sample_dist;
    const float *g_opacity, *g_depth, *g_normal;      // [N, NF], [N, NF], [N, NF, 3]; NULL = zero
    float* g_sdf[2];
    float* g_grad[2];
    float* g_dir[2];                                  // [N, 3] or NULL
};

template <int NF>
__device__ __forceinline__ void gb_upstream(const GbBwdArgs& p, int ray, float (&go)[NF], float (&gd)[NF], float (&gn)[NF][3]) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        go[f] = p.g_opacity != nullptr ? p.g_opacity[(size_t)ray * NF + f] : 0.f;
        gd[f] = p.g_depth != nullptr ? p.g_depth[(size_t)ray * NF + f] : 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) gn[f][k] = p.g_normal != nullptr ? p.g_normal[((size_t)ray * NF + f) * 3 + k] : 0.f;
    }
}

// S = 16 CPS, 16 lanes per ray (k_gbuffer_rows' layout and loads; no group of rays ahead: the registers hold c, nx and T per sample).
// Forward: sequential product inside the lane, exclusive product scan over the 16 lanes.  Backward: the lane's samples composed
// last to first into one affine map, a suffix scan of the maps over the 16 lanes (DPP row_shl, the identity shifted in), then the
// recurrence again inside the lane.  The gradients replace the sdf / gradient registers and leave with 16-byte stores.
template <int CPS, int NF>
__global__ __launch_bounds__(256) void k_gbuffer_bwd_rows(const GbBwdArgs p) {
    constexpr int S = 16 * CPS;
    const int lane = threadIdx.x & 63, l = lane & 15, row = lane >> 4;
    for (int g = blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < p.n_rays; g += gridDim.x * 4) {
        const int ray = g * 4 + row;
        const bool ok = ray < p.n_rays;
        const int r = ok ? ray : p.n_rays - 1;
        const size_t base = (size_t)r * S + l * CPS;
        float z[CPS], s[NF][CPS], gr[NF][3 * CPS], d[NF][3], go[NF], gd[NF], gn[NF][3];
        load_run<CPS>(p.z + base, z);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            load_run<CPS>(p.sdf[f] + base, s[f]);
            load_run<3 * CPS>(p.grad[f] + 3 * base, gr[f]);
#pragma unroll
            for (int k = 0; k < 3; ++k) d[f][k] = p.dir[f][3 * (size_t)r + k];
        }
        gb_upstream<NF>(p, r, go, gd, gn);
        const float z_next = dpp<0x101>(0.f, z[0]);       // row_shl:1: the first depth of lane l + 1
        float dist[CPS];
#pragma unroll
        for (int i = 0; i + 1 < CPS; ++i) dist[i] = z[i + 1] - z[i];
        dist[CPS - 1] = l == 15 ? p.sample_dist : z_next - z[CPS - 1];
        float cf[NF][CPS], nx[NF][CPS], tc[NF][CPS], Tk[CPS];
        float Pl = 1.f;
#pragma unroll
        for (int i = 0; i < CPS; ++i) {
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                s[f][i] = alpha_sample(d[f][0], d[f][1], d[f][2], gr[f][3 * i], gr[f][3 * i + 1], gr[f][3 * i + 2], s[f][i], dist[i],
                                       p.inv_s[f], cf[f][i], nx[f][i], tc[f][i]);      // the sdf's register holds alpha from here on
                Pl *= 1.f - s[f][i] + 1e-7f;
            }
        }
        float T = group_excl_prod<16>(Pl, l);
        if (NF == 1) T *= __shfl(cf[0][0], lane & 48, 64);     // SURVEY B-3: the seed is c_0, lane 0 of the group has it
        float M = 1.f, C = 0.f;      // this lane's samples as one map x -> C + M x, applied last to first
#pragma unroll
        for (int i = 0; i < CPS; ++i) {
            Tk[i] = T;
#pragma unroll
            for (int f = 0; f < NF; ++f) T *= 1.f - s[f][i] + 1e-7f;
        }
#pragma unroll
        for (int i = CPS - 1; i >= 0; --i) {
            const float m = z[i] + dist[i] * 0.5f;
            float fac = 1.f, sk = 0.f;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float q = go[f] + gd[f] * m + (gn[f][0] * gr[f][3 * i] + gn[f][1] * gr[f][3 * i + 1] + gn[f][2] * gr[f][3 * i + 2]);
                fac *= 1.f - s[f][i] + 1e-7f;
                sk += s[f][i] * q;
            }
            C = sk + fac * C;
            M = fac * M;
        }
        // inclusive suffix scan over the group's lanes l .. 15: (sm, sc) o (om, oc) = (sm om, sc + sm oc)
        float sm = M, sc = C, om, oc;
        om = dpp<0x101>(1.f, sm), oc = dpp<0x101>(0.f, sc), sc = sc + sm * oc, sm = sm * om;
        om = dpp<0x102>(1.f, sm), oc = dpp<0x102>(0.f, sc), sc = sc + sm * oc, sm = sm * om;
        om = dpp<0x104>(1.f, sm), oc = dpp<0x104>(0.f, sc), sc = sc + sm * oc, sm = sm * om;
        om = dpp<0x108>(1.f, sm), oc = dpp<0x108>(0.f, sc), sc = sc + sm * oc;
        float P = dpp<0x101>(0.f, sc);      // the recurrence's value behind this lane's last sample (0 in lane 15)
        float rd[NF][3];
#pragma unroll
        for (int f = 0; f < NF; ++f) rd[f][0] = rd[f][1] = rd[f][2] = 0.f;
#pragma unroll
        for (int i = CPS - 1; i >= 0; --i) {
            const float m = z[i] + dist[i] * 0.5f;
            float fc[NF], q[NF], sk = 0.f, fac = 1.f;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                q[f] = go[f] + gd[f] * m + (gn[f][0] * gr[f][3 * i] + gn[f][1] * gr[f][3 * i + 1] + gn[f][2] * gr[f][3 * i + 2]);
                fc[f] = 1.f - s[f][i] + 1e-7f;
                fac *= fc[f];
                sk += s[f][i] * q[f];
            }
            const float P_in = sk + fac * P;         // in front of this sample: P_{-1} at sample 0
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float a = s[f][i];
                const float other = NF == 2 ? fc[1 - f] : 1.f;
                const float ga = (a > 0.f && a < 1.f) ? Tk[i] * q[f] - Tk[i] * P * other : 0.f;      // clip(0, 1)
                float g_s, gtc;
                alpha_sample_bwd<NF == 1, true>(cf[f][i], nx[f][i], tc[f][i], dist[i], p.inv_s[f], ga, (i == 0 && l == 0) ? P_in : 0.f, g_s, gtc);
                const float w = a * Tk[i];
                s[f][i] = g_s;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    rd[f][k] += gtc * gr[f][3 * i + k];
                    gr[f][3 * i + k] = gtc * d[f][k] + w * gn[f][k];
                }
            }
            P = P_in;
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (ok) {
                store_run<CPS>(p.g_sdf[f] + base, s[f]);
                store_run<3 * CPS>(p.g_grad[f] + 3 * base, gr[f]);
            }
            if (p.g_dir[f] != nullptr) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float t = group_sum<16>(rd[f][k]);
                    if (ok && l == 0) p.g_dir[f][3 * (size_t)ray + k] = t;
                }
            }
        }
    }
}

// what one lane holds of one sample in the wave-per-ray form; a lane behind the last sample has alpha 0 and factor 1
template <int NF>
struct GbSample {
    bool ok;
    size_t i;
    float dist, m, fac, a[NF], c[NF], nx[NF], tc[NF], g[NF][3];
};
template <int NF>
__device__ __forceinline__ void gb_sample(const GbBwdArgs& p, size_t base, int e, const float (&d)[NF][3], GbSample<NF>& o) {
    o.ok = e < p.S;
    o.i = base + (o.ok ? e : p.S - 1);
    const float z = p.z[o.i];
    o.dist = (o.ok && e + 1 < p.S) ? p.z[o.i + 1] - z : p.sample_dist;
    o.m = z + o.dist * 0.5f;
    o.fac = 1.f;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o.g[f][k] = p.grad[f][3 * o.i + k];
        o.a[f] = alpha_sample(d[f][0], d[f][1], d[f][2], o.g[f][0], o.g[f][1], o.g[f][2], p.sdf[f][o.i], o.dist, p.inv_s[f], o.c[f], o.nx[f],
                              o.tc[f]);
        if (!o.ok) o.a[f] = 0.f;
        o.fac *= o.ok ? (1.f - o.a[f] + 1e-7f) : 1.f;
    }
}

// Every other S: one wave per ray, sample e = lane + 64 m (k_gbuffer's layout).  The transmittance is carried forward over the
// 64-sample segments and the suffix recurrence backward from the LAST one, so a first sweep leaves the transmittance in front of
// segment m in lane m (registers, not memory) and a second sweep walks the segments last to first, evaluating alpha again.  Rays of
// more than 64 segments take these two sweeps once per 64 segments, from the back.
template <int NF>
__global__ __launch_bounds__(256) void k_gbuffer_bwd(const GbBwdArgs p) {
    const int lane = threadIdx.x & 63, S = p.S, nseg = (S + 63) >> 6;
    for (int ray = blockIdx.x * 4 + (threadIdx.x >> 6); ray < p.n_rays; ray += gridDim.x * 4) {
        const size_t base = (size_t)ray * S;
        float d[NF][3], go[NF], gd[NF], gn[NF][3], rd[NF][3];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d[f][k] = p.dir[f][3 * (size_t)ray + k], rd[f][k] = 0.f;
        }
        gb_upstream<NF>(p, ray, go, gd, gn);
        GbSample<NF> x;
        float seed = 1.f;
        if (NF == 1) {      // SURVEY B-3: the first factor is c_0
            gb_sample<NF>(p, base, 0, d, x);
            seed = x.c[0];
        }
        float Pc = 0.f;     // the recurrence's value behind the segments already walked
        for (int hi = nseg; hi > 0; hi -= 64) {
            const int lo = hi > 64 ? hi - 64 : 0;
            float carry = seed, T_in = seed;       // T_in: in front of segment lo + lane
            for (int m = 0; m + 1 < hi; ++m) {
                gb_sample<NF>(p, base, m * 64 + lane, d, x);
                carry *= __shfl(wave_incl_prod(x.fac, lane), 63, 64);
                if (m + 1 - lo == lane) T_in = carry;
            }
            for (int m = hi - 1; m >= lo; --m) {
                gb_sample<NF>(p, base, m * 64 + lane, d, x);
                const float incl = wave_incl_prod(x.fac, lane);
                float excl = __shfl_up(incl, 1, 64);
                if (lane == 0) excl = 1.f;
                const float T = __shfl(T_in, m - lo, 64) * excl;
                float q[NF], sk = 0.f;
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    q[f] = go[f] + gd[f] * x.m + (gn[f][0] * x.g[f][0] + gn[f][1] * x.g[f][1] + gn[f][2] * x.g[f][2]);
                    sk += x.a[f] * q[f];
                }
                float sm = x.fac, sc = sk;      // inclusive suffix scan of the maps over lanes l .. 63
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float om = __shfl_down(sm, off, 64), oc = __shfl_down(sc, off, 64);
                    if (lane + off < 64) {
                        sc = sc + sm * oc;
                        sm = sm * om;
                    }
                }
                const float nm = __shfl_down(sm, 1, 64), nc = __shfl_down(sc, 1, 64);
                const float P = lane == 63 ? Pc : nc + nm * Pc;       // behind this lane's sample
                const float P_in = sk + x.fac * P;                    // in front of it
                Pc = __shfl(P_in, 0, 64);
                if (x.ok) {
#pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        const float a = x.a[f];
                        const float other = NF == 2 ? 1.f - x.a[1 - f] + 1e-7f : 1.f;
                        const float ga = (a > 0.f && a < 1.f) ? T * q[f] - T * P * other : 0.f;      // clip(0, 1)
                        float g_s, gtc;
                        alpha_sample_bwd<NF == 1, true>(x.c[f], x.nx[f], x.tc[f], x.dist, p.inv_s[f], ga, (m == 0 && lane == 0) ? P_in : 0.f, g_s, gtc);
                        const float w = a * T;
                        p.g_sdf[f][x.i] = g_s;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            p.g_grad[f][3 * x.i + k] = gtc * d[f][k] + w * gn[f][k];
                            rd[f][k] += gtc * x.g[f][k];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (p.g_dir[f] != nullptr) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float t = wave_sum(rd[f][k]);
                    if (lane == 0) p.g_dir[f][3 * (size_t)ray + k] = t;
                }
            }
        }
    }
}

template <int NF>
static int gbuffer_bwd_launch(const GbBwdArgs& p, hipStream_t s) {
    bool rows = p.S % 64 == 0 && aligned16(p.z);
    for (int f = 0; f < NF; ++f) rows = rows && aligned16(p.sdf[f]) && aligned16(p.grad[f]) && aligned16(p.g_sdf[f]) && aligned16(p.g_grad[f]);
    const int groups = (p.n_rays + 3) / 4;      // 4 rays per wave, 4 waves per block
    const dim3 rgrid((groups + 3) / 4 < 2048 ? (groups + 3) / 4 : 2048);
    if (rows && p.S == 64)
        hipLaunchKernelGGL((k_gbuffer_bwd_rows<4, NF>), rgrid, dim3(256), 0, s, p);
    else if (rows && p.S == 128)
        hipLaunchKernelGGL((k_gbuffer_bwd_rows<8, NF>), rgrid, dim3(256), 0, s, p);
    else if (rows && p.S == 192)
        hipLaunchKernelGGL((k_gbuffer_bwd_rows<12, NF>), rgrid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((k_gbuffer_bwd<NF>), dim3(composite_grid(p.n_rays)), dim3(256), 0, s, p);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int gbuffer1_bwd(const float* sdf, const float* grad, const float* rays_d, const float* z_vals, int n_rays, int S, float sample_dist,
                 float inv_s, const float* g_opacity, const float* g_depth, const float* g_normal, float* g_sdf, float* g_grad,
                 float* g_rays_d, hipStream_t s) {
    HN_REQUIRE(S >= 1, "hn_gbuffer1_bwd: S = %d, must be positive", S);
    HN_REQUIRE(n_rays >= 0, "hn_gbuffer1_bwd: n_rays = %d", n_rays);
    if (n_rays == 0) return HN_OK;
    HN_REQUIRE(sdf != nullptr && grad != nullptr && rays_d != nullptr && z_vals != nullptr, "hn_gbuffer1_bwd: a NULL input");
    HN_REQUIRE(g_sdf != nullptr && g_grad != nullptr, "hn_gbuffer1_bwd: g_sdf and g_grad are required");
    HN_REQUIRE(g_opacity != nullptr || g_depth != nullptr || g_normal != nullptr, "hn_gbuffer1_bwd: no upstream gradient (all three NULL)");
    GbBwdArgs p = {};
    p.sdf[0] = sdf, p.grad[0] = grad, p.dir[0] = rays_d, p.inv_s[0] = inv_s;
    p.z = z_vals, p.n_rays = n_rays, p.S = S, p.sample_dist = sample_dist;
    p.g_opacity = g_opacity, p.g_depth = g_depth, p.g_normal = g_normal;
    p.g_sdf[0] = g_sdf, p.g_grad[0] = g_grad, p.g_dir[0] = g_rays_d;
    return gbuffer_bwd_launch<1>(p, s);
}

int gbuffer2_bwd(const float* sdf_hand, const float* grad_hand, const float* rays_d_hand, float inv_s_hand, const float* sdf_obj,
                 const float* grad_obj, const float* rays_d_obj, float inv_s_obj, const float* z_vals, int n_frames, int rays_per_frame,
                 int S, float sample_dist, const float* g_opacity, const float* g_depth, const float* g_normal, float* g_sdf_hand,
                 float* g_grad_hand, float* g_sdf_obj, float* g_grad_obj, float* g_rays_d_hand, float* g_rays_d_obj, hipStream_t s) {
    HN_REQUIRE(S >= 1, "hn_gbuffer2_bwd: S = %d, must be positive", S);
    HN_REQUIRE(n_frames >= 0 && rays_per_frame >= 0, "hn_gbuffer2_bwd: %d frames x %d rays", n_frames, rays_per_frame);
    const long long n = (long long)n_frames * rays_per_frame;
    HN_REQUIRE(n <= 0x7fffffffLL, "hn_gbuffer2_bwd: %d frames x %d rays do not fit an int", n_frames, rays_per_frame);
    if (n == 0) return HN_OK;
    HN_REQUIRE(sdf_hand != nullptr && grad_hand != nullptr && rays_d_hand != nullptr && sdf_obj != nullptr && grad_obj != nullptr &&
                   rays_d_obj != nullptr && z_vals != nullptr,
               "hn_gbuffer2_bwd: a NULL input");
    HN_REQUIRE(g_sdf_hand != nullptr && g_grad_hand != nullptr && g_sdf_obj != nullptr && g_grad_obj != nullptr,
               "hn_gbuffer2_bwd: g_sdf and g_grad of both fields are required");
    HN_REQUIRE(g_opacity != nullptr || g_depth != nullptr || g_normal != nullptr, "hn_gbuffer2_bwd: no upstream gradient (all three NULL)");
    GbBwdArgs p = {};
    p.sdf[0] = sdf_hand, p.grad[0] = grad_hand, p.dir[0] = rays_d_hand, p.inv_s[0] = inv_s_hand;
    p.sdf[1] = sdf_obj, p.grad[1] = grad_obj, p.dir[1] = rays_d_obj, p.inv_s[1] = inv_s_obj;
    p.z = z_vals, p.n_rays = (int)n, p.S = S, p.sample_dist = sample_dist;
    p.g_opacity = g_opacity, p.g_depth = g_depth, p.g_normal = g_normal;
    p.g_sdf[0] = g_sdf_hand, p.g_grad[0] = g_grad_hand, p.g_dir[0] = g_rays_d_hand;
    p.g_sdf[1] = g_sdf_obj, p.g_grad[1] = g_grad_obj, p.g_dir[1] = g_rays_d_obj;
    return gbuffer_bwd_launch<2>(p, s);
}

}  // namespace hn

extern "C" {
int hn_gbuffer1(const float* sdf, const float* grad, const float* rays_d, const float* z_vals, int n_rays, int S, float sample_dist,
                float inv_s, float* opacity, float* depth, float* normal, hn_stream_t stream) {
    return hn::gbuffer1(sdf, grad, rays_d, z_vals, n_rays, S, sample_dist, inv_s, opacity, depth, normal, (hipStream_t)stream);
}
int hn_gbuffer2(const float* sdf_hand, const float* grad_hand, const float* rays_d_hand, float inv_s_hand, const float* sdf_obj,
                const float* grad_obj, const float* rays_d_obj, float inv_s_obj, const float* z_vals, int n_frames, int rays_per_frame,
                int S, float sample_dist, const float* Ro, float* opacity, float* depth, float* normal, hn_stream_t stream) {
    return hn::gbuffer2(sdf_hand, grad_hand, rays_d_hand, inv_s_hand, sdf_obj, grad_obj, rays_d_obj, inv_s_obj, z_vals, n_frames,
                        rays_per_frame, S, sample_dist, Ro, opacity, depth, normal, (hipStream_t)stream);
}
int hn_gbuffer1_bwd(const float* sdf, const float* grad, const float* rays_d, const float* z_vals, int n_rays, int S, float sample_dist,
                    float inv_s, const float* g_opacity, const float* g_depth, const float* g_normal, float* g_sdf, float* g_grad,
                    float* g_rays_d, hn_stream_t stream) {
    return hn::gbuffer1_bwd(sdf, grad, rays_d, z_vals, n_rays, S, sample_dist, inv_s, g_opacity, g_depth, g_normal, g_sdf, g_grad, g_rays_d,
                            (hipStream_t)stream);
}
int hn_gbuffer2_bwd(const float* sdf_hand, const float* grad_hand, const float* rays_d_hand, float inv_s_hand, const float* sdf_obj,
                    const float* grad_obj, const float* rays_d_obj, float inv_s_obj, const float* z_vals, int n_frames, int rays_per_frame,
                    int S, float sample_dist, const float* g_opacity, const float* g_depth, const float* g_normal, float* g_sdf_hand,
                    float* g_grad_hand, float* g_sdf_obj, float* g_grad_obj, float* g_rays_d_hand, float* g_rays_d_obj, hn_stream_t stream) {
    return hn::gbuffer2_bwd(sdf_hand, grad_hand, rays_d_hand, inv_s_hand, sdf_obj, grad_obj, rays_d_obj, inv_s_obj, z_vals, n_frames,
                            rays_per_frame, S, sample_dist, g_opacity, g_depth, g_normal, g_sdf_hand, g_grad_hand, g_sdf_obj, g_grad_obj,
                            g_rays_d_hand, g_rays_d_obj, (hipStream_t)stream);
}
}
