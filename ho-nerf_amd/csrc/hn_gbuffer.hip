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
}
