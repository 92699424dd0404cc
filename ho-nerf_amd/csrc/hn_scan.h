// What the alpha / compositing kernels (hn_composite.hip) and the geometry-buffer kernels (hn_gbuffer.hip) share: the per-sample
// SDF -> alpha arithmetic and its adjoint (one statement of each, so that the kernels cannot drift), the wavefront and DPP scans, the
// 16-byte run loads and stores and the grid cap.
#pragma once
#include "hn_common.h"

namespace hn {

__device__ __forceinline__ float sigmoid_e(float x) { return 1.f / (1.f + expf(-x)); }

// utils/renderer.py:147-161 (401-415 for the two-field renderer) with cos_anneal_ratio = 1, for one sample: ray direction d, field
// gradient g, sdf s, section length dist -> alpha clipped to [0, 1]; c = sigmoid((s - half) inv_s), the cdf in front of the section.
// This form also hands back what the adjoint needs: nx = sigmoid((s + half) inv_s), the cdf behind the section, and true_cos.
__device__ __forceinline__ float alpha_sample(float dx, float dy, float dz, float gx, float gy, float gz, float s, float dist,
                                              float inv_s, float& c, float& nx, float& true_cos) {
    true_cos = dx * gx + dy * gy + dz * gz;
    const float iter_cos = -fmaxf(-true_cos, 0.f);     // cos_anneal_ratio = 1
    const float half = iter_cos * dist * 0.5f;
    c = sigmoid_e((s - half) * inv_s);
    nx = sigmoid_e((s + half) * inv_s);
    const float a = ((c - nx) + 1e-5f) / (c + 1e-5f);
    return fminf(fmaxf(a, 0.f), 1.f);
}
__device__ __forceinline__ float alpha_sample(float dx, float dy, float dz, float gx, float gy, float gz, float s, float dist,
                                              float inv_s, float& c) {
    float nx, true_cos;
    return alpha_sample(dx, dy, dz, gx, gy, gz, s, dist, inv_s, c, nx, true_cos);
}

// Adjoint of alpha_sample for one sample, from the cdf values c and nx and true_cos the forward statement computed: ga is the
// gradient on alpha with the clip applied (0 where the unclipped quotient is outside (0, 1)), gc_in a direct gradient on c
// (HAS_GC; the one-field seed) -> g_s on the sdf and gtc on true_cos (g_grad = gtc d, g_rays_d = sum gtc grad).  The section
// length carries no gradient.  k_alpha_bwd, k_alpha_bwd_up (hn_composite.hip) and the geometry buffers' adjoint (hn_gbuffer.hip)
// all go through this one statement.
// g_s = gx1 + gx2 is a difference of two terms that agree to 4 - 5 digits wherever c and nx are close (a back-facing sample has
// c == nx): ga (B - A) / B^2 c (1 - c) - ga / B nx (1 - nx).  With B - A = nx the sum is
//   g_s = -ga inv_s nx / B^2 (c (c - nx) + 1e-5 (1 - nx))      (+ gc_in inv_s c (1 - c)),
// two terms of one sign.  COMBINED_SDF takes that form (the geometry buffers' adjoint: against float64 it is 1e-6 where the sum is
// 1e-3); the alpha kernels keep the sum, and with it the bits they have always given.
template <bool HAS_GC, bool COMBINED_SDF = false>
__device__ __forceinline__ void alpha_sample_bwd(float c, float nx, float tc, float dist, float inv_s, float ga, float gc_in,
                                                 float& g_s, float& gtc) {
    const float A = (c - nx) + 1e-5f, B = c + 1e-5f;
    // a = A / B: da/dc = (B - A) / B^2, da/dnx = -1 / B
    float gc = ga * (B - A) / (B * B);
    if (HAS_GC) gc += gc_in;
    const float gnx = -ga / B;
    const float gx1 = gc * inv_s * c * (1.f - c);      // x1 = s - half
    const float gx2 = gnx * inv_s * nx * (1.f - nx);   // x2 = s + half
    if (COMBINED_SDF) {
        g_s = -(ga * inv_s) * nx / (B * B) * (c * (c - nx) + 1e-5f * (1.f - nx));
        if (HAS_GC) g_s += gc_in * inv_s * c * (1.f - c);
    } else {
        g_s = gx1 + gx2;
    }
    const float ghalf = gx2 - gx1;
    gtc = (tc < 0.f) ? ghalf * dist * 0.5f : 0.f;      // iter_cos = min(true_cos, 0)
}

__device__ __forceinline__ float wave_incl_prod(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off, 64);
        if (lane >= off) v *= o;
    }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int CTRL>
__device__ __forceinline__ float dpp(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL,
                                                                  0xf, 0xf, false));
}
// loads CPS consecutive floats / CPS consecutive float3 of this lane (16-byte accesses)
template <int CPS>
__device__ __forceinline__ void load_run(const float* __restrict__ p, float (&v)[CPS]) {
#pragma unroll
    for (int q = 0; q < CPS / 4; ++q) {
        const float4 t = reinterpret_cast<const float4*>(p)[q];
        v[4 * q] = t.x;
        v[4 * q + 1] = t.y;
        v[4 * q + 2] = t.z;
        v[4 * q + 3] = t.w;
    }
}
// the store of such a run
template <int CPS>
__device__ __forceinline__ void store_run(float* __restrict__ p, const float (&v)[CPS]) {
#pragma unroll
    for (int q = 0; q < CPS / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
// sum over a group of LPR (8 or 16) consecutive lanes, result in every lane of the group: xor butterflies as DPP
// (quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140): VALU only
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
    v += dpp<0xB1>(0.f, v);
    v += dpp<0x4E>(0.f, v);
    v += dpp<0x141>(0.f, v);
    if (LPR == 16) v += dpp<0x140>(0.f, v);
    return v;
}
// exclusive product scan over the group (lane l of the group gets the product of lanes 0 .. l-1; lane 0 gets 1)
template <int LPR>
__device__ __forceinline__ float group_excl_prod(float v, int l) {
    float t;
    t = dpp<0x111>(1.f, v);
    v *= (LPR == 16 || l >= 1) ? t : 1.f;
    t = dpp<0x112>(1.f, v);
    v *= (LPR == 16 || l >= 2) ? t : 1.f;
    t = dpp<0x114>(1.f, v);
    v *= (LPR == 16 || l >= 4) ? t : 1.f;
    if (LPR == 16) v *= dpp<0x118>(1.f, v);
    t = dpp<0x111>(1.f, v);          // shift the inclusive scan by one lane
    return l >= 1 ? t : 1.f;
}

// 4 rays per block; at most 8 blocks per CU, grid-stride beyond that
static inline int composite_grid(int n_rays) {
    const int blocks = (n_rays + 3) / 4;
    return blocks < 2048 ? blocks : 2048;
}

}  // namespace hn
