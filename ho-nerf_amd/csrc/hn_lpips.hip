// LPIPS (VGG16, version 0.1, linear layers on, spatial off, eval mode) on the device: the third column of
// analys_results/analys_psnr_ssim_lpips.py:28-33,44 (lpips.LPIPS(net='vgg') on x = u8 / 128 - 1) for F pairs of 8-bit interleaved RGB
// images [F, H, W, 3] of one size.  tests/test_lpips_cpu.py restates it in float64 torch; DESIGN.md 3.18 is the contract.
//
// The model (hn_lpips_create) holds the 13 convolutions' weights packed once into MFMA fragment order, their biases and the five
// 1x1 linear weight vectors.  A call runs the 2 F images (a's, then b's) through the whole stack as ONE batch: activations are
// channel-last fp32 [N, h, w, C] in the caller's workspace.  No allocation, no synchronisation, no floating-point atomics: every
// output element is one fmaf chain in a fixed order that does not depend on where its tile lies, every reduction combines its
// partials in a fixed order per image, so a repeated call, another batch size or another position in the batch give the same bits.
//
// The convolution stack (packing, patch gather, exact-fp32 implicit GEMM, pool: k_cv_pack, k_cv_im2col, k_cv_conv, k_cv_pool) is
// hn_conv3x3.h, shared with hn_vggloss.hip.  LPIPS runs it with all nine taps live and one K split for every layer and size.
//
// Its own kernels:
//   LpLoad           the scaling layer, as the patch gather's loader: u8 -> ((u8 / 128 - 1) - shift) / scale (the gather's zeros outside
//                    the image are the zero padding of the SCALED input)
//   k_lp_head        per pixel of a tap (one wave per pixel, lanes over channels): n(f) = f / (sqrt(sum_c f^2) + 1e-10) for both
//                    images, sum_c w[c] (n(fa) - n(fb))^2 in fp32, summed over the wave's 16 pixels and the workgroup's 4 waves in fp64
//                    -> one partial per 64 pixels
//   k_lp_head_final  one wave per pair: strided sum of the partials, butterfly, the mean -> per_tap [F, 5]
//   k_lp_nchw        a tap [N, h, w, C] -> torch's [N, C, h, w] (hn_lpips_features)
#include "hn_conv3x3.h"

struct hn_lpips_model {
    void* blob = nullptr;                // one device allocation: packed weights, biases, linear weights
    const float4* wpk[13] = {};
    const float* bias[13] = {};
    const float* lin[5] = {};
};

namespace hn {
namespace {

constexpr int LP_CONVS = 13, LP_TAPS = 5;
constexpr int LP_CIN[LP_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_TAP_C[LP_TAPS] = {64, 128, 256, 512, 512};
constexpr int LP_MIN_SIDE = 16;                                   // the fifth tap is floor(H / 16) x floor(W / 16)
constexpr long long LP_MAX = 1LL << 31;                           // N H W 64, the largest activation, stays below this

constexpr int HEAD_THREADS = 256, HEAD_PX_WAVE = 16, HEAD_PX = (HEAD_THREADS / 64) * HEAD_PX_WAVE;

// ---- the scaling layer, inside the first layer's patch gather -------------------------------------------------------------------------
struct LpLoad {
    const unsigned char *a, *b;          // [., h, w, 3]: image f of a at f < n_a, of b at f - n_a
    int n_a, h, w;
    __device__ float operator()(int f, int yy, int xx, int c) const {
        const unsigned char* img = f < n_a ? a + (long long)f * h * w * 3 : b + (long long)(f - n_a) * h * w * 3;
        const float shift = c == 0 ? -0.030f : c == 1 ? -0.088f : -0.188f;
        const float scale = c == 0 ? 0.458f : c == 1 ? 0.448f : 0.450f;
        const float u = (float)img[((long long)yy * w + xx) * 3 + c] / 128.f - 1.f;          // exact
        return (u - shift) / scale;
    }
};

// ---- the head ----------------------------------------------------------------------------------------------------------------------
// feat [2 F, hw, C]: image f of a at f, of b at F + f.  grid (blocks per image, F) -> partial [F, blocks]
__global__ void __launch_bounds__(HEAD_THREADS) k_lp_head(const float* __restrict__ feat, const float* __restrict__ lin, int n_pairs, int hw, int c,
                                                          double* __restrict__ partial) {
    __shared__ double red[HEAD_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.y, nj = c / 64;
    const float* fa = feat + (long long)f * hw * c;
    const float* fb = feat + (long long)(n_pairs + f) * hw * c;
    float wl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wl[j] = j < nj ? lin[lane + 64 * j] : 0.f;
    double sum = 0.0;
    const int p0 = blockIdx.x * HEAD_PX + wave * HEAD_PX_WAVE;
    for (int p = p0; p < p0 + HEAD_PX_WAVE && p < hw; ++p) {                    // uniform over the wave
        float va[8], vb[8], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            va[j] = j < nj ? fa[(long long)p * c + lane + 64 * j] : 0.f;
            vb[j] = j < nj ? fb[(long long)p * c + lane + 64 * j] : 0.f;
            sa += va[j] * va[j];
            sb += vb[j] * vb[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sa += __shfl_xor(sa, o, 64);
            sb += __shfl_xor(sb, o, 64);
        }
        const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = va[j] / na - vb[j] / nb;                            // a and b enter alike: swapping them gives the same bits
            d += wl[j] * (e * e);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        sum += (double)d;
    }
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < HEAD_THREADS / 64; ++k) s += red[k];
        partial[(long long)f * gridDim.x + blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(64) k_lp_head_final(const double* __restrict__ partial, int blocks, double count, int tap, double* __restrict__ per_tap) {
    const double* p = partial + (long long)blockIdx.x * blocks;
    double v = 0.0;
    for (int k = threadIdx.x; k < blocks; k += 64) v += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x == 0) per_tap[(long long)blockIdx.x * LP_TAPS + tap] = v / count;
}

__global__ void __launch_bounds__(256) k_lp_nchw(const float* __restrict__ in, int n_img, int hw, int c, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)n_img * hw * c;
    if (i >= total) return;
    const int p = (int)(i % hw), ch = (int)((i / hw) % c);
    const long long f = i / ((long long)hw * c);
    out[i] = in[(f * hw + p) * c + ch];
}

// ---- shapes and the workspace ------------------------------------------------------------------------------------------------------
struct LpShape {
    int h[LP_TAPS], w[LP_TAPS];
    size_t s0, s1, tap[LP_TAPS], partial;       // byte offsets into the workspace
    int head_blocks[LP_TAPS];
};

// n_img images through the stack, n_pairs > 0: with the head's partials
int lp_shape(const char* who, long long n_img, long long n_pairs, long long height, long long width, LpShape& s, size_t& bytes) {
    HN_REQUIRE(n_img >= 1 && height >= LP_MIN_SIDE && width >= LP_MIN_SIDE,
               "%s: n_images = %lld, height = %lld, width = %lld: at least one image of %d x %d (the fifth tap is floor(H / 16) x floor(W / 16))", who,
               n_pairs > 0 ? n_pairs : n_img, height, width, LP_MIN_SIDE, LP_MIN_SIDE);
    HN_REQUIRE(height < LP_MAX && width < LP_MAX && n_img < LP_MAX && height * width < LP_MAX && n_img * height * width < LP_MAX / 64,
               "%s: n_images = %lld, height = %lld, width = %lld: the largest activation, images x height x width x 64, must stay below 2^31", who,
               n_pairs > 0 ? n_pairs : n_img, height, width);
    const size_t px = (size_t)(n_img * height * width);
    size_t off = 0;
    s.s0 = off;
    off += up256(px * 64 * sizeof(float));
    s.s1 = off;
    off += up256(px * 32 * sizeof(float));
    for (int k = 0; k < LP_TAPS; ++k) {
        s.h[k] = (int)(height >> k);
        s.w[k] = (int)(width >> k);
        s.tap[k] = off;
        off += up256((size_t)n_img * s.h[k] * s.w[k] * LP_TAP_C[k] * sizeof(float));
        s.head_blocks[k] = (s.h[k] * s.w[k] + HEAD_PX - 1) / HEAD_PX;
    }
    s.partial = off;
    if (n_pairs > 0) off += up256((size_t)n_pairs * s.head_blocks[0] * sizeof(double));
    bytes = off;
    return HN_OK;
}

// every layer with all nine taps (the first: its one gathered tap) and one split, whatever the size
int lp_conv(const hn_lpips_model* m, int layer, const float* in, float* out, long long n_img, int h, int w, hipStream_t s) {
    const bool first = layer == 0;
    const int cin = first ? CV_KC : LP_CIN[layer], cout = LP_COUT[layer];
    return cv_conv<false, false>(in, m->wpk[layer], n_img * h * w, h, w, cin, cout, first, CV_ALL_TAPS, (first ? 1 : 9) * (cin / CV_KC), 1, nullptr,
                   CvFwd{m->bias[layer], out, cout}, s);
}

// the five taps of n_a images of `a` followed by n_b of `b`, channel-last, at sh.tap[] of the workspace
int lp_stack(const hn_lpips_model* m, const unsigned char* a, const unsigned char* b, long long n_a, long long n_b, const LpShape& sh, char* ws, hipStream_t s) {
    const long long n = n_a + n_b;
    float *s0 = (float*)(ws + sh.s0), *s1 = (float*)(ws + sh.s1);
    float* tap[LP_TAPS];
    for (int k = 0; k < LP_TAPS; ++k) tap[k] = (float*)(ws + sh.tap[k]);
    HN_TRY_RC(cv_im2col(LpLoad{a, b, (int)n_a, sh.h[0], sh.w[0]}, n, sh.h[0], sh.w[0], s1, s));
    HN_TRY_RC(lp_conv(m, 0, s1, s0, n, sh.h[0], sh.w[0], s));
    HN_TRY_RC(lp_conv(m, 1, s0, tap[0], n, sh.h[0], sh.w[0], s));
    HN_TRY_RC(cv_pool(tap[0], s1, n, sh.h[0], sh.w[0], 64, s));
    HN_TRY_RC(lp_conv(m, 2, s1, s0, n, sh.h[1], sh.w[1], s));
    HN_TRY_RC(lp_conv(m, 3, s0, tap[1], n, sh.h[1], sh.w[1], s));
    HN_TRY_RC(cv_pool(tap[1], s1, n, sh.h[1], sh.w[1], 128, s));
    HN_TRY_RC(lp_conv(m, 4, s1, s0, n, sh.h[2], sh.w[2], s));
    HN_TRY_RC(lp_conv(m, 5, s0, s1, n, sh.h[2], sh.w[2], s));
    HN_TRY_RC(lp_conv(m, 6, s1, tap[2], n, sh.h[2], sh.w[2], s));
    HN_TRY_RC(cv_pool(tap[2], s0, n, sh.h[2], sh.w[2], 256, s));
    HN_TRY_RC(lp_conv(m, 7, s0, s1, n, sh.h[3], sh.w[3], s));
    HN_TRY_RC(lp_conv(m, 8, s1, s0, n, sh.h[3], sh.w[3], s));
    HN_TRY_RC(lp_conv(m, 9, s0, tap[3], n, sh.h[3], sh.w[3], s));
    HN_TRY_RC(cv_pool(tap[3], s0, n, sh.h[3], sh.w[3], 512, s));
    HN_TRY_RC(lp_conv(m, 10, s0, s1, n, sh.h[4], sh.w[4], s));
    HN_TRY_RC(lp_conv(m, 11, s1, s0, n, sh.h[4], sh.w[4], s));
    HN_TRY_RC(lp_conv(m, 12, s0, tap[4], n, sh.h[4], sh.w[4], s));
    return HN_OK;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

int hn_lpips_create(const float* const* conv_weight, const float* const* conv_bias, const float* const* lin_weight, hn_lpips_model** out, hn_stream_t stream) {
    HN_REQUIRE(conv_weight && conv_bias && lin_weight && out, "hn_lpips_create: NULL conv_weight / conv_bias / lin_weight / out");
    for (int l = 0; l < LP_CONVS; ++l) HN_REQUIRE(conv_weight[l] && conv_bias[l], "hn_lpips_create: NULL weight or bias of convolution %d", l);
    for (int k = 0; k < LP_TAPS; ++k) HN_REQUIRE(lin_weight[k], "hn_lpips_create: NULL linear weight %d", k);
    hipStream_t s = (hipStream_t)stream;
    size_t off_w[LP_CONVS], off_b[LP_CONVS], off_l[LP_TAPS], off = 0;
    for (int l = 0; l < LP_CONVS; ++l) {
        off_w[l] = off;
        off += up256(cv_pack_floats(LP_CIN[l], LP_COUT[l], 0) * sizeof(float));
        off_b[l] = off;
        off += up256((size_t)LP_COUT[l] * sizeof(float));
    }
    for (int k = 0; k < LP_TAPS; ++k) {
        off_l[k] = off;
        off += up256((size_t)LP_TAP_C[k] * sizeof(float));
    }
    void* blob = nullptr;
    HN_CHECK_HIP(hipMalloc(&blob, off));
    hn_lpips_model* m = new hn_lpips_model();
    m->blob = blob;
    int rc = HN_OK;
    auto fail = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == HN_OK) {
            set_error("hn_lpips_create: %s failed: %s", what, hipGetErrorString(e));
            rc = HN_EHIP;
        }
    };
    for (int l = 0; l < LP_CONVS && rc == HN_OK; ++l) {
        float* w = (float*)((char*)blob + off_w[l]);
        fail(cv_pack(conv_weight[l], LP_CIN[l], LP_COUT[l], 0, w, s), "the pack launch");
        fail(hipMemcpyAsync((char*)blob + off_b[l], conv_bias[l], LP_COUT[l] * sizeof(float), hipMemcpyDeviceToDevice, s), "the bias copy");
        m->wpk[l] = (const float4*)w;
        m->bias[l] = (const float*)((char*)blob + off_b[l]);
    }
    for (int k = 0; k < LP_TAPS && rc == HN_OK; ++k) {
        fail(hipMemcpyAsync((char*)blob + off_l[k], lin_weight[k], LP_TAP_C[k] * sizeof(float), hipMemcpyDeviceToDevice, s), "the linear weight copy");
        m->lin[k] = (const float*)((char*)blob + off_l[k]);
    }
    if (rc == HN_OK) fail(hipStreamSynchronize(s), "hipStreamSynchronize");       // the caller's tensors may go once this returns
    if (rc != HN_OK) {
        (void)hipFree(blob);
        delete m;
        return rc;
    }
    *out = m;
    return HN_OK;
}

int hn_lpips_destroy(hn_lpips_model* m) {
    if (m == nullptr) return HN_OK;
    if (m->blob != nullptr) HN_CHECK_HIP(hipFree(m->blob));
    delete m;
    return HN_OK;
}

size_t hn_lpips_workspace_bytes(long long n_pairs, long long height, long long width) {
    LpShape sh;
    size_t bytes = 0;
    if (n_pairs < 1 || n_pairs >= LP_MAX) {
        set_error("hn_lpips_workspace_bytes: n_pairs = %lld", n_pairs);
        return 0;
    }
    return lp_shape("hn_lpips_workspace_bytes", 2 * n_pairs, n_pairs, height, width, sh, bytes) == HN_OK ? bytes : 0;
}

int hn_lpips(const hn_lpips_model* model, const unsigned char* a, const unsigned char* b, long long n_pairs, long long height, long long width, double* per_tap,
             void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    LpShape sh;
    size_t need = 0;
    HN_REQUIRE(n_pairs >= 1 && n_pairs < LP_MAX, "hn_lpips: n_pairs = %lld", n_pairs);
    HN_TRY_RC(lp_shape("hn_lpips", 2 * n_pairs, n_pairs, height, width, sh, need));
    HN_REQUIRE(model && a && b && per_tap && workspace, "hn_lpips: NULL model / a / b / per_tap / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_lpips: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)per_tap & 7) == 0, "hn_lpips: workspace not 16-byte aligned, or per_tap not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    HN_TRY_RC(lp_stack(model, a, b, n_pairs, n_pairs, sh, ws, s));
    double* partial = (double*)(ws + sh.partial);
    for (int k = 0; k < LP_TAPS; ++k) {
        const int hw = sh.h[k] * sh.w[k];
        k_lp_head<<<dim3((unsigned)sh.head_blocks[k], (unsigned)n_pairs), HEAD_THREADS, 0, s>>>((const float*)(ws + sh.tap[k]), model->lin[k], (int)n_pairs, hw,
                                                                                              LP_TAP_C[k], partial);
        HN_LAUNCH_CHECK();
        k_lp_head_final<<<(unsigned)n_pairs, 64, 0, s>>>(partial, sh.head_blocks[k], (double)hw, k, per_tap);
        HN_LAUNCH_CHECK();
    }
    return HN_OK;
}

int hn_lpips_features(const hn_lpips_model* model, const unsigned char* img, long long n_images, long long height, long long width, float* tap0, float* tap1,
                      float* tap2, float* tap3, float* tap4, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    LpShape sh;
    size_t need = 0;
    HN_TRY_RC(lp_shape("hn_lpips_features", n_images, 0, height, width, sh, need));
    HN_REQUIRE(model && img && tap0 && tap1 && tap2 && tap3 && tap4 && workspace, "hn_lpips_features: NULL model / img / tap / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_lpips_features: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_lpips_features: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    HN_TRY_RC(lp_stack(model, img, img, n_images, 0, sh, ws, s));
    float* outs[LP_TAPS] = {tap0, tap1, tap2, tap3, tap4};
    for (int k = 0; k < LP_TAPS; ++k) {
        const long long total = n_images * sh.h[k] * sh.w[k] * LP_TAP_C[k];
        k_lp_nchw<<<(unsigned)((total + 255) / 256), 256, 0, s>>>((const float*)(ws + sh.tap[k]), (int)n_images, sh.h[k] * sh.w[k], LP_TAP_C[k], outs[k]);
        HN_LAUNCH_CHECK();
    }
    return HN_OK;
}

}  // extern "C"
