// The VGG19 perceptual loss of training (utils/fields.py:407-433 VGGLoss, exp_runner.py:228-236) on the device, forward and backward:
// loss = sum_k mean |tap_k(source) - tap_k(target)| over the five taps relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 of VGG19's
// `features` (the ReLU outputs of the convolutions 0, 2, 4, 8, 12 counted from 0; MaxPool2d(2, 2) in floor mode in front of the
// convolutions 2, 4, 8, 12), and d loss / d source.  The input goes in as it is: no normalisation, no scaling layer.  DESIGN.md 3.19
// is the contract, honerf_amd.training.vgg_loss_reference the torch restatement the tests hold it to.
//
// The model (hn_vgg_loss_create) holds every convolution's weights packed twice into MFMA fragment order: for the forward pass
// (K = 9 Cin, tap-major) and for backward-data (K = 9 Cout, taps flipped, Cin and Cout swapped; the 3 input channels of the first
// convolution padded to one N tile).  Activations are channel-last fp32 in the caller's workspace.  hn_vgg_loss_fwd runs source and
// target through the stack as one batch of 2 and leaves every layer's output and the four pooled tensors in the workspace;
// hn_vgg_loss_bwd reads them.  No allocation, no synchronisation, no floating-point atomics: every sum is taken in an order that the
// shape alone decides, so a repeated call gives the same bits.
//
// Precision: exact fp32, v_mfma_f32_32x32x2_f32, for the reason hn_conv3x3.h gives.
//
// The convolution stack (both packings, patch gather, implicit GEMM with its K split and live-tap list, the partials' sum, pool:
// k_cv_pack, k_cv_im2col, k_cv_conv, k_cv_reduce, k_cv_pool) is hn_conv3x3.h, shared with hn_lpips.hip.  What this file decides for
// the small images this loss sees (21 x 21 -> 21, 10, 5, 2, 1 pixels per side): the K chunks of a layer of a few rows are split so
// that it still occupies every CU (vg_splits: as many splits as bring the launch to VG_TARGET_BLOCKS workgroups), and taps that lie
// outside the image for every pixel (a side of 1: only the centre row / column of taps is live) are left out of the mask.
//
// Its own kernels:
//   VgLoad          the patch gather's loader: the two caller buffers through (y, x, channel) strides -> [2, h, w, 32]
//   VgEpi           the backward epilogues.  VG_PLAIN: the value (gradient at a pooled tensor).  VG_GATE: backward-data landing on a
//                   ReLU output y: (+ sign(y_source - y_target) g_loss / numel where y is a tap), times [y > 0].  VG_LAST: the 3
//                   channels of d loss / d source through the caller's strides.  (Forward is the shared CvFwd: + bias, ReLU.)
//   k_vg_seed       the gradient at the last tap: VG_GATE on zeros
//   k_vg_pool_bwd   the gradient to the first maximum of each window in row-major order, times [y > 0]
//   k_vg_l1         sum |s - t| of one tap's 4096-element slice in fp64 -> one partial; k_vg_l1_final: the partials in index order,
//                   the five means, their sum
#include "hn_conv3x3.h"

struct hn_vgg_loss_model {
    void* blob = nullptr;                // one device allocation: both packings, biases
    const float4* wf[13] = {};
    const float4* wb[13] = {};
    const float* bias[13] = {};
};

namespace hn {
namespace {

constexpr int VG_CONVS = 13, VG_TAPS = 5;
constexpr int VG_CIN[VG_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
constexpr int VG_COUT[VG_CONVS] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int VG_LEVEL[VG_CONVS] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4};           // pools in front of the layer
constexpr int VG_TAP_OF[VG_CONVS] = {0, -1, 1, -1, 2, -1, -1, -1, 3, -1, -1, -1, 4};  // the tap a layer's output is, or -1
constexpr int VG_MIN_SIDE = 16;
constexpr long long VG_MAX = 1LL << 31;
constexpr int VG_TARGET_BLOCKS = 256;                             // the CUs of an MI355X: a launch below this is split over K

constexpr int L1_THREADS = 256, L1_PER_BLOCK = L1_THREADS * 16;

// ---- the first layer's patches -------------------------------------------------------------------------------------------------------
struct VgLoad {
    const float *src, *tgt;              // image 0, image 1
    long long sy, sx, sc;
    __device__ float operator()(int f, int yy, int xx, int c) const { return (f == 0 ? src : tgt)[yy * sy + xx * sx + c * sc]; }
};

// ---- the backward epilogues ------------------------------------------------------------------------------------------------------------
enum { VG_PLAIN, VG_GATE, VG_LAST };

struct VgEpi {
    int mode = VG_PLAIN;
    int n_real = 0;                      // channels of `out` (and of ys, yt): its row pitch
    const float* ys = nullptr;           // VG_GATE: the source's ReLU output this gradient lands on, [M, n_real]
    const float* yt = nullptr;           // VG_GATE where that output is a tap: the target's; else NULL
    const float* g_loss = nullptr;       // device scalar
    float inv_numel = 0.f;
    float* out = nullptr;
    int w = 1;                           // VG_LAST: pixel m = y w + x -> out[y sy + x sx + n sc]
    long long sy = 0, sx = 0, sc = 0;

    __device__ void operator()(int m, int n, float v) const {
        const long long i = (long long)m * n_real + n;
        if (mode == VG_PLAIN) {
            out[i] = v;
        } else if (mode == VG_GATE) {
            const float y = ys[i];
            if (yt != nullptr) {
                const float d = y - yt[i];
                v += (float)((d > 0.f) - (d < 0.f)) * (*g_loss * inv_numel);
            }
            out[i] = y > 0.f ? v : 0.f;
        } else if (n < n_real) {
            const int y = m / w, x = m - y * w;
            out[y * sy + x * sx + n * sc] = v;
        }
    }
};

// the gradient at the last tap: the epilogue on zeros
__global__ void __launch_bounds__(256) k_vg_seed(long long total, VgEpi epi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    epi((int)(i / epi.n_real), (int)(i % epi.n_real), 0.f);
}

// ---- the pool, backward ---------------------------------------------------------------------------------------------------------------
// y [h, w, c] (>= 0: ReLU outputs), dp [h / 2, w / 2, c] -> g [h, w, c]: dp at the first maximum of each window (row-major order), where
// that maximum is positive; 0 elsewhere and in the row / column an odd size leaves outside every window
__global__ void __launch_bounds__(256) k_vg_pool_bwd(const float* __restrict__ y, const float* __restrict__ dp, int h, int w, int c, float* __restrict__ g) {
    const int ho = h / 2, wo = w / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)h * w * c;
    if (i >= total) return;
    const int ch = (int)(i % c);
    const long long p = i / c;
    const int x = (int)(p % w), yy = (int)(p / w);
    float out = 0.f;
    if (yy < 2 * ho && x < 2 * wo) {
        const float* s = y + ((long long)(yy & ~1) * w + (x & ~1)) * c + ch;
        const float v00 = s[0], v01 = s[c], v10 = s[(long long)w * c], v11 = s[(long long)w * c + c];
        int arg = 0;
        float mx = v00;
        if (v01 > mx) mx = v01, arg = 1;
        if (v10 > mx) mx = v10, arg = 2;
        if (v11 > mx) mx = v11, arg = 3;
        if (arg == (yy & 1) * 2 + (x & 1) && mx > 0.f) out = dp[((long long)(yy >> 1) * wo + (x >> 1)) * c + ch];
    }
    g[i] = out;
}

// ---- the L1 means ------------------------------------------------------------------------------------------------------------------
struct VgTaps {
    const float* p[VG_TAPS];             // source [numel], then target [numel]
    long long numel[VG_TAPS];            // multiples of 64
};

// grid (blocks of the largest tap, 5) -> partial [5, gridDim.x]
__global__ void __launch_bounds__(L1_THREADS) k_vg_l1(VgTaps taps, double* __restrict__ partial) {
    __shared__ double red[L1_THREADS / 64];
    const int k = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* s = taps.p[k];
    const long long numel = taps.numel[k];
    const float* t = s + numel;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = (long long)blockIdx.x * L1_PER_BLOCK + (long long)(j * L1_THREADS + threadIdx.x) * 4;
        if (i < numel) {
            const float4 a = *(const float4*)(s + i), b = *(const float4*)(t + i);
            sum += (double)fabsf(a.x - b.x);
            sum += (double)fabsf(a.y - b.y);
            sum += (double)fabsf(a.z - b.z);
            sum += (double)fabsf(a.w - b.w);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < L1_THREADS / 64; ++j) v += red[j];
        partial[(long long)k * gridDim.x + blockIdx.x] = v;
    }
}

// one wave: terms [6] = loss, the five tap means
__global__ void __launch_bounds__(64) k_vg_l1_final(const double* __restrict__ partial, int blocks, VgTaps taps, float* __restrict__ terms) {
    double total = 0.0;
    for (int k = 0; k < VG_TAPS; ++k) {
        double v = 0.0;
        for (int j = threadIdx.x; j < blocks; j += 64) v += partial[(long long)k * blocks + j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        const double mean = v / (double)taps.numel[k];
        total += mean;
        if (threadIdx.x == 0) terms[1 + k] = (float)mean;
    }
    if (threadIdx.x == 0) terms[0] = (float)total;
}

// ---- shapes and the workspace ------------------------------------------------------------------------------------------------------
struct VgShape {
    int h[VG_TAPS], w[VG_TAPS];                          // per level
    size_t col, y[VG_CONVS], pool[VG_TAPS - 1], partial, l1, ga, gb, dp;       // byte offsets into the workspace
    int l1_blocks;
};

inline int vg_tapmask(int h, int w) {
    int mask = 0;
    for (int tap = 0; tap < 9; ++tap)
        if ((tap / 3 == 1 || h > 1) && (tap % 3 == 1 || w > 1)) mask |= 1 << tap;
    return mask;
}

inline int vg_live_taps(int h, int w) { return (h > 1 ? 3 : 1) * (w > 1 ? 3 : 1); }

// splits of the K chunks of a launch of M rows x npad columns: 1 where the tiles alone fill the machine
inline int vg_splits(long long M, int npad, int n_chunks) {
    const long long blocks = (M + CV_BM - 1) / CV_BM * (npad / CV_BN);
    if (blocks >= VG_TARGET_BLOCKS) return 1;
    const long long s = (VG_TARGET_BLOCKS + blocks - 1) / blocks;
    return (int)(s < n_chunks ? s : n_chunks);
}

int vg_shape(const char* who, long long height, long long width, VgShape& s, size_t& bytes) {
    HN_REQUIRE(height >= VG_MIN_SIDE && width >= VG_MIN_SIDE, "%s: height = %lld, width = %lld: at least %d x %d (the fifth tap is floor(H / 16) x floor(W / 16))", who,
               height, width, VG_MIN_SIDE, VG_MIN_SIDE);
    HN_REQUIRE(height < VG_MAX && width < VG_MAX && height * width < VG_MAX && 2 * height * width < VG_MAX / 64,
               "%s: height = %lld, width = %lld: the largest activation, 2 x height x width x 64, must stay below 2^31", who, height, width);
    for (int k = 0; k < VG_TAPS; ++k) {
        s.h[k] = (int)(height >> k);
        s.w[k] = (int)(width >> k);
    }
    const size_t px = (size_t)(height * width);
    size_t off = 0, part = 0;
    s.col = off;
    off += up256(2 * px * CV_KC * sizeof(float));
    for (int l = 0; l < VG_CONVS; ++l) {
        const int lv = VG_LEVEL[l];
        const size_t hw = (size_t)s.h[lv] * s.w[lv];
        s.y[l] = off;
        off += up256(2 * hw * VG_COUT[l] * sizeof(float));
        if (l > 0 && VG_LEVEL[l - 1] != lv) {
            s.pool[lv - 1] = off;
            off += up256(2 * hw * VG_CIN[l] * sizeof(float));
        }
        // the partial tiles of this layer's launches, forward (2 images) and backward-data (1 image)
        const int live = l == 0 ? 1 : vg_live_taps(s.h[lv], s.w[lv]);
        const int kf = l == 0 ? CV_KC : VG_CIN[l];
        const int sf = vg_splits(2 * (long long)hw, VG_COUT[l], live * kf / CV_KC);
        if (sf > 1 && (size_t)sf * 2 * hw * VG_COUT[l] > part) part = (size_t)sf * 2 * hw * VG_COUT[l];
        const int nb = cv_npad(VG_CIN[l]);
        const int sb = vg_splits((long long)hw, nb, vg_live_taps(s.h[lv], s.w[lv]) * VG_COUT[l] / CV_KC);
        if (sb > 1 && (size_t)sb * hw * nb > part) part = (size_t)sb * hw * nb;
    }
    s.partial = off;
    off += up256(part * sizeof(float));
    s.l1_blocks = (int)((px * 64 + L1_PER_BLOCK - 1) / L1_PER_BLOCK);
    s.l1 = off;
    off += up256((size_t)VG_TAPS * s.l1_blocks * sizeof(double));
    s.ga = off;
    off += up256(px * 64 * sizeof(float));
    s.gb = off;
    off += up256(px * 64 * sizeof(float));
    s.dp = off;
    off += up256(px * 64 * sizeof(float));
    bytes = off;
    return HN_OK;
}

// one convolution, either direction: in [M = n_img h w, kc] against the packing wpk of npad rows, live taps only, split by vg_splits
template <class Epi>
int vg_conv(const float* in, const float4* wpk, long long M, int h, int w, int kc, int npad, bool single, float* partial, const Epi& epi, hipStream_t s) {
    const int n_chunks = (single ? 1 : vg_live_taps(h, w)) * (kc / CV_KC);
    return cv_conv<true, true>(in, wpk, M, h, w, kc, npad, single, vg_tapmask(h, w), n_chunks, vg_splits(M, npad, n_chunks), partial, epi, s);
}

int vg_check_strides(const char* who, long long h, long long w, long long sy, long long sx, long long sc) {
    HN_REQUIRE(sy > 0 && sx > 0 && sc > 0, "%s: strides (%lld, %lld, %lld) must be positive", who, sy, sx, sc);
    HN_REQUIRE(sy < VG_MAX && sx < VG_MAX && sc < VG_MAX && (h - 1) * sy + (w - 1) * sx + 2 * sc < VG_MAX,
               "%s: strides (%lld, %lld, %lld) reach beyond 2^31 elements", who, sy, sx, sc);
    return HN_OK;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

int hn_vgg_loss_create(const float* const* conv_weight, const float* const* conv_bias, hn_vgg_loss_model** out, hn_stream_t stream) {
    HN_REQUIRE(conv_weight && conv_bias && out, "hn_vgg_loss_create: NULL conv_weight / conv_bias / out");
    for (int l = 0; l < VG_CONVS; ++l) HN_REQUIRE(conv_weight[l] && conv_bias[l], "hn_vgg_loss_create: NULL weight or bias of convolution %d", l);
    hipStream_t s = (hipStream_t)stream;
    size_t off_f[VG_CONVS], off_r[VG_CONVS], off_b[VG_CONVS], off = 0;
    for (int l = 0; l < VG_CONVS; ++l) {
        off_f[l] = off;
        off += up256(cv_pack_floats(VG_CIN[l], VG_COUT[l], 0) * sizeof(float));
        off_r[l] = off;
        off += up256(cv_pack_floats(VG_CIN[l], VG_COUT[l], 1) * sizeof(float));
        off_b[l] = off;
        off += up256((size_t)VG_COUT[l] * sizeof(float));
    }
    void* blob = nullptr;
    HN_CHECK_HIP(hipMalloc(&blob, off));
    hn_vgg_loss_model* m = new hn_vgg_loss_model();
    m->blob = blob;
    int rc = HN_OK;
    auto fail = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == HN_OK) {
            set_error("hn_vgg_loss_create: %s failed: %s", what, hipGetErrorString(e));
            rc = HN_EHIP;
        }
    };
    for (int l = 0; l < VG_CONVS && rc == HN_OK; ++l) {
        float* wf = (float*)((char*)blob + off_f[l]);
        float* wr = (float*)((char*)blob + off_r[l]);
        fail(cv_pack(conv_weight[l], VG_CIN[l], VG_COUT[l], 0, wf, s), "the forward pack launch");
        fail(cv_pack(conv_weight[l], VG_CIN[l], VG_COUT[l], 1, wr, s), "the backward pack launch");
        fail(hipMemcpyAsync((char*)blob + off_b[l], conv_bias[l], VG_COUT[l] * sizeof(float), hipMemcpyDeviceToDevice, s), "the bias copy");
        m->wf[l] = (const float4*)wf;
        m->wb[l] = (const float4*)wr;
        m->bias[l] = (const float*)((char*)blob + off_b[l]);
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

int hn_vgg_loss_destroy(hn_vgg_loss_model* m) {
    if (m == nullptr) return HN_OK;
    if (m->blob != nullptr) HN_CHECK_HIP(hipFree(m->blob));
    delete m;
    return HN_OK;
}

size_t hn_vgg_loss_workspace_bytes(long long height, long long width) {
    VgShape sh;
    size_t bytes = 0;
    return vg_shape("hn_vgg_loss_workspace_bytes", height, width, sh, bytes) == HN_OK ? bytes : 0;
}

int hn_vgg_loss_fwd(const hn_vgg_loss_model* model, const float* source, const float* target, long long height, long long width, long long stride_y,
                    long long stride_x, long long stride_c, float* terms, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    VgShape sh;
    size_t need = 0;
    HN_TRY_RC(vg_shape("hn_vgg_loss_fwd", height, width, sh, need));
    HN_REQUIRE(model && source && target && terms && workspace, "hn_vgg_loss_fwd: NULL model / source / target / terms / workspace");
    HN_TRY_RC(vg_check_strides("hn_vgg_loss_fwd", height, width, stride_y, stride_x, stride_c));
    HN_REQUIRE(workspace_bytes >= need, "hn_vgg_loss_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)terms & 3) == 0, "hn_vgg_loss_fwd: workspace not 16-byte aligned, or terms not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* partial = (float*)(ws + sh.partial);
    float* col = (float*)(ws + sh.col);
    HN_TRY_RC(cv_im2col(VgLoad{source, target, stride_y, stride_x, stride_c}, 2, sh.h[0], sh.w[0], col, s));
    const float* x = col;
    for (int l = 0; l < VG_CONVS; ++l) {
        const int lv = VG_LEVEL[l], h = sh.h[lv], w = sh.w[lv];
        if (l > 0 && VG_LEVEL[l - 1] != lv) {
            float* pooled = (float*)(ws + sh.pool[lv - 1]);
            HN_TRY_RC(cv_pool(x, pooled, 2, sh.h[lv - 1], sh.w[lv - 1], VG_CIN[l], s));
            x = pooled;
        }
        const CvFwd e{model->bias[l], (float*)(ws + sh.y[l]), VG_COUT[l]};
        HN_TRY_RC(vg_conv(x, model->wf[l], 2LL * h * w, h, w, l == 0 ? CV_KC : VG_CIN[l], VG_COUT[l], l == 0, partial, e, s));
        x = e.out;
    }
    VgTaps taps;
    for (int l = 0; l < VG_CONVS; ++l)
        if (VG_TAP_OF[l] >= 0) {
            const int lv = VG_LEVEL[l];
            taps.p[VG_TAP_OF[l]] = (const float*)(ws + sh.y[l]);
            taps.numel[VG_TAP_OF[l]] = (long long)sh.h[lv] * sh.w[lv] * VG_COUT[l];
        }
    double* l1 = (double*)(ws + sh.l1);
    k_vg_l1<<<dim3((unsigned)sh.l1_blocks, VG_TAPS), L1_THREADS, 0, s>>>(taps, l1);
    HN_LAUNCH_CHECK();
    k_vg_l1_final<<<1, 64, 0, s>>>(l1, sh.l1_blocks, taps, terms);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_vgg_loss_bwd(const hn_vgg_loss_model* model, long long height, long long width, long long stride_y, long long stride_x, long long stride_c,
                    const float* g_loss, void* workspace, size_t workspace_bytes, float* g_source, hn_stream_t stream) {
    VgShape sh;
    size_t need = 0;
    HN_TRY_RC(vg_shape("hn_vgg_loss_bwd", height, width, sh, need));
    HN_REQUIRE(model && g_loss && workspace && g_source, "hn_vgg_loss_bwd: NULL model / g_loss / workspace / g_source");
    HN_TRY_RC(vg_check_strides("hn_vgg_loss_bwd", height, width, stride_y, stride_x, stride_c));
    HN_REQUIRE(workspace_bytes >= need, "hn_vgg_loss_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)g_loss & 3) == 0 && ((uintptr_t)g_source & 3) == 0,
               "hn_vgg_loss_bwd: workspace not 16-byte aligned, or g_loss / g_source not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* partial = (float*)(ws + sh.partial);
    float *cur = (float*)(ws + sh.ga), *other = (float*)(ws + sh.gb), *dp = (float*)(ws + sh.dp);
    auto gate = [&](int l, float* out) {               // the epilogue of a gradient that lands on layer l's output
        const int lv = VG_LEVEL[l];
        const long long numel = (long long)sh.h[lv] * sh.w[lv] * VG_COUT[l];
        VgEpi e;
        e.mode = VG_GATE;
        e.n_real = VG_COUT[l];
        e.ys = (const float*)(ws + sh.y[l]);
        e.yt = VG_TAP_OF[l] >= 0 ? e.ys + numel : nullptr;
        e.g_loss = g_loss;
        e.inv_numel = (float)(1.0 / (double)numel);
        e.out = out;
        return e;
    };
    {
        const int lv = VG_LEVEL[VG_CONVS - 1];
        const long long total = (long long)sh.h[lv] * sh.w[lv] * VG_COUT[VG_CONVS - 1];
        k_vg_seed<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(total, gate(VG_CONVS - 1, cur));
        HN_LAUNCH_CHECK();
    }
    for (int l = VG_CONVS - 1; l >= 1; --l) {
        const int lv = VG_LEVEL[l], h = sh.h[lv], w = sh.w[lv];
        const bool pooled = VG_LEVEL[l - 1] != lv;
        VgEpi e;
        if (pooled) {
            e.mode = VG_PLAIN;
            e.n_real = VG_CIN[l];
            e.out = dp;
        } else {
            e = gate(l - 1, other);
        }
        HN_TRY_RC(vg_conv(cur, model->wb[l], (long long)h * w, h, w, VG_COUT[l], VG_CIN[l], false, partial, e, s));
        if (pooled) {
            const int hp = sh.h[lv - 1], wp = sh.w[lv - 1];
            const long long total = (long long)hp * wp * VG_CIN[l];
            k_vg_pool_bwd<<<(unsigned)((total + 255) / 256), 256, 0, s>>>((const float*)(ws + sh.y[l - 1]), dp, hp, wp, VG_CIN[l], other);
            HN_LAUNCH_CHECK();
        }
        float* tmp = cur;
        cur = other;
        other = tmp;
    }
    VgEpi e;
    e.mode = VG_LAST;
    e.n_real = 3;
    e.out = g_source;
    e.w = sh.w[0];
    e.sy = stride_y;
    e.sx = stride_x;
    e.sc = stride_c;
    HN_TRY_RC(vg_conv(cur, model->wb[0], (long long)sh.h[0] * sh.w[0], sh.h[0], sh.w[0], VG_COUT[0], cv_npad(VG_CIN[0]), false, partial, e, s));
    return HN_OK;
}

}  // extern "C"
