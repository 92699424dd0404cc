// LPIPS (VGG16, version 0.1, linear layers on, spatial off, eval mode) on the device: the third column of
// analys_results/analys_psnr_ssim_lpips.py:28-33,44 (lpips.LPIPS(net='vgg') on x = u8 / 128 - 1) for F pairs of 8-bit interleaved RGB
// images [F, H, W, 3] of one size.  tests/test_lpips_cpu.py restates it in float64 torch; DESIGN.md 3.18 is the contract.
//
// The model (hn_lpips_create) holds the 13 convolutions' weights packed once into MFMA fragment order, their biases and the five
// 1x1 linear weight vectors.  A call runs the 2 F images (a's, then b's) through the whole stack as ONE batch: activations are
// channel-last fp32 [N, h, w, C] in the caller's workspace, so the K axis of every convolution (tap-major: k = (3 ky + kx) Cin + c) is
// contiguous in memory.  No allocation, no synchronisation, no floating-point atomics: every output element is one fmaf chain in a
// fixed order that does not depend on where its tile lies, every reduction combines its partials in a fixed order per image, so a
// repeated call, another batch size or another position in the batch give the same bits.
//
// Precision: exact fp32, v_mfma_f32_32x32x2_f32 (each output = one fp32 fmaf chain over K, the bias added after it).  Activations of
// trained VGG weights are not known here and nothing bounds them to fp16's range, which rules out fp16 operands without a per-layer
// rescale; the fp32 MFMA needs none.
//
// Kernels:
//   k_lp_pack        [Cout, Cin, 3, 3] -> fragments [Cout / 32][Kpad / 8][64 lanes] float4: lane l holds W[n = 32 nt + (l & 31)]
//                    [k = 8 g + 4 (l >> 5) + 0..3], zero for k >= 9 Cin (the first layer: K = 27 -> 32)
//   k_lp_im2col      the scaling layer and the first layer's patch gather: u8 -> ((u8 / 128 - 1) - shift) / scale, the 27 values of
//                    the 3 x 3 x 3 patch (zero outside the image, as the zero padding of the SCALED input is) + 5 zeros -> [N, H, W, 32]:
//                    the first convolution then is the same kernel with one tap and Cin = 32
//   k_lp_conv        implicit GEMM, 128 output pixels x 64 output channels per workgroup of 4 waves (2 x 2: a wave owns 64 pixels x 32
//                    channels = two 32 x 32 accumulators), K in chunks of 32 channels of one tap.  A chunk's 128 x 32 activations
//                    (zeros where the tap leaves the image) and its 64 x 32 weights go global -> registers -> LDS, the next chunk's
//                    loads in flight while this chunk's 32 MFMAs per wave run, two LDS buffers, one barrier per chunk.  One
//                    ds_read_b128 feeds 4 k-steps (lane half h takes k = 4 h + 0..3 of each group of 8: the order of k inside a
//                    group is free as long as both operands agree).  The A tile's pitch of 36 floats keeps those reads free of bank
//                    conflicts.  Epilogue: + bias, ReLU, 128-byte row stores.
//   k_lp_pool        MaxPool2d(2, 2), floor mode: [N, h, w, C] -> [N, h / 2, w / 2, C]
//   k_lp_head        per pixel of a tap (one wave per pixel, lanes over channels): n(f) = f / (sqrt(sum_c f^2) + 1e-10) for both
//                    images, sum_c w[c] (n(fa) - n(fb))^2 in fp32, summed over the wave's 16 pixels and the workgroup's 4 waves in fp64
//                    -> one partial per 64 pixels
//   k_lp_head_final  one wave per pair: strided sum of the partials, butterfly, the mean -> per_tap [F, 5]
//   k_lp_nchw        a tap [N, h, w, C] -> torch's [N, C, h, w] (hn_lpips_features)
#include "hn_common.h"

struct hn_lpips_model {
    void* blob = nullptr;                // one device allocation: packed weights, biases, linear weights
    const float4* wpk[13] = {};
    const float* bias[13] = {};
    const float* lin[5] = {};
};

namespace hn {
namespace {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LP_CONVS = 13, LP_TAPS = 5;
constexpr int LP_CIN[LP_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_TAP_C[LP_TAPS] = {64, 128, 256, 512, 512};
constexpr int LP_MIN_SIDE = 16;                                   // the fifth tap is floor(H / 16) x floor(W / 16)
constexpr long long LP_MAX = 1LL << 31;                           // N H W 64, the largest activation, stays below this

constexpr int CV_BM = 128, CV_BN = 64, CV_KC = 32, CV_THREADS = 256;
constexpr int CV_APITCH = CV_KC + 4;                              // floats; 36 l mod 64 is a different multiple of 4 for 16 lanes
constexpr int CV_A_FLOATS = CV_BM * CV_APITCH;                    // per buffer
constexpr int CV_B_FLOAT4 = (CV_BN / 32) * (CV_KC / 8) * 64;      // per buffer: 512 float4
static_assert(CV_A_FLOATS * 4 * 2 + CV_B_FLOAT4 * 16 * 2 <= 64 * 1024, "static LDS");
static_assert(CV_BM * (CV_KC / 4) == 4 * CV_THREADS && CV_B_FLOAT4 == 2 * CV_THREADS, "loads per thread and chunk");

constexpr int HEAD_THREADS = 256, HEAD_PX_WAVE = 16, HEAD_PX = (HEAD_THREADS / 64) * HEAD_PX_WAVE;

__host__ __device__ inline int lp_kpad(int cin) { return (9 * cin + CV_KC - 1) / CV_KC * CV_KC; }

// ---- weights -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lp_pack(const float* __restrict__ w, int cin, int cout, float* __restrict__ out) {
    const int kpad = lp_kpad(cin), groups = kpad / 8;
    const long long total = (long long)cout * kpad;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const long long fg = i >> 8;                                   // nt * groups + g
    const int g = (int)(fg % groups), nt = (int)(fg / groups);
    const int n = 32 * nt + (lane & 31), k = 8 * g + 4 * (lane >> 5) + j;
    float v = 0.f;
    if (k < 9 * cin) {
        const int tap = k / cin, c = k - tap * cin;
        v = w[((long long)n * cin + c) * 9 + tap];
    }
    out[i] = v;
}

// ---- the scaling layer + the first layer's patches -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lp_im2col(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int n_a, int n_img,
                                                   int h, int w, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // (pixel m, quarter q): k = 4 q .. 4 q + 3
    const long long M = (long long)n_img * h * w;
    if (i >= M * 8) return;
    const long long m = i >> 3;
    const int q = (int)(i & 7);
    const int f = (int)(m / ((long long)h * w));
    const int rem = (int)(m - (long long)f * h * w), y = rem / w, x = rem - y * w;
    const unsigned char* img = f < n_a ? a + (long long)f * h * w * 3 : b + (long long)(f - n_a) * h * w * 3;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        v[j] = 0.f;
        if (k < 27) {
            const int tap = k / 3, c = k - 3 * tap, yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                const float shift = c == 0 ? -0.030f : c == 1 ? -0.088f : -0.188f;
                const float scale = c == 0 ? 0.458f : c == 1 ? 0.448f : 0.450f;
                const float u = (float)img[((long long)yy * w + xx) * 3 + c] / 128.f - 1.f;          // exact
                v[j] = (u - shift) / scale;
            }
        }
    }
    *(float4*)(out + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------
// in [n_img, h, w, cin] (cin a multiple of 32), taps = 9: 3 x 3, zero padding 1; taps = 1: the pixel itself.  out [n_img, h, w, cout].
__global__ void __launch_bounds__(CV_THREADS) k_lp_conv(const float* __restrict__ in, const float4* __restrict__ wpk, const float* __restrict__ bias,
                                                        float* __restrict__ out, int M, int h, int w, int cin, int cout, int taps) {
    __shared__ __attribute__((aligned(16))) float sA[2][CV_A_FLOATS];
    __shared__ float4 sB[2][CV_B_FLOAT4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * CV_BM, by = blockIdx.y;
    const int cchunks = cin / CV_KC, n_chunks = taps * cchunks, groups = n_chunks * (CV_KC / 8);
    // the four tile rows this thread stages: r = (t >> 3) + 32 i, floats 4 q .. 4 q + 3 of the chunk
    const int q = t & 7;
    int py[4], px[4];
    bool pv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + (t >> 3) + 32 * i;
        pv[i] = m < M;
        const int rem = pv[i] ? m % (h * w) : 0;
        py[i] = rem / w;
        px[i] = rem - py[i] * w;
    }
    lp_f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    // step ch: fetch chunk ch + 1 into registers, run chunk ch from LDS buffer ch & 1, park the registers in the other buffer, barrier
    // (that buffer was last read in step ch - 1, which every wave has left).  Step -1 only fetches and parks chunk 0.
    for (int ch = -1; ch < n_chunks; ++ch) {
        const int buf = ch & 1, nx = ch + 1;
        const bool more = nx < n_chunks;
        float4 ra0, ra1, ra2, ra3, rb0, rb1;
        ra0 = ra1 = ra2 = ra3 = rb0 = rb1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (more) {
            const int tap = nx / cchunks, c0 = (nx - tap * cchunks) * CV_KC;
            const int dy = taps == 9 ? tap / 3 - 1 : 0, dx = taps == 9 ? tap % 3 - 1 : 0;
            // (py + dy, px + dx) inside the image: then pixel m + dy w + dx is that neighbour, in the same image
            const float* src = in + ((long long)m0 + (t >> 3) + dy * w + dx) * cin + c0 + 4 * q;
            const long long step = 32LL * cin;
            if (pv[0] && (unsigned)(py[0] + dy) < (unsigned)h && (unsigned)(px[0] + dx) < (unsigned)w) ra0 = *(const float4*)(src);
            if (pv[1] && (unsigned)(py[1] + dy) < (unsigned)h && (unsigned)(px[1] + dx) < (unsigned)w) ra1 = *(const float4*)(src + step);
            if (pv[2] && (unsigned)(py[2] + dy) < (unsigned)h && (unsigned)(px[2] + dx) < (unsigned)w) ra2 = *(const float4*)(src + 2 * step);
            if (pv[3] && (unsigned)(py[3] + dy) < (unsigned)h && (unsigned)(px[3] + dx) < (unsigned)w) ra3 = *(const float4*)(src + 3 * step);
            const float4* wsrc = wpk + ((long long)(2 * by) * groups + nx * (CV_KC / 8)) * 64 + t;
            rb0 = wsrc[0];
            rb1 = wsrc[(long long)groups * 64];
        }
        if (ch >= 0) {
#pragma unroll
            for (int g = 0; g < CV_KC / 8; ++g) {
                const float4 bv = sB[buf][wn * 256 + g * 64 + lane];
                float4 av[2];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    av[mt] = *(const float4*)(&sA[buf][(64 * wm + 32 * mt + (lane & 31)) * CV_APITCH + 8 * g + 4 * (lane >> 5)]);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt].x, bv.x, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt].y, bv.y, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt].z, bv.z, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt].w, bv.w, acc[mt], 0, 0, 0);
                }
            }
        }
        if (more) {
            float* dst = &sA[buf ^ 1][(t >> 3) * CV_APITCH + 4 * q];
            *(float4*)(dst) = ra0;
            *(float4*)(dst + 32 * CV_APITCH) = ra1;
            *(float4*)(dst + 64 * CV_APITCH) = ra2;
            *(float4*)(dst + 96 * CV_APITCH) = ra3;
            sB[buf ^ 1][t] = rb0;
            sB[buf ^ 1][256 + t] = rb1;
        }
        __syncthreads();
    }
    // accumulator register r of lane l: pixel row (r & 3) + 8 (r >> 2) + 4 (l >> 5), channel column l & 31
    const int n = CV_BN * by + 32 * wn + (lane & 31);
    const float bn = bias[n];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 64 * wm + 32 * mt + tile_row(r, lane >> 5);
            if (m < M) out[(long long)m * cout + n] = fmaxf(acc[mt][r] + bn, 0.f);
        }
}

// ---- the pool ----------------------------------------------------------------------------------------------------------------------
__device__ inline float4 max4(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }

__global__ void __launch_bounds__(256) k_lp_pool(const float* __restrict__ in, int n_img, int h, int w, int c, float* __restrict__ out) {
    const int ho = h / 2, wo = w / 2, c4 = c / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)n_img * ho * wo * c4;
    if (i >= total) return;
    const int cq = (int)(i % c4);
    const long long p = i / c4;
    const int x = (int)(p % wo), y = (int)((p / wo) % ho), f = (int)(p / ((long long)wo * ho));
    const float* s = in + (((long long)f * h + 2 * y) * w + 2 * x) * c + 4 * cq;          // rows 2 y, 2 y + 1 < h; columns 2 x, 2 x + 1 < w
    const float4 v = max4(max4(*(const float4*)s, *(const float4*)(s + c)), max4(*(const float4*)(s + (long long)w * c), *(const float4*)(s + (long long)w * c + c)));
    *(float4*)(out + i * 4) = v;
}

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

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

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

int lp_conv(const hn_lpips_model* m, int layer, const float* in, float* out, long long n_img, int h, int w, hipStream_t s) {
    const int first = layer == 0, cin = first ? CV_KC : LP_CIN[layer], cout = LP_COUT[layer];
    const long long M = n_img * h * w;
    k_lp_conv<<<dim3((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)(cout / CV_BN)), CV_THREADS, 0, s>>>(in, m->wpk[layer], m->bias[layer], out, (int)M, h, w, cin,
                                                                                                             cout, first ? 1 : 9);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int lp_pool(const float* in, float* out, long long n_img, int h, int w, int c, hipStream_t s) {
    const long long total = n_img * (h / 2) * (w / 2) * (c / 4);
    k_lp_pool<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(in, (int)n_img, h, w, c, out);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

// the five taps of n_a images of `a` followed by n_b of `b`, channel-last, at sh.tap[] of the workspace
int lp_stack(const hn_lpips_model* m, const unsigned char* a, const unsigned char* b, long long n_a, long long n_b, const LpShape& sh, char* ws, hipStream_t s) {
    const long long n = n_a + n_b;
    float *s0 = (float*)(ws + sh.s0), *s1 = (float*)(ws + sh.s1);
    float* tap[LP_TAPS];
    for (int k = 0; k < LP_TAPS; ++k) tap[k] = (float*)(ws + sh.tap[k]);
    const long long quarters = n * sh.h[0] * sh.w[0] * 8;
    k_lp_im2col<<<(unsigned)((quarters + 255) / 256), 256, 0, s>>>(a, b, (int)n_a, (int)n, sh.h[0], sh.w[0], s1);
    HN_LAUNCH_CHECK();
    HN_TRY_RC(lp_conv(m, 0, s1, s0, n, sh.h[0], sh.w[0], s));
    HN_TRY_RC(lp_conv(m, 1, s0, tap[0], n, sh.h[0], sh.w[0], s));
    HN_TRY_RC(lp_pool(tap[0], s1, n, sh.h[0], sh.w[0], 64, s));
    HN_TRY_RC(lp_conv(m, 2, s1, s0, n, sh.h[1], sh.w[1], s));
    HN_TRY_RC(lp_conv(m, 3, s0, tap[1], n, sh.h[1], sh.w[1], s));
    HN_TRY_RC(lp_pool(tap[1], s1, n, sh.h[1], sh.w[1], 128, s));
    HN_TRY_RC(lp_conv(m, 4, s1, s0, n, sh.h[2], sh.w[2], s));
    HN_TRY_RC(lp_conv(m, 5, s0, s1, n, sh.h[2], sh.w[2], s));
    HN_TRY_RC(lp_conv(m, 6, s1, tap[2], n, sh.h[2], sh.w[2], s));
    HN_TRY_RC(lp_pool(tap[2], s0, n, sh.h[2], sh.w[2], 256, s));
    HN_TRY_RC(lp_conv(m, 7, s0, s1, n, sh.h[3], sh.w[3], s));
    HN_TRY_RC(lp_conv(m, 8, s1, s0, n, sh.h[3], sh.w[3], s));
    HN_TRY_RC(lp_conv(m, 9, s0, tap[3], n, sh.h[3], sh.w[3], s));
    HN_TRY_RC(lp_pool(tap[3], s0, n, sh.h[3], sh.w[3], 512, s));
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
        off += up256((size_t)LP_COUT[l] * lp_kpad(LP_CIN[l]) * sizeof(float));
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
        const long long total = (long long)LP_COUT[l] * lp_kpad(LP_CIN[l]);
        k_lp_pack<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(conv_weight[l], LP_CIN[l], LP_COUT[l], w);
        fail(hipGetLastError(), "the pack launch");
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
