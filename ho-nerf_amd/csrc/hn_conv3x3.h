// The exact-fp32 3 x 3 convolution stack that LPIPS (hn_lpips.hip, VGG16) and the perceptual loss of training (hn_vggloss.hip, VGG19,
// forward and backward-data) both run: weight packing, the first layer's patch gather, the implicit-GEMM convolution with its K split
// and live-tap list, the split partials' sum, MaxPool2d(2, 2) and the host launchers.  DESIGN.md 3.18 describes it.
//
// Header only: everything here is a template or lives in the unnamed namespace, so each of the two .hip files compiles its own copy
// under its own -ffp-contract setting (the Makefile gives hn_lpips.hip `off` for its head, hn_vggloss.hip the default for its VG_GATE
// epilogue).  Nothing in this file has a multiply feeding an add outside the MFMA builtins, which no contraction setting touches.
//
// Activations are channel-last fp32 [N, h, w, C], so the K axis of every convolution (tap-major: k = (3 ky + kx) Cin + c) is contiguous
// in memory.  Every output element is one fp32 fmaf chain over its K range in a fixed order that does not depend on where its tile
// lies; a split launch adds the ranges' partial sums in index order.
//
// Precision: exact fp32, v_mfma_f32_32x32x2_f32 (each output = one fp32 fmaf chain over K, the bias added after it).  Activations of
// trained VGG weights are not known here and nothing bounds them to fp16's range, which rules out fp16 operands without a per-layer
// rescale; the fp32 MFMA needs none.
//
// Kernels:
//   k_cv_pack        [Cout, Cin, 3, 3] -> fragments [N / 32][Kpad / 8][64 lanes] float4: lane l holds W[n = 32 nt + (l & 31)]
//                    [k = 8 g + 4 (l >> 5) + 0..3], zero for k beyond 9 x the K channels (the first layer: K = 27 -> 32); forward
//                    (N = Cout, K = 9 Cin) or backward-data (N = Cin padded to one N tile, K = 9 Cout, taps flipped)
//   k_cv_im2col      the first layer's patch gather: the 27 values of the 3 x 3 x 3 patch (zero outside the image) + 5 zeros
//                    -> [N, H, W, 32], each value fetched by the caller's loader: the first convolution then is the same kernel with
//                    one tap and Cin = 32
//   k_cv_conv        implicit GEMM, 128 output pixels x 64 output channels per workgroup of 4 waves (2 x 2: a wave owns 64 pixels x 32
//                    channels = two 32 x 32 accumulators), K in chunks of 32 channels of one tap.  A chunk's 128 x 32 activations
//                    (zeros where the tap leaves the image) and its 64 x 32 weights go global -> registers -> LDS, the next chunk's
//                    loads in flight while this chunk's 32 MFMAs per wave run, two LDS buffers, one barrier per chunk.  One
//                    ds_read_b128 feeds 4 k-steps (lane half h takes k = 4 h + 0..3 of each group of 8: the order of k inside a
//                    group is free as long as both operands agree).  The A tile's pitch of 36 floats keeps those reads free of bank
//                    conflicts.  blockIdx.z splits the K chunks, each split writing its partial tile, so that a layer of a few rows
//                    still occupies every CU; taps outside the caller's mask are neither loaded nor multiplied.  An unsplit launch
//                    runs the epilogue itself, 128-byte row stores.
//   k_cv_reduce      sums the splits' partials in index order, then the epilogue
//   the epilogue     a functor epi(m, n, v): CvFwd below (+ bias, ReLU) or the including file's own
//   k_cv_pool        MaxPool2d(2, 2), floor mode: [N, h, w, C] -> [N, h / 2, w / 2, C]
#pragma once
#include "hn_common.h"

namespace hn {
namespace {

typedef float cv_f32x16 __attribute__((ext_vector_type(16)));

constexpr int CV_BM = 128, CV_BN = 64, CV_KC = 32, CV_THREADS = 256;
constexpr int CV_APITCH = CV_KC + 4;                              // floats; 36 l mod 64 is a different multiple of 4 for 16 lanes
constexpr int CV_A_FLOATS = CV_BM * CV_APITCH;                    // per buffer
constexpr int CV_B_FLOAT4 = (CV_BN / 32) * (CV_KC / 8) * 64;      // per buffer: 512 float4
static_assert(CV_A_FLOATS * 4 * 2 + CV_B_FLOAT4 * 16 * 2 <= 64 * 1024, "static LDS");
static_assert(CV_BM * (CV_KC / 4) == 4 * CV_THREADS && CV_B_FLOAT4 == 2 * CV_THREADS, "loads per thread and chunk");
constexpr int CV_ALL_TAPS = 0x1ff;                                // bit 3 (dy + 1) + (dx + 1)

__host__ __device__ inline int cv_kpad(int k_channels) { return (9 * k_channels + CV_KC - 1) / CV_KC * CV_KC; }
__host__ __device__ inline int cv_npad(int n) { return (n + CV_BN - 1) / CV_BN * CV_BN; }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- weights -----------------------------------------------------------------------------------------------------------------------
// forward:  N = cout, k = tap cin + c        -> w[n, c, tap]
// backward: N = cin (padded to 64), k = tap cout + o -> w[o, n, 8 - tap]: d x[q, n] = sum_{tap, o} g[q + d(tap), o] w[o, n, 8 - tap]
__global__ void __launch_bounds__(256) k_cv_pack(const float* __restrict__ w, int cin, int cout, int bwd, float* __restrict__ out) {
    const int kc = bwd ? cout : cin, n_rows = bwd ? cv_npad(cin) : cout;
    const int kpad = cv_kpad(kc), groups = kpad / 8;
    const long long total = (long long)n_rows * kpad;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const long long fg = i >> 8;                                   // nt * groups + g
    const int g = (int)(fg % groups), nt = (int)(fg / groups);
    const int n = 32 * nt + (lane & 31), k = 8 * g + 4 * (lane >> 5) + j;
    float v = 0.f;
    if (k < 9 * kc) {
        const int tap = k / kc, c = k - tap * kc;
        if (!bwd)
            v = w[((long long)n * cin + c) * 9 + tap];
        else if (n < cin)
            v = w[((long long)c * cin + n) * 9 + (8 - tap)];
    }
    out[i] = v;
}

// the floats of one packing, and its launch into `out`
inline long long cv_pack_floats(int cin, int cout, int bwd) { return bwd ? (long long)cv_npad(cin) * cv_kpad(cout) : (long long)cout * cv_kpad(cin); }

inline hipError_t cv_pack(const float* w, int cin, int cout, int bwd, float* out, hipStream_t s) {
    k_cv_pack<<<(unsigned)((cv_pack_floats(cin, cout, bwd) + 255) / 256), 256, 0, s>>>(w, cin, cout, bwd, out);
    return hipGetLastError();
}

// ---- the first layer's patches -------------------------------------------------------------------------------------------------------
// load(f, yy, xx, c): channel c of pixel (yy, xx), inside the image, of image f
template <class Load>
__global__ void __launch_bounds__(256) k_cv_im2col(Load load, int n_img, int h, int w, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // (pixel m, quarter q): k = 4 q .. 4 q + 3
    const long long M = (long long)n_img * h * w;
    if (i >= M * 8) return;
    const long long m = i >> 3;
    const int q = (int)(i & 7);
    const int f = (int)(m / ((long long)h * w));
    const int rem = (int)(m - (long long)f * h * w), y = rem / w, x = rem - y * w;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        v[j] = 0.f;
        if (k < 27) {
            const int tap = k / 3, c = k - 3 * tap, yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) v[j] = load(f, yy, xx, c);
        }
    }
    *(float4*)(out + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

template <class Load>
int cv_im2col(const Load& load, long long n_img, int h, int w, float* out, hipStream_t s) {
    const long long quarters = n_img * h * w * 8;
    k_cv_im2col<<<(unsigned)((quarters + 255) / 256), 256, 0, s>>>(load, (int)n_img, h, w, out);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------
// the forward epilogue: + bias, ReLU -> out [M, cout]
struct CvFwd {
    const float* bias;
    float* out;
    int cout;
    __device__ void operator()(int m, int n, float v) const { out[(long long)m * cout + n] = fmaxf(v + bias[n], 0.f); }
};

// the j-th live tap of the mask
__device__ inline int cv_live_tap(int mask, int j) {
    int tap = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b)
        if ((mask >> b) & 1) {
            if (j == 0) tap = b;
            --j;
        }
    return tap;
}

// in [n_img, h, w, cin] (cin a multiple of 32; M = n_img h w rows).  single: the pixel itself against a one-tap packing (the first
// layer on its gathered patches); else 3 x 3 with zero padding 1 over the live taps of `tapmask`, n_chunks = live taps x cin / 32.
// grid (M tiles, N / 64, splits).  SPLIT, TAPS: whether the launch may split K and may leave taps out; a caller that never does
// either (LPIPS: measured 10 % slower with them) instantiates the loop without the K range and the tap list.
template <bool SPLIT, bool TAPS, class Epi>
__global__ void __launch_bounds__(CV_THREADS) k_cv_conv(const float* __restrict__ in, const float4* __restrict__ wpk, int M, int h, int w, int cin, int tapmask,
                                                        int single, int n_chunks, float* __restrict__ partial, Epi epi) {
    __shared__ __attribute__((aligned(16))) float sA[2][CV_A_FLOATS];
    __shared__ float4 sB[2][CV_B_FLOAT4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * CV_BM, by = blockIdx.y, bz = SPLIT ? blockIdx.z : 0, splits = SPLIT ? gridDim.z : 1;
    const int cchunks = cin / CV_KC, groups = (single ? 1 : 9) * cchunks * (CV_KC / 8);
    const int c_lo = SPLIT ? (int)((long long)bz * n_chunks / splits) : 0, c_hi = SPLIT ? (int)((long long)(bz + 1) * n_chunks / splits) : n_chunks;
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
    cv_f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    // step ch: fetch chunk ch + 1 into registers, run chunk ch from LDS buffer ch & 1, park the registers in the other buffer, barrier
    // (that buffer was last read in step ch - 1, which every wave has left).  Step c_lo - 1 only fetches and parks chunk c_lo.
    for (int ch = c_lo - 1; ch < c_hi; ++ch) {
        const int buf = ch & 1, nx = ch + 1;
        const bool more = nx < c_hi;
        float4 ra0, ra1, ra2, ra3, rb0, rb1;
        ra0 = ra1 = ra2 = ra3 = rb0 = rb1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (more) {
            const int lt = nx / cchunks, cc = nx - lt * cchunks, c0 = cc * CV_KC;
            const int tap = single ? 4 : TAPS ? cv_live_tap(tapmask, lt) : lt;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            const int wchunk = single ? nx : tap * cchunks + cc;
            // (py + dy, px + dx) inside the image: then pixel m + dy w + dx is that neighbour, in the same image
            const float* src = in + ((long long)m0 + (t >> 3) + dy * w + dx) * cin + c0 + 4 * q;
            const long long step = 32LL * cin;
            if (pv[0] && (unsigned)(py[0] + dy) < (unsigned)h && (unsigned)(px[0] + dx) < (unsigned)w) ra0 = *(const float4*)(src);
            if (pv[1] && (unsigned)(py[1] + dy) < (unsigned)h && (unsigned)(px[1] + dx) < (unsigned)w) ra1 = *(const float4*)(src + step);
            if (pv[2] && (unsigned)(py[2] + dy) < (unsigned)h && (unsigned)(px[2] + dx) < (unsigned)w) ra2 = *(const float4*)(src + 2 * step);
            if (pv[3] && (unsigned)(py[3] + dy) < (unsigned)h && (unsigned)(px[3] + dx) < (unsigned)w) ra3 = *(const float4*)(src + 3 * step);
            const float4* wsrc = wpk + ((long long)(2 * by) * groups + wchunk * (CV_KC / 8)) * 64 + t;
            rb0 = wsrc[0];
            rb1 = wsrc[(long long)groups * 64];
        }
        if (ch >= c_lo) {
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
    const int n = CV_BN * by + 32 * wn + (lane & 31), npad = CV_BN * gridDim.y;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 64 * wm + 32 * mt + tile_row(r, lane >> 5);
            if (m < M) {
                if (splits == 1)
                    epi(m, n, acc[mt][r]);
                else
                    partial[((long long)bz * M + m) * npad + n] = acc[mt][r];
            }
        }
}

// partial [splits, M, npad]: the sum over the splits in index order, then the epilogue
template <class Epi>
__global__ void __launch_bounds__(256) k_cv_reduce(const float* __restrict__ partial, int M, int npad, int splits, Epi epi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, n4 = npad / 4;
    if (i >= (long long)M * n4) return;
    const int m = (int)(i / n4), n = 4 * (int)(i - (long long)m * n4);
    const long long slab = (long long)M * npad;
    const float* p = partial + (long long)m * npad + n;
    float4 s = *(const float4*)p;
    for (int k = 1; k < splits; ++k) {
        const float4 v = *(const float4*)(p + k * slab);
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
    }
    epi(m, n, s.x);
    epi(m, n + 1, s.y);
    epi(m, n + 2, s.z);
    epi(m, n + 3, s.w);
}

// one convolution, either direction: in [M = n_img h w, kc] against the packing wpk of npad rows, over the live taps of `tapmask`
// (single: the one-tap packing), the n_chunks = live taps x kc / 32 chunks cut into `splits` ranges; splits > 1 needs
// partial [splits, M, npad]
template <bool SPLIT, bool TAPS, class Epi>
int cv_conv(const float* in, const float4* wpk, long long M, int h, int w, int kc, int npad, bool single, int tapmask, int n_chunks, int splits, float* partial,
            const Epi& epi, hipStream_t s) {
    HN_REQUIRE((SPLIT || splits == 1) && (TAPS || tapmask == CV_ALL_TAPS), "cv_conv: %d splits and tap mask 0x%x in a launch compiled without them", splits, tapmask);
    k_cv_conv<SPLIT, TAPS><<<dim3((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)(npad / CV_BN), (unsigned)splits), CV_THREADS, 0, s>>>(in, wpk, (int)M, h, w, kc, tapmask,
                                                                                                                           single ? 1 : 0, n_chunks, partial, epi);
    HN_LAUNCH_CHECK();
    if constexpr (SPLIT)
        if (splits > 1) {
            const long long total = M * (npad / 4);
            k_cv_reduce<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(partial, (int)M, npad, splits, epi);
            HN_LAUNCH_CHECK();
        }
    return HN_OK;
}

// ---- the pool ----------------------------------------------------------------------------------------------------------------------
__device__ inline float4 max4(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }

__global__ void __launch_bounds__(256) k_cv_pool(const float* __restrict__ in, int n_img, int h, int w, int c, float* __restrict__ out) {
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

int cv_pool(const float* in, float* out, long long n_img, int h, int w, int c, hipStream_t s) {
    const long long total = n_img * (h / 2) * (w / 2) * (c / 4);
    k_cv_pool<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(in, (int)n_img, h, w, c, out);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // namespace
}  // namespace hn
