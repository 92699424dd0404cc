// Image metrics on the device: the PSNR and SSIM of analys_results/analys_psnr_ssim_lpips.py:23-26 (skimage's peak_signal_noise_ratio
// and structural_similarity(channel_axis=2, data_range=255)) for F pairs of 8-bit interleaved RGB images [F, H, W, 3] of one size.
// tests/test_image_metrics_cpu.py restates both in float64 numpy; DESIGN.md 3.16 is the contract.
//
// Two calls, all on device pointers, outputs and workspace supplied by the caller, no synchronisation, no allocation, no
// floating-point atomics (every reduction combines its partials in a fixed order: a repeated call gives the same bits):
//   sse    per image the exact sum over its H W 3 bytes of (a - b)^2 as an unsigned 64-bit integer (PSNR is 10 log10(255^2 N / sse),
//          formed by the caller in fp64).
//   ssim   per channel the mean over the (H - 6) x (W - 6) windows that lie inside the image of
//              S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
//          a 7 x 7 uniform window, sample covariance (49 / 48), C1 = (0.01 255)^2, C2 = (0.03 255)^2.  The five window sums (x, y,
//          xx, yy, xy) are INTEGERS (49 255^2 < 2^24), the moments come from them in fp64 (vx = (49 sxx - sx^2) / (49 48), the
//          numerator still an exact int32), so the only rounding is in S itself and in the mean.  Optionally the S map in fp32.
//
// Passes:
//   k_im_sse         a workgroup owns IM_CHUNK consecutive bytes of one image: 16 bytes per lane and step (memcpy from the byte
//                    address: image starts are not aligned when H W 3 is no multiple of 16), a uint32 sum per lane (at most 128 terms
//                    of 255^2), a uint64 sum per workgroup -> one partial
//   k_im_ssim        a workgroup owns IM_TH x IM_TW output pixels of one image.  The tile's IM_TH + 6 input rows of (IM_TW + 6) x 3
//                    contiguous bytes are staged in LDS as they lie in memory (4 bytes per load from the byte address: rows start
//                    anywhere when 3 W is no multiple of 4).  A lane owns one interleaved column j = 3 x + c, so that the channels need
//                    no special case: the horizontal 7-sum of row r at j is the sum of bytes j, j + 3, .., j + 18.  The lane walks down
//                    the rows, keeps the last seven horizontal sums in registers and the vertical sum of them as a running value (add
//                    the new row, take off the one that leaves), evaluates S, adds it in fp64.  Lanes of one channel are then summed
//                    in lane order -> one partial per tile and channel
//   k_im_sse_final / k_im_ssim_final   one wave per image (and channel): a strided sum of the partials per lane, a butterfly over the
//                    lanes (the same tree on every run), the mean for SSIM
#include "hn_common.h"

namespace hn {
namespace {

constexpr int IM_SSE_THREADS = 256;
constexpr int IM_SSE_STEPS = 8;                                   // 16-byte steps per lane: 128 terms <= 128 * 65025 < 2^32
constexpr long long IM_CHUNK = (long long)IM_SSE_THREADS * 16 * IM_SSE_STEPS;    // bytes of one image per workgroup
constexpr int IM_TW = 64, IM_TH = 32;                             // output pixels per tile
constexpr int IM_COLS = 3 * IM_TW;                                // interleaved output columns = lanes per workgroup (3 waves)
constexpr int IM_ROWS = IM_TH + 6;                                // staged input rows
constexpr int IM_ROW_BYTES = 3 * (IM_TW + 6);                     // staged bytes per row (210)
constexpr int IM_PITCH = 216;                                     // LDS row pitch in bytes (a multiple of 4, >= IM_ROW_BYTES)
constexpr long long IM_MAX = 1LL << 31;                           // F H W 3 stays below this
static_assert(IM_PITCH % 4 == 0 && IM_PITCH >= IM_ROW_BYTES && IM_COLS % 64 == 0, "LDS rows hold a staged row; whole waves");

struct ImShape {
    long long n_bytes;              // per image
    long long chunks;               // k_im_sse workgroups per image
    long long tiles_x, tiles_y;     // k_im_ssim workgroups per image
};

int im_shape(const char* who, long long n_images, long long height, long long width, ImShape& s, size_t& bytes) {
    HN_REQUIRE(n_images >= 1 && height >= 7 && width >= 7, "%s: n_images = %lld, height = %lld, width = %lld: at least one image of 7 x 7", who,
               n_images, height, width);
    HN_REQUIRE(height < IM_MAX && width < IM_MAX && n_images < IM_MAX && height * width < IM_MAX && n_images * height * width * 3 < IM_MAX,
               "%s: n_images = %lld, height = %lld, width = %lld: n_images x height x width x 3 must stay below 2^31", who, n_images, height, width);
    s.n_bytes = height * width * 3;
    s.chunks = (s.n_bytes + IM_CHUNK - 1) / IM_CHUNK;
    s.tiles_x = (width - 6 + IM_TW - 1) / IM_TW;
    s.tiles_y = (height - 6 + IM_TH - 1) / IM_TH;
    const size_t sse = sizeof(unsigned long long) * (size_t)(n_images * s.chunks);
    const size_t ssim = sizeof(double) * 3 * (size_t)(n_images * s.tiles_x * s.tiles_y);
    bytes = ((sse > ssim ? sse : ssim) + 255) & ~(size_t)255;
    return HN_OK;
}

// ---- squared error -----------------------------------------------------------------------------------------------------------------
__device__ inline unsigned sq_diff4(unsigned a, unsigned b) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
        s += (unsigned)(d * d);
    }
    return s;
}

__global__ void __launch_bounds__(IM_SSE_THREADS) k_im_sse(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                           long long n_bytes, int chunks, unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long red[IM_SSE_THREADS / 64];
    const long long f = blockIdx.x / chunks, c = blockIdx.x - f * chunks;
    const long long lo = c * IM_CHUNK, hi = lo + IM_CHUNK < n_bytes ? lo + IM_CHUNK : n_bytes;      // within the image
    const unsigned char* pa = a + f * n_bytes;
    const unsigned char* pb = b + f * n_bytes;
    unsigned acc = 0;
#pragma unroll
    for (int it = 0; it < IM_SSE_STEPS; ++it) {
        const long long i = lo + ((long long)it * IM_SSE_THREADS + threadIdx.x) * 16;
        if (i + 16 <= hi) {
            unsigned va[4], vb[4];
            __builtin_memcpy(va, pa + i, 16);
            __builtin_memcpy(vb, pb + i, 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += sq_diff4(va[k], vb[k]);
        } else {
            for (long long j = i; j < hi; ++j) {                  // the image's last, short step
                const int d = (int)pa[j] - (int)pb[j];
                acc += (unsigned)(d * d);
            }
        }
    }
    unsigned long long v = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < IM_SSE_THREADS / 64; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(64) k_im_sse_final(const unsigned long long* __restrict__ partial, int chunks,
                                                     unsigned long long* __restrict__ sse) {
    const unsigned long long* p = partial + (long long)blockIdx.x * chunks;
    unsigned long long v = 0;
    for (int k = threadIdx.x; k < chunks; k += 64) v += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x == 0) sse[blockIdx.x] = v;
}

// ---- SSIM --------------------------------------------------------------------------------------------------------------------------
// one tile row of one image into LDS: `n` bytes from the byte address src, four at a time and the last n % 4 one by one
__device__ inline void stage_row(unsigned char* dst, const unsigned char* __restrict__ src, int n, int lane, int lanes) {
    const int nw = n >> 2;
    for (int w = lane; w < nw; w += lanes) {
        unsigned v;
        __builtin_memcpy(&v, src + 4 * w, 4);
        *(unsigned*)(dst + 4 * w) = v;
    }
    for (int k = 4 * nw + lane; k < n; k += lanes) dst[k] = src[k];
}

__device__ inline double ssim_of(int sx, int sy, int sxx, int syy, int sxy) {
    constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double ux = (double)sx / 49.0, uy = (double)sy / 49.0;
    const double vx = (double)(49 * sxx - sx * sx) / 2352.0;        // 49 * 48; the numerators are exact: 49^2 255^2 < 2^31
    const double vy = (double)(49 * syy - sy * sy) / 2352.0;
    const double vxy = (double)(49 * sxy - sx * sy) / 2352.0;
    const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * vxy + C2;
    const double b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
    return (a1 * a2) / (b1 * b2);
}

__global__ void __launch_bounds__(IM_COLS) k_im_ssim(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int height,
                                                     int width, int tiles_x, int tiles_y, double* __restrict__ partial,
                                                     float* __restrict__ s_map) {
    __shared__ __attribute__((aligned(16))) unsigned char sa[IM_ROWS * IM_PITCH], sb[IM_ROWS * IM_PITCH];
    __shared__ double red[IM_COLS];
    const int tiles = tiles_x * tiles_y;
    const long long f = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - f * tiles), ty = t / tiles_x, tx = t - ty * tiles_x;
    const int x0 = tx * IM_TW, y0 = ty * IM_TH;                    // the tile's first output pixel = its first input pixel
    const int out_w = width - 6, out_h = height - 6;
    const int in_cols = (width - x0 < IM_TW + 6 ? width - x0 : IM_TW + 6), in_rows = (height - y0 < IM_ROWS ? height - y0 : IM_ROWS);
    const int row_bytes = 3 * in_cols;                             // <= IM_ROW_BYTES
    const long long img = f * (long long)height * width * 3;
    // waves take rows in turn; a row is one contiguous run of bytes
    for (int r = threadIdx.x >> 6; r < in_rows; r += IM_COLS / 64) {
        const long long off = img + ((long long)(y0 + r) * width + x0) * 3;
        stage_row(sa + r * IM_PITCH, a + off, row_bytes, threadIdx.x & 63, 64);
        stage_row(sb + r * IM_PITCH, b + off, row_bytes, threadIdx.x & 63, 64);
    }
    __syncthreads();
    const int j = threadIdx.x;                                     // interleaved column: pixel x0 + j / 3, channel j % 3
    const bool live = x0 + j / 3 < out_w;                          // then bytes j .. j + 18 of every staged row were loaded
    int ring[7][5];
    int v[5] = {0, 0, 0, 0, 0};
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < IM_ROWS; ++r) {
        if (r < in_rows) {                                         // uniform over the workgroup
            int h[5] = {0, 0, 0, 0, 0};
            if (live) {
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const int x = sa[r * IM_PITCH + j + 3 * k], y = sb[r * IM_PITCH + j + 3 * k];
                    h[0] += x;
                    h[1] += y;
                    h[2] += x * x;
                    h[3] += y * y;
                    h[4] += x * y;
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                v[q] += h[q];
                if (r >= 7) v[q] -= ring[r % 7][q];
                ring[r % 7][q] = h[q];
            }
            if (r >= 6 && live) {
                const int oy = y0 + r - 6;                         // < out_h, since r < in_rows
                const double s = ssim_of(v[0], v[1], v[2], v[3], v[4]);
                acc += s;
                if (s_map) s_map[((f * out_h + oy) * (long long)out_w + x0) * 3 + j] = (float)s;
            }
        }
    }
    red[j] = acc;
    __syncthreads();
    if (j < 3) {                                                   // channel j: the lanes j, j + 3, .. in order (idle lanes hold 0)
        double s = 0.0;
        for (int k = j; k < IM_COLS; k += 3) s += red[k];
        partial[(long long)blockIdx.x * 3 + j] = s;
    }
}

__global__ void __launch_bounds__(64) k_im_ssim_final(const double* __restrict__ partial, int tiles, double count, double* __restrict__ ssim_ch) {
    const long long f = blockIdx.x / 3;
    const int c = (int)(blockIdx.x - 3 * f);
    const double* p = partial + f * tiles * 3 + c;
    double v = 0.0;
    for (int k = threadIdx.x; k < tiles; k += 64) v += p[3LL * k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x == 0) ssim_ch[blockIdx.x] = v / count;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_im_workspace_bytes(long long n_images, long long height, long long width) {
    ImShape sh;
    size_t bytes = 0;
    return im_shape("hn_im_workspace_bytes", n_images, height, width, sh, bytes) == HN_OK ? bytes : 0;
}

int hn_im_sse(const unsigned char* a, const unsigned char* b, long long n_images, long long height, long long width, unsigned long long* sse,
              void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    ImShape sh;
    size_t need = 0;
    HN_TRY_RC(im_shape("hn_im_sse", n_images, height, width, sh, need));
    HN_REQUIRE(a && b && sse && workspace, "hn_im_sse: NULL a / b / sse / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_im_sse: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sse & 7) == 0, "hn_im_sse: workspace / sse not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* partial = (unsigned long long*)workspace;
    k_im_sse<<<(unsigned)(n_images * sh.chunks), IM_SSE_THREADS, 0, s>>>(a, b, sh.n_bytes, (int)sh.chunks, partial);
    HN_LAUNCH_CHECK();
    k_im_sse_final<<<(unsigned)n_images, 64, 0, s>>>(partial, (int)sh.chunks, sse);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_im_ssim(const unsigned char* a, const unsigned char* b, long long n_images, long long height, long long width, double* ssim_ch,
               float* s_map, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    ImShape sh;
    size_t need = 0;
    HN_TRY_RC(im_shape("hn_im_ssim", n_images, height, width, sh, need));
    HN_REQUIRE(a && b && ssim_ch && workspace, "hn_im_ssim: NULL a / b / ssim_ch / workspace");
    HN_REQUIRE(workspace_bytes >= need, "hn_im_ssim: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)ssim_ch & 7) == 0 && ((uintptr_t)s_map & 3) == 0,
               "hn_im_ssim: workspace / ssim_ch not 8-byte aligned, or s_map not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const long long tiles = sh.tiles_x * sh.tiles_y;
    k_im_ssim<<<(unsigned)(n_images * tiles), IM_COLS, 0, s>>>(a, b, (int)height, (int)width, (int)sh.tiles_x, (int)sh.tiles_y, partial, s_map);
    HN_LAUNCH_CHECK();
    k_im_ssim_final<<<(unsigned)(3 * n_images), 64, 0, s>>>(partial, (int)tiles, (double)(height - 6) * (double)(width - 6), ssim_ch);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
