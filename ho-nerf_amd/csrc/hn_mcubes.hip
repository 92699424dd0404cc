// Marching cubes on the device: a float32 scalar volume [nx, ny, nz] (x slowest, the 'ij' grid of extract_geometry) -> an indexed
// triangle mesh, both on the device.  Replaces the PyMCubes call of extract_geometry (utils/renderer.py:279-284, 561-564).
//
// Conventions (tests/test_mesh_cpu.py restates them in numpy):
//   - a grid point is INSIDE when value < threshold (the bit of its corner is set in the cube index);
//   - grid point p = (i, j, k) owns its +x, +y and +z edges; every owned edge whose two ends differ in the inside test carries exactly
//     one vertex, shared by every cell that uses the edge, placed at p + t e_axis with t = (thr - v(p)) / (v(p + e_axis) - v(p));
//   - vertex ids: by the owning point's linear index, then axis x, y, z; triangle ids: by the cell's linear index (that of its
//     (0,0,0) corner), then by the triangle's place in the table.  Offsets come from integer scans, so the output is the same bits
//     on every run;
//   - the table is the classic 256-case one (Lorensen / Bourke corner and edge numbering, below), whose triangles face the inside
//     corners; each triangle is emitted in reverse order, so its normal (v1 - v0) x (v2 - v0) points toward increasing value
//     (outward for an SDF): the orientation the reference obtains by flipping PyMCubes' output (triangles[..., ::-1]).
//
// Passes (every launch maps 4 consecutive points to a thread, 1024 points to a 256-thread workgroup):
//   k_mc_count   per point: crossing owned edges (0-3) and, as a cell's origin, its triangle count; one sum of each per workgroup
//   k_mc_scan    one workgroup: exclusive scans of the workgroup sums -> vertex / triangle offsets and the totals V, T
//   k_mc_verts   per point: vertex base (int32) and a flag byte (crossing owned edges, inside bit) into the workspace, and the
//                positions of its vertices
//   k_mc_tris    per cell: the case from the flag bytes of its 8 corners (the volume is not read again), the vertex ids of its
//                edges from the owners' bases and flags, the triangles
#include "hn_mc_tables.h"   // the case table and the integer scans, shared with hn_mcubes_sparse.hip

namespace hn {
namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_PPT = 4;                        // points per thread
constexpr int MC_PPB = MC_THREADS * MC_PPT;      // points per workgroup
constexpr int MC_SCAN_THREADS = 1024;

// Where the 4 points of a thread sit: (i, j, k) of each, and whether each is inside the volume.
struct Quad {
    int i[MC_PPT], j[MC_PPT], k[MC_PPT];
    bool valid[MC_PPT];
};

__device__ __forceinline__ Quad quad_of(long long p0, long long n, int ny, int nz) {
    Quad q;
    const long long nyz = (long long)ny * nz;
    int i = (int)(p0 / nyz);
    const long long r = p0 - (long long)i * nyz;
    int j = (int)(r / nz);
    int k = (int)(r - (long long)j * nz);
#pragma unroll
    for (int m = 0; m < MC_PPT; ++m) {
        q.i[m] = i;
        q.j[m] = j;
        q.k[m] = k;
        q.valid[m] = p0 + m < n;
        if (++k == nz) {
            k = 0;
            if (++j == ny) {
                j = 0;
                ++i;
            }
        }
    }
    return q;
}

// The 5 consecutive elements a[q .. q + 4] (0 past the end of the array).  VEC: q and n are multiples of 4, so the first four
// come in one 16-byte load (T = float) or one 4-byte load (T = unsigned char).
template <typename T, bool VEC>
__device__ __forceinline__ void load5(const T* __restrict__ a, long long q, long long n, T out[5]) {
    if (VEC) {
        if (q + 4 <= n) {
            using V4 = typename std::conditional<sizeof(T) == 4, float4, uchar4>::type;
            const V4 v = *reinterpret_cast<const V4*>(a + q);
            out[0] = v.x;
            out[1] = v.y;
            out[2] = v.z;
            out[3] = v.w;
        } else {
            out[0] = out[1] = out[2] = out[3] = T(0);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) out[m] = q + m < n ? a[q + m] : T(0);
    }
    out[4] = q + 4 < n ? a[q + 4] : T(0);
}

// The 8 corners of the cells whose origins are the thread's 4 points, as 4 rows of 5: row 0 the points themselves (+z along the
// row), row 1 at +y, row 2 at +x, row 3 at +x+y.
template <typename T, bool VEC>
__device__ __forceinline__ void load_rows(const T* __restrict__ a, long long p0, long long n, int ny, int nz, T rows[4][5]) {
    const long long nyz = (long long)ny * nz;
    load5<T, VEC>(a, p0, n, rows[0]);
    load5<T, VEC>(a, p0 + nz, n, rows[1]);
    load5<T, VEC>(a, p0 + nyz, n, rows[2]);
    load5<T, VEC>(a, p0 + nyz + nz, n, rows[3]);
}

// Cube index of the cell at point m from its corners' inside bits (Bourke's corner order).
template <typename F>
__device__ __forceinline__ int cube_case(F in, const int m) {
    return in(0, m) | in(2, m) << 1 | in(3, m) << 2 | in(1, m) << 3 | in(0, m + 1) << 4 | in(2, m + 1) << 5 | in(3, m + 1) << 6 |
           in(1, m + 1) << 7;
}

struct PointCounts {
    int edges[MC_PPT];   // crossing owned edges: bit 0 x, bit 1 y, bit 2 z
    int tris[MC_PPT];    // triangles of the cell at the point (0 where the point is no cell origin)
};

__device__ __forceinline__ PointCounts point_counts(const float rows[4][5], const Quad& q, int nx, int ny, int nz, float thr) {
    PointCounts c;
    auto in = [&](int r, int m) { return rows[r][m] < thr ? 1 : 0; };
#pragma unroll
    for (int m = 0; m < MC_PPT; ++m) {
        const bool hx = q.i[m] + 1 < nx, hy = q.j[m] + 1 < ny, hz = q.k[m] + 1 < nz;
        const int i0 = in(0, m);
        int e = 0;
        if (q.valid[m]) {
            e = (hx && i0 != in(2, m) ? 1 : 0) | (hy && i0 != in(1, m) ? 2 : 0) | (hz && i0 != in(0, m + 1) ? 4 : 0);
        }
        c.edges[m] = e;
        c.tris[m] = (q.valid[m] && hx && hy && hz) ? (int)c_tri_count[cube_case(in, m)] : 0;
    }
    return c;
}

// ---- pass 1: counts per workgroup ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mc_count(const float* __restrict__ vol, int nx, int ny, int nz, float thr,
                                                         int* __restrict__ blk_v, int* __restrict__ blk_t) {
    const long long n = (long long)nx * ny * nz;
    const long long p0 = ((long long)blockIdx.x * MC_THREADS + threadIdx.x) * MC_PPT;
    int nv = 0, nt = 0;
    if (p0 < n) {
        float rows[4][5];
        load_rows<float, VEC>(vol, p0, n, ny, nz, rows);
        const Quad q = quad_of(p0, n, ny, nz);
        const PointCounts c = point_counts(rows, q, nx, ny, nz, thr);
#pragma unroll
        for (int m = 0; m < MC_PPT; ++m) {
            nv += __popc(c.edges[m]);
            nt += c.tris[m];
        }
    }
    __shared__ int red[2][MC_THREADS / 64];
    nv = wave_sum(nv);
    nt = wave_sum(nt);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w] = nv;
        red[1][w] = nt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sv = 0, st = 0;
#pragma unroll
        for (int u = 0; u < MC_THREADS / 64; ++u) {
            sv += red[0][u];
            st += red[1][u];
        }
        blk_v[blockIdx.x] = sv;
        blk_t[blockIdx.x] = st;
    }
}

// ---- pass 2: exclusive scans of the workgroup sums (one workgroup) ---------------------------------------------------------------
// Tiles of MC_SCAN_THREADS x 4 sums: each thread adds its 4 in order, the workgroup scans the thread sums (int: a tile holds at most
// 4096 x 5120 triangles), the running carry is 64-bit.  totals = {V, T}.
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_mc_scan(const int* __restrict__ blk_v, const int* __restrict__ blk_t, int nb,
                                                             long long* __restrict__ off_v, long long* __restrict__ off_t,
                                                             long long* __restrict__ totals) {
    __shared__ int lds[MC_SCAN_THREADS / 64];
    long long carry_v = 0, carry_t = 0;
    for (int base = 0; base < nb; base += MC_SCAN_THREADS * 4) {
        const int b0 = base + threadIdx.x * 4;
        int v[4], t[4], sv = 0, st = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = b0 + u < nb ? blk_v[b0 + u] : 0;
            t[u] = b0 + u < nb ? blk_t[b0 + u] : 0;
            sv += v[u];
            st += t[u];
        }
        int tot_v, tot_t;
        long long ev = carry_v + block_excl_scan<MC_SCAN_THREADS>(sv, lds, tot_v);
        long long et = carry_t + block_excl_scan<MC_SCAN_THREADS>(st, lds, tot_t);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b0 + u < nb) {
                off_v[b0 + u] = ev;
                off_t[b0 + u] = et;
            }
            ev += v[u];
            et += t[u];
        }
        carry_v += tot_v;
        carry_t += tot_t;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry_v;
        totals[1] = carry_t;
    }
}

// ---- pass 3: vertex bases, flag bytes and vertex positions -----------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mc_verts(const float* __restrict__ vol, int nx, int ny, int nz, float thr,
                                                         const long long* __restrict__ off_v, int* __restrict__ vbase,
                                                         unsigned char* __restrict__ flags, float* __restrict__ verts, long long n_verts) {
    __shared__ int lds[MC_THREADS / 64];
    const long long n = (long long)nx * ny * nz;
    const long long p0 = ((long long)blockIdx.x * MC_THREADS + threadIdx.x) * MC_PPT;
    float rows[4][5];
    Quad q;
    PointCounts c = {};
    int nv = 0;
    if (p0 < n) {
        load_rows<float, VEC>(vol, p0, n, ny, nz, rows);
        q = quad_of(p0, n, ny, nz);
        c = point_counts(rows, q, nx, ny, nz, thr);
#pragma unroll
        for (int m = 0; m < MC_PPT; ++m) nv += __popc(c.edges[m]);
    }
    int total;
    const int excl = block_excl_scan<MC_THREADS>(nv, lds, total);
    if (p0 >= n) return;
    long long vid = off_v[blockIdx.x] + excl;
    int base[MC_PPT];
    unsigned char fl[MC_PPT];
#pragma unroll
    for (int m = 0; m < MC_PPT; ++m) {
        base[m] = (int)vid;
        fl[m] = (unsigned char)(c.edges[m] | (rows[0][m] < thr ? 8 : 0));
        const float v0 = rows[0][m];
        // the other end of the x, y, z edge: rows 2, 1 at m; row 0 at m + 1
        const float v1[3] = {rows[2][m], rows[1][m], rows[0][m + 1]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (c.edges[m] >> a & 1) {
                if (vid < n_verts) {
                    const float t = (thr - v0) / (v1[a] - v0);
                    float* o = verts + 3 * vid;
                    o[0] = (float)q.i[m] + (a == 0 ? t : 0.f);
                    o[1] = (float)q.j[m] + (a == 1 ? t : 0.f);
                    o[2] = (float)q.k[m] + (a == 2 ? t : 0.f);
                }
                ++vid;
            }
        }
    }
    if (p0 + MC_PPT <= n) {
        *reinterpret_cast<int4*>(vbase + p0) = make_int4(base[0], base[1], base[2], base[3]);
        *reinterpret_cast<uchar4*>(flags + p0) = make_uchar4(fl[0], fl[1], fl[2], fl[3]);
    } else {
#pragma unroll
        for (int m = 0; m < MC_PPT; ++m) {
            if (q.valid[m]) {
                vbase[p0 + m] = base[m];
                flags[p0 + m] = fl[m];
            }
        }
    }
}

// ---- pass 4: triangles -----------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mc_tris(const unsigned char* __restrict__ flags, const int* __restrict__ vbase, int nx,
                                                        int ny, int nz, const long long* __restrict__ off_t, long long* __restrict__ tris,
                                                        long long n_tris) {
    __shared__ int lds[MC_THREADS / 64];
    const long long n = (long long)nx * ny * nz;
    const long long nyz = (long long)ny * nz;
    const long long p0 = ((long long)blockIdx.x * MC_THREADS + threadIdx.x) * MC_PPT;
    unsigned char rows[4][5];
    Quad q;
    int cases[MC_PPT] = {0, 0, 0, 0};
    int nt = 0;
    if (p0 < n) {
        load_rows<unsigned char, VEC>(flags, p0, n, ny, nz, rows);
        q = quad_of(p0, n, ny, nz);
        auto in = [&](int r, int m) { return (int)(rows[r][m] >> 3) & 1; };
#pragma unroll
        for (int m = 0; m < MC_PPT; ++m) {
            if (q.valid[m] && q.i[m] + 1 < nx && q.j[m] + 1 < ny && q.k[m] + 1 < nz) {
                cases[m] = cube_case(in, m);
                nt += c_tri_count[cases[m]];
            }
        }
    }
    int total;
    const int excl = block_excl_scan<MC_THREADS>(nt, lds, total);
    if (p0 >= n || nt == 0) return;
    long long tid = off_t[blockIdx.x] + excl;
#pragma unroll
    for (int m = 0; m < MC_PPT; ++m) {
        const int cs = cases[m];
        const int cnt = c_tri_count[cs];
        const long long p = p0 + m;
        for (int s = 0; s < cnt; ++s, ++tid) {
            long long id[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int e = c_tri_table[cs][3 * s + u];
                const long long o = p + c_edge_owner[e][0] * nyz + c_edge_owner[e][1] * nz + c_edge_owner[e][2];
                const int axis = c_edge_owner[e][3];
                id[u] = (long long)vbase[o] + __popc(flags[o] & ((1 << axis) - 1));
            }
            if (tid < n_tris) {
                long long* out = tris + 3 * tid;
                out[0] = id[2];   // reversed: the normal points toward increasing value
                out[1] = id[1];
                out[2] = id[0];
            }
        }
    }
}

struct McLayout {
    long long n = 0, nb = 0;
    size_t blk_v = 0, blk_t = 0, off_v = 0, off_t = 0, vbase = 0, flags = 0, bytes = 0;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int mc_layout(int nx, int ny, int nz, McLayout& L) {
    HN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "hn_mcubes: every dim must be >= 2 (got %d x %d x %d)", nx, ny, nz);
    L.n = (long long)nx * ny * nz;
    HN_REQUIRE(3 * L.n < (1LL << 31), "hn_mcubes: %d x %d x %d has %lld edge ids, which overflow int32 (3 nx ny nz must be < 2^31)", nx, ny,
               nz, 3 * L.n);
    L.nb = (L.n + MC_PPB - 1) / MC_PPB;
    size_t at = 0;
    L.blk_v = at, at = align256(at + sizeof(int) * L.nb);
    L.blk_t = at, at = align256(at + sizeof(int) * L.nb);
    L.off_v = at, at = align256(at + sizeof(long long) * L.nb);
    L.off_t = at, at = align256(at + sizeof(long long) * L.nb);
    L.vbase = at, at = align256(at + sizeof(int) * L.n);
    L.flags = at, at = align256(at + L.n);
    L.bytes = at;
    return HN_OK;
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_mcubes_workspace_bytes(int nx, int ny, int nz) {
    McLayout L;
    return mc_layout(nx, ny, nz, L) == HN_OK ? L.bytes : 0;
}

int hn_mcubes_count(const float* volume, int nx, int ny, int nz, float threshold, long long* totals, void* workspace,
                    size_t workspace_bytes, hn_stream_t stream) {
    McLayout L;
    HN_TRY_RC(mc_layout(nx, ny, nz, L));
    HN_REQUIRE(volume && totals && workspace, "hn_mcubes_count: NULL volume / totals / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_mcubes_count: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)volume & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "hn_mcubes_count: volume / workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int* blk_v = (int*)(ws + L.blk_v);
    int* blk_t = (int*)(ws + L.blk_t);
    if (nz % 4 == 0)
        k_mc_count<true><<<(unsigned)L.nb, MC_THREADS, 0, s>>>(volume, nx, ny, nz, threshold, blk_v, blk_t);
    else
        k_mc_count<false><<<(unsigned)L.nb, MC_THREADS, 0, s>>>(volume, nx, ny, nz, threshold, blk_v, blk_t);
    HN_LAUNCH_CHECK();
    k_mc_scan<<<1, MC_SCAN_THREADS, 0, s>>>(blk_v, blk_t, (int)L.nb, (long long*)(ws + L.off_v), (long long*)(ws + L.off_t), totals);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcubes_emit(const float* volume, int nx, int ny, int nz, float threshold, void* workspace, size_t workspace_bytes, long long n_verts,
                   long long n_tris, float* vertices, long long* triangles, hn_stream_t stream) {
    McLayout L;
    HN_TRY_RC(mc_layout(nx, ny, nz, L));
    HN_REQUIRE(volume && workspace, "hn_mcubes_emit: NULL volume / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_mcubes_emit: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(n_verts >= 0 && n_tris >= 0 && n_verts <= 3 * L.n && n_tris <= 5 * L.n, "hn_mcubes_emit: bad sizes V = %lld, T = %lld",
               n_verts, n_tris);
    if (n_verts == 0 || n_tris == 0) return HN_OK;   // no crossing: nothing to launch
    HN_REQUIRE(vertices && triangles, "hn_mcubes_emit: NULL vertices / triangles");
    HN_REQUIRE(((uintptr_t)volume & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "hn_mcubes_emit: volume / workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int* vbase = (int*)(ws + L.vbase);
    unsigned char* flags = (unsigned char*)(ws + L.flags);
    if (nz % 4 == 0) {
        k_mc_verts<true><<<(unsigned)L.nb, MC_THREADS, 0, s>>>(volume, nx, ny, nz, threshold, (const long long*)(ws + L.off_v), vbase, flags,
                                                              vertices, n_verts);
        HN_LAUNCH_CHECK();
        k_mc_tris<true><<<(unsigned)L.nb, MC_THREADS, 0, s>>>(flags, vbase, nx, ny, nz, (const long long*)(ws + L.off_t), triangles, n_tris);
    } else {
        k_mc_verts<false><<<(unsigned)L.nb, MC_THREADS, 0, s>>>(volume, nx, ny, nz, threshold, (const long long*)(ws + L.off_v), vbase, flags,
                                                               vertices, n_verts);
        HN_LAUNCH_CHECK();
        k_mc_tris<false><<<(unsigned)L.nb, MC_THREADS, 0, s>>>(flags, vbase, nx, ny, nz, (const long long*)(ws + L.off_t), triangles, n_tris);
    }
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
