// Narrow-band marching cubes: the mesh of hn_mcubes.hip, bit for bit, from field values in a band of blocks around the level set
// only.  The caller owns the field: these kernels say WHERE values are needed (grid indices), take the values back, and mesh them.
//
// Grid and blocks.  dims (nx, ny, nz), every dim in [2, 2048]; block edge b = 4 or 8 cells.  Along an axis of n points there are
// nb = ceil((n - 1) / b) blocks; block i covers the cells between points i b and min((i + 1) b, n - 1) (its extent, ext <= b cells:
// the last block may be shorter).  Block ids are linear with x slowest, as everything else here.
// Lattice: the (nbx + 1)(nby + 1)(nbz + 1) block corners, point min(i b, n - 1) per axis.
// Brick: the (b + 1)^3 values of an active block, local index (lx (b + 1) + ly)(b + 1) + lz: its own points and the apron on its +x,
// +y, +z faces.  Local indices above the extent lie beyond the grid: invalid, never read (hn_mcs_brick_points repeats a valid index
// there so that the caller's field launch stays in bounds).
// Ownership.  Grid point g belongs to block min(g / b, nb - 1) per axis: local index < b, and the grid's last layer to the last block
// (where no block begins).  The owner of a point owns its +x, +y, +z edges and their vertices, as in the dense mesher; a cell belongs
// to the block that covers it.  A cell whose edge is owned by a neighbouring brick finds the vertex through the block -> slot table.
//
// Passes:
//   hn_mcs_lattice       lattice indices
//   hn_mcs_classify      mask: corners disagree on value < threshold (the dense mesher's inside test), or a corner within `reach`
//   hn_mcs_compact       k_mcs_mask_count -> k_mcs_scan -> k_mcs_mask_emit: ascending active list, block -> slot table, total
//   hn_mcs_brick_points  grid indices of bricks
//   hn_mcs_leaks         k_mcs_leak_mark: a crossing edge on a block's boundary marks the inactive blocks that share it;
//                        k_mcs_leak_count: blocks marked and not yet in the table (an integer atomic per workgroup)
//   hn_mcs_count         k_mcs_brick_count (one workgroup per brick, the brick in LDS) -> k_mcs_scan
//   hn_mcs_emit          k_mcs_verts (positions, keys, per-point vertex base and edge flags) -> k_mcs_tris
// Every offset comes from an integer scan and no float is ever accumulated: two runs give the same bits.  The vertex position is
// hn_mcubes.hip's expression on the same operands (this file is compiled without FMA contraction, as that one is).
#include "hn_mc_tables.h"

namespace hn {
namespace {

constexpr int MCS_THREADS = 256;
constexpr int MCS_PPT = 4;                          // blocks per thread of the mask passes
constexpr int MCS_PPB = MCS_THREADS * MCS_PPT;
constexpr int MCS_SCAN_THREADS = 1024;
constexpr int MCS_MAX_DIM = 2048;

struct McsGrid {
    int n[3];      // points per axis
    int nb[3];     // blocks per axis
    int b;         // cells per block edge
};

__host__ __device__ inline long long mcs_blocks(const McsGrid& g) { return (long long)g.nb[0] * g.nb[1] * g.nb[2]; }
__host__ __device__ inline long long mcs_lattice(const McsGrid& g) { return (long long)(g.nb[0] + 1) * (g.nb[1] + 1) * (g.nb[2] + 1); }

struct McsBlock {
    int c[3];      // block coordinates
    int o[3];      // grid index of the block's first point
    int ext[3];    // cells of the block per axis (valid local indices are 0 .. ext)
};

__device__ __forceinline__ McsBlock mcs_block(const McsGrid& g, int blk) {
    McsBlock B;
    B.c[2] = blk % g.nb[2];
    const int r = blk / g.nb[2];
    B.c[1] = r % g.nb[1];
    B.c[0] = r / g.nb[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        B.o[a] = B.c[a] * g.b;
        B.ext[a] = min(g.b, g.n[a] - 1 - B.o[a]);
    }
    return B;
}

// ---- lattice and classification --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MCS_THREADS) k_mcs_lattice(McsGrid g, long long n, int* __restrict__ idx) {
    const long long p = (long long)blockIdx.x * MCS_THREADS + threadIdx.x;
    if (p >= n) return;
    const int lz = g.nb[2] + 1, ly = g.nb[1] + 1;
    const int k = (int)(p % lz);
    const long long r = p / lz;
    const int j = (int)(r % ly), i = (int)(r / ly);
    int* o = idx + 3 * p;
    o[0] = min(i * g.b, g.n[0] - 1);
    o[1] = min(j * g.b, g.n[1] - 1);
    o[2] = min(k * g.b, g.n[2] - 1);
}

__global__ void __launch_bounds__(MCS_THREADS) k_mcs_classify(const float* __restrict__ lat, McsGrid g, float thr, float reach,
                                                              unsigned char* __restrict__ mask) {
    const long long blk = (long long)blockIdx.x * MCS_THREADS + threadIdx.x;
    if (blk >= mcs_blocks(g)) return;
    const McsBlock B = mcs_block(g, (int)blk);
    const long long lz = g.nb[2] + 1, ly = g.nb[1] + 1;
    int n_in = 0;
    float near = INFINITY;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float v = lat[((long long)(B.c[0] + (c >> 2)) * ly + B.c[1] + (c >> 1 & 1)) * lz + B.c[2] + (c & 1)];
        n_in += v < thr ? 1 : 0;
        near = fminf(near, fabsf(v - thr));
    }
    mask[blk] = ((n_in != 0 && n_in != 8) || near <= reach) ? 1 : 0;
}

// ---- compaction of the mask ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mask4(const unsigned char* __restrict__ mask, long long p0, long long n, int m[MCS_PPT]) {
#pragma unroll
    for (int u = 0; u < MCS_PPT; ++u) m[u] = (p0 + u < n && mask[p0 + u]) ? 1 : 0;
}

__global__ void __launch_bounds__(MCS_THREADS) k_mcs_mask_count(const unsigned char* __restrict__ mask, long long n, int* __restrict__ wg_n) {
    __shared__ int lds[MCS_THREADS / 64];
    int m[MCS_PPT];
    mask4(mask, ((long long)blockIdx.x * MCS_THREADS + threadIdx.x) * MCS_PPT, n, m);
    int total;
    block_excl_scan<MCS_THREADS>(m[0] + m[1] + m[2] + m[3], lds, total);
    if (threadIdx.x == 0) wg_n[blockIdx.x] = total;
}

// Exclusive scans of one or two arrays of workgroup sums (b may be NULL) by one workgroup: tiles of MCS_SCAN_THREADS x 4 sums, an
// int scan inside the tile, a 64-bit running carry.  totals = {sum a, sum b}.  (hn_mcubes.hip's k_mc_scan.)
__global__ void __launch_bounds__(MCS_SCAN_THREADS) k_mcs_scan(const int* __restrict__ a, const int* __restrict__ b, int n,
                                                               long long* __restrict__ off_a, long long* __restrict__ off_b,
                                                               long long* __restrict__ totals) {
    __shared__ int lds[MCS_SCAN_THREADS / 64];
    long long carry_a = 0, carry_b = 0;
    for (int base = 0; base < n; base += MCS_SCAN_THREADS * 4) {
        const int i0 = base + threadIdx.x * 4;
        int va[4], vb[4], sa = 0, sb = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            va[u] = i0 + u < n ? a[i0 + u] : 0;
            vb[u] = (b && i0 + u < n) ? b[i0 + u] : 0;
            sa += va[u];
            sb += vb[u];
        }
        int tot_a, tot_b;
        long long ea = carry_a + block_excl_scan<MCS_SCAN_THREADS>(sa, lds, tot_a);
        long long eb = carry_b + block_excl_scan<MCS_SCAN_THREADS>(sb, lds, tot_b);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < n) {
                off_a[i0 + u] = ea;
                if (b) off_b[i0 + u] = eb;
            }
            ea += va[u];
            eb += vb[u];
        }
        carry_a += tot_a;
        carry_b += tot_b;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry_a;
        if (b) totals[1] = carry_b;
    }
}

__global__ void __launch_bounds__(MCS_THREADS) k_mcs_mask_emit(const unsigned char* __restrict__ mask, long long n,
                                                               const long long* __restrict__ wg_off, int* __restrict__ list,
                                                               int* __restrict__ table) {
    __shared__ int lds[MCS_THREADS / 64];
    const long long p0 = ((long long)blockIdx.x * MCS_THREADS + threadIdx.x) * MCS_PPT;
    int m[MCS_PPT];
    mask4(mask, p0, n, m);
    int total;
    const int excl = block_excl_scan<MCS_THREADS>(m[0] + m[1] + m[2] + m[3], lds, total);
    long long slot = wg_off[blockIdx.x] + excl;     // < n < 2^31
#pragma unroll
    for (int u = 0; u < MCS_PPT; ++u) {
        if (p0 + u < n) {
            table[p0 + u] = m[u] ? (int)slot : -1;
            if (m[u]) list[slot++] = (int)(p0 + u);
        }
    }
}

// ---- brick indices ---------------------------------------------------------------------------------------------------------------
template <int B>
__global__ void __launch_bounds__(MCS_THREADS) k_mcs_brick_points(const int* __restrict__ list, long long slot_begin, long long n_pts,
                                                                  McsGrid g, int* __restrict__ idx) {
    constexpr int E = B + 1, P = E * E * E;
    const long long q = (long long)blockIdx.x * MCS_THREADS + threadIdx.x;
    if (q >= n_pts) return;
    const long long s = q / P;
    const int p = (int)(q - s * P);
    const McsBlock K = mcs_block(g, list[slot_begin + s]);
    const int l[3] = {p / (E * E), p / E % E, p % E};
    int* o = idx + 3 * q;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = K.o[a] + min(l[a], K.ext[a]);
}

// ---- a brick in LDS ----------------------------------------------------------------------------------------------------------------
// One workgroup per brick: NT threads, PPT consecutive local points per thread (NT PPT >= (B + 1)^3).
template <int B>
struct BrickCfg {
    static constexpr int E = B + 1, P = E * E * E;
    static constexpr int NT = B == 8 ? 256 : 128;
    static constexpr int PPT = (P + NT - 1) / NT;
};

template <int B>
__device__ __forceinline__ void brick_load(const float* __restrict__ bricks, long long slot, float* sv) {
    using C = BrickCfg<B>;
    const float* src = bricks + slot * C::P;
    for (int p = threadIdx.x; p < C::P; p += C::NT) sv[p] = src[p];
    __syncthreads();
}

// What a thread's point contributes: crossing owned edges (bit 0 x, 1 y, 2 z), the inside bit (8), the case of the cell it is the
// origin of (0 where it is none), and where it sits.
struct BrickPoint {
    int l[3];
    int edges;
    int cs;
    bool valid;
};

template <int B>
__device__ __forceinline__ BrickPoint brick_point(const float* sv, const McsGrid& g, const McsBlock& K, int p, float thr) {
    using C = BrickCfg<B>;
    constexpr int E = C::E;
    BrickPoint r;
    r.l[0] = p / (E * E);
    r.l[1] = p / E % E;
    r.l[2] = p % E;
    r.edges = 0;
    r.cs = 0;
    r.valid = p < C::P && r.l[0] <= K.ext[0] && r.l[1] <= K.ext[1] && r.l[2] <= K.ext[2];
    if (!r.valid) return r;
    const int stride[3] = {E * E, E, 1};
    const int i0 = sv[p] < thr ? 1 : 0;
    bool owned = true, cell = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        owned = owned && (r.l[a] < B || K.o[a] + r.l[a] == g.n[a] - 1);
        cell = cell && r.l[a] < K.ext[a];
    }
    if (owned) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (r.l[a] < K.ext[a] && i0 != (sv[p + stride[a]] < thr ? 1 : 0)) r.edges |= 1 << a;
        }
    }
    r.edges |= i0 << 3;
    if (cell) {
        // Bourke's corner order: corner c at ((c & 1) ^ (c >> 1 & 1), c >> 1 & 1, c >> 2)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int dx = (c & 1) ^ (c >> 1 & 1), dy = c >> 1 & 1, dz = c >> 2;
            r.cs |= (sv[p + dx * E * E + dy * E + dz] < thr ? 1 : 0) << c;
        }
    }
    return r;
}

template <int B>
__global__ void __launch_bounds__(BrickCfg<B>::NT) k_mcs_brick_count(const float* __restrict__ bricks, const int* __restrict__ list, McsGrid g,
                                                                     float thr, int* __restrict__ brk_v, int* __restrict__ brk_t) {
    using C = BrickCfg<B>;
    __shared__ float sv[C::P];
    __shared__ int red[2][C::NT / 64];
    const long long slot = blockIdx.x;
    brick_load<B>(bricks, slot, sv);
    const McsBlock K = mcs_block(g, list[slot]);
    int nv = 0, nt = 0;
#pragma unroll
    for (int m = 0; m < C::PPT; ++m) {
        const BrickPoint r = brick_point<B>(sv, g, K, threadIdx.x * C::PPT + m, thr);
        nv += __popc(r.edges & 7);
        nt += c_tri_count[r.cs];
    }
    nv = wave_sum(nv);
    nt = wave_sum(nt);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w] = nv;
        red[1][w] = nt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sa = 0, sb = 0;
#pragma unroll
        for (int u = 0; u < C::NT / 64; ++u) {
            sa += red[0][u];
            sb += red[1][u];
        }
        brk_v[slot] = sa;
        brk_t[slot] = sb;
    }
}

template <int B>
__global__ void __launch_bounds__(BrickCfg<B>::NT) k_mcs_verts(const float* __restrict__ bricks, const int* __restrict__ list, McsGrid g,
                                                               float thr, const long long* __restrict__ off_v, int* __restrict__ vbase,
                                                               unsigned char* __restrict__ flags, float* __restrict__ verts,
                                                               long long* __restrict__ vkeys, long long n_verts) {
    using C = BrickCfg<B>;
    constexpr int E = C::E;
    __shared__ float sv[C::P];
    __shared__ int lds[C::NT / 64];
    const long long slot = blockIdx.x;
    brick_load<B>(bricks, slot, sv);
    const McsBlock K = mcs_block(g, list[slot]);
    BrickPoint r[C::PPT];
    int nv = 0;
#pragma unroll
    for (int m = 0; m < C::PPT; ++m) {
        r[m] = brick_point<B>(sv, g, K, threadIdx.x * C::PPT + m, thr);
        nv += __popc(r[m].edges & 7);
    }
    int total;
    const int excl = block_excl_scan<C::NT>(nv, lds, total);
    long long vid = off_v[slot] + excl;
    const int stride[3] = {E * E, E, 1};
#pragma unroll
    for (int m = 0; m < C::PPT; ++m) {
        const int p = threadIdx.x * C::PPT + m;
        if (!r[m].valid) continue;
        vbase[slot * C::P + p] = (int)vid;
        flags[slot * C::P + p] = (unsigned char)r[m].edges;
        if (!(r[m].edges & 7)) continue;
        const int gi[3] = {K.o[0] + r[m].l[0], K.o[1] + r[m].l[1], K.o[2] + r[m].l[2]};
        const long long lin = ((long long)gi[0] * g.n[1] + gi[1]) * g.n[2] + gi[2];
        const float v0 = sv[p];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (r[m].edges >> a & 1) {
                if (vid < n_verts) {
                    const float v1 = sv[p + stride[a]];
                    const float t = (thr - v0) / (v1 - v0);
                    float* o = verts + 3 * vid;
                    o[0] = (float)gi[0] + (a == 0 ? t : 0.f);
                    o[1] = (float)gi[1] + (a == 1 ? t : 0.f);
                    o[2] = (float)gi[2] + (a == 2 ? t : 0.f);
                    vkeys[vid] = lin * 3 + a;
                }
                ++vid;
            }
        }
    }
}

template <int B>
__global__ void __launch_bounds__(BrickCfg<B>::NT) k_mcs_tris(const float* __restrict__ bricks, const int* __restrict__ list,
                                                              const int* __restrict__ table, McsGrid g, float thr,
                                                              const long long* __restrict__ off_t, const int* __restrict__ vbase,
                                                              const unsigned char* __restrict__ flags, long long* __restrict__ tris,
                                                              long long* __restrict__ tkeys, long long n_tris) {
    using C = BrickCfg<B>;
    constexpr int E = C::E;
    __shared__ float sv[C::P];
    __shared__ int lds[C::NT / 64];
    const long long slot = blockIdx.x;
    brick_load<B>(bricks, slot, sv);
    const int blk = list[slot];
    const McsBlock K = mcs_block(g, blk);
    BrickPoint r[C::PPT];
    int nt = 0;
#pragma unroll
    for (int m = 0; m < C::PPT; ++m) {
        r[m] = brick_point<B>(sv, g, K, threadIdx.x * C::PPT + m, thr);
        nt += c_tri_count[r[m].cs];
    }
    int total;
    const int excl = block_excl_scan<C::NT>(nt, lds, total);
    if (nt == 0) return;
    long long tid = off_t[slot] + excl;
#pragma unroll
    for (int m = 0; m < C::PPT; ++m) {
        const int cs = r[m].cs;
        const int cnt = c_tri_count[cs];
        if (cnt == 0) continue;
        const long long cell = ((long long)(K.o[0] + r[m].l[0]) * g.n[1] + K.o[1] + r[m].l[1]) * g.n[2] + K.o[2] + r[m].l[2];
        for (int s = 0; s < cnt; ++s, ++tid) {
            long long id[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int e = c_tri_table[cs][3 * s + u];
                // the edge's owning point, and the brick that owns that point
                int ol[3], nbr = 0;
                bool own = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int gi = K.o[a] + r[m].l[a] + c_edge_owner[e][a];
                    const int oc = min(gi / g.b, g.nb[a] - 1);
                    ol[a] = gi - oc * g.b;
                    own = own && oc == K.c[a];
                    nbr = nbr * g.nb[a] + oc;
                }
                const long long os = own ? slot : (long long)table[nbr];
                const int axis = c_edge_owner[e][3];
                if (os < 0) {
                    id[u] = -1;   // the owner is not in the band (a leak the caller did not grow away)
                } else {
                    const long long o = os * C::P + (ol[0] * E + ol[1]) * E + ol[2];
                    id[u] = (long long)vbase[o] + __popc(flags[o] & ((1 << axis) - 1));
                }
            }
            if (tid < n_tris) {
                long long* out = tris + 3 * tid;
                out[0] = id[2];   // reversed: the normal points toward increasing value
                out[1] = id[1];
                out[2] = id[0];
                tkeys[tid] = cell * 8 + s;
            }
        }
    }
}

// ---- leaks -----------------------------------------------------------------------------------------------------------------------
// A crossing grid edge on the boundary of an active block lies in up to three more blocks (one across a face, three around a block
// edge).  Each of them that is not in the table is marked in the mask.  Every writer stores the same byte, so the order is immaterial.
template <int B>
__global__ void __launch_bounds__(BrickCfg<B>::NT) k_mcs_leak_mark(const float* __restrict__ bricks, const int* __restrict__ list,
                                                                   const int* __restrict__ table, McsGrid g, float thr,
                                                                   unsigned char* __restrict__ mask) {
    using C = BrickCfg<B>;
    constexpr int E = C::E;
    __shared__ float sv[C::P];
    const long long slot = blockIdx.x;
    brick_load<B>(bricks, slot, sv);
    const McsBlock K = mcs_block(g, list[slot]);
    const int stride[3] = {E * E, E, 1};
#pragma unroll
    for (int m = 0; m < C::PPT; ++m) {
        const int p = threadIdx.x * C::PPT + m;
        const int l[3] = {p / (E * E), p / E % E, p % E};
        if (p >= C::P || l[0] > K.ext[0] || l[1] > K.ext[1] || l[2] > K.ext[2]) continue;
        const bool i0 = sv[p] < thr;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (l[a] >= K.ext[a] || i0 == (sv[p + stride[a]] < thr)) continue;
            // the two transverse axes: the neighbour below where the edge lies on the block's low face, above on its high face
            // (a block has at least one cell, so an edge lies on at most one of the two faces per axis)
            const int u = (a + 1) % 3, w = (a + 2) % 3;
            const int su = (l[u] == 0 && K.c[u] > 0) ? -1 : (l[u] == K.ext[u] && K.c[u] + 1 < g.nb[u]) ? 1 : 0;
            const int sw = (l[w] == 0 && K.c[w] > 0) ? -1 : (l[w] == K.ext[w] && K.c[w] + 1 < g.nb[w]) ? 1 : 0;
#pragma unroll
            for (int q = 1; q < 4; ++q) {      // q & 1: step along u, q & 2: step along w
                if (((q & 1) && !su) || ((q & 2) && !sw)) continue;
                int c[3] = {K.c[0], K.c[1], K.c[2]};
                c[u] += (q & 1) ? su : 0;
                c[w] += (q & 2) ? sw : 0;
                const long long nbr = ((long long)c[0] * g.nb[1] + c[1]) * g.nb[2] + c[2];
                if (table[nbr] < 0) mask[nbr] = 1;
            }
        }
    }
}

__global__ void __launch_bounds__(MCS_THREADS) k_mcs_leak_count(const unsigned char* __restrict__ mask, const int* __restrict__ table,
                                                                long long n, unsigned long long* __restrict__ added) {
    __shared__ int lds[MCS_THREADS / 64];
    const long long p0 = ((long long)blockIdx.x * MCS_THREADS + threadIdx.x) * MCS_PPT;
    int c = 0;
#pragma unroll
    for (int u = 0; u < MCS_PPT; ++u) c += (p0 + u < n && mask[p0 + u] && table[p0 + u] < 0) ? 1 : 0;
    int total;
    block_excl_scan<MCS_THREADS>(c, lds, total);
    if (threadIdx.x == 0 && total) atomicAdd(added, (unsigned long long)total);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
int mcs_grid(const char* who, int nx, int ny, int nz, int block, McsGrid& g) {
    HN_REQUIRE(block == 4 || block == 8, "%s: block must be 4 or 8 (got %d)", who, block);
    HN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && nx <= MCS_MAX_DIM && ny <= MCS_MAX_DIM && nz <= MCS_MAX_DIM,
               "%s: every dim must be >= 2 and <= %d (got %d x %d x %d)", who, MCS_MAX_DIM, nx, ny, nz);
    g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
    g.b = block;
    for (int a = 0; a < 3; ++a) g.nb[a] = (g.n[a] - 1 + block - 1) / block;
    return HN_OK;     // at most 512^3 blocks and 513^3 lattice points: both fit int32
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct McsLayout {
    long long n_wg = 0;       // workgroups of the mask passes
    size_t wg_n = 0, wg_off = 0, brk_v = 0, brk_t = 0, off_v = 0, off_t = 0, vbase = 0, flags = 0, bytes = 0;
};

int mcs_layout(const char* who, const McsGrid& g, long long n_slots, McsLayout& L) {
    const long long nblk = mcs_blocks(g);
    HN_REQUIRE(n_slots >= 0 && n_slots <= nblk, "%s: n_slots = %lld outside [0, %lld blocks]", who, n_slots, nblk);
    const long long P = (long long)(g.b + 1) * (g.b + 1) * (g.b + 1);
    L.n_wg = (nblk + MCS_PPB - 1) / MCS_PPB;
    size_t at = 0;
    L.wg_n = at, at = align256(at + sizeof(int) * L.n_wg);
    L.wg_off = at, at = align256(at + sizeof(long long) * L.n_wg);
    L.brk_v = at, at = align256(at + sizeof(int) * n_slots);
    L.brk_t = at, at = align256(at + sizeof(int) * n_slots);
    L.off_v = at, at = align256(at + sizeof(long long) * n_slots);
    L.off_t = at, at = align256(at + sizeof(long long) * n_slots);
    L.vbase = at, at = align256(at + sizeof(int) * n_slots * P);
    L.flags = at, at = align256(at + n_slots * P);
    L.bytes = at;
    return HN_OK;
}

unsigned grid_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_mcs_workspace_bytes(int nx, int ny, int nz, int block, long long n_slots) {
    McsGrid g;
    McsLayout L;
    if (mcs_grid("hn_mcs_workspace_bytes", nx, ny, nz, block, g) != HN_OK) return 0;
    return mcs_layout("hn_mcs_workspace_bytes", g, n_slots, L) == HN_OK ? L.bytes : 0;
}

int hn_mcs_lattice(int nx, int ny, int nz, int block, int* indices, hn_stream_t stream) {
    McsGrid g;
    HN_TRY_RC(mcs_grid("hn_mcs_lattice", nx, ny, nz, block, g));
    HN_REQUIRE(indices, "hn_mcs_lattice: NULL indices");
    const long long n = mcs_lattice(g);
    k_mcs_lattice<<<grid_of(n, MCS_THREADS), MCS_THREADS, 0, (hipStream_t)stream>>>(g, n, indices);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcs_classify(const float* lattice_values, int nx, int ny, int nz, int block, float threshold, float reach, unsigned char* mask,
                    hn_stream_t stream) {
    McsGrid g;
    HN_TRY_RC(mcs_grid("hn_mcs_classify", nx, ny, nz, block, g));
    HN_REQUIRE(lattice_values && mask, "hn_mcs_classify: NULL lattice_values / mask");
    HN_REQUIRE(reach >= 0.f, "hn_mcs_classify: reach must be >= 0 (got %g)", (double)reach);
    k_mcs_classify<<<grid_of(mcs_blocks(g), MCS_THREADS), MCS_THREADS, 0, (hipStream_t)stream>>>(lattice_values, g, threshold, reach, mask);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcs_compact(const unsigned char* mask, int nx, int ny, int nz, int block, int* list, int* table, long long* total, void* workspace,
                   size_t workspace_bytes, hn_stream_t stream) {
    McsGrid g;
    McsLayout L;
    HN_TRY_RC(mcs_grid("hn_mcs_compact", nx, ny, nz, block, g));
    HN_TRY_RC(mcs_layout("hn_mcs_compact", g, 0, L));
    HN_REQUIRE(mask && list && table && total && workspace, "hn_mcs_compact: NULL mask / list / table / total / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_mcs_compact: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_mcs_compact: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const long long n = mcs_blocks(g);
    int* wg_n = (int*)(ws + L.wg_n);
    long long* wg_off = (long long*)(ws + L.wg_off);
    k_mcs_mask_count<<<(unsigned)L.n_wg, MCS_THREADS, 0, s>>>(mask, n, wg_n);
    HN_LAUNCH_CHECK();
    k_mcs_scan<<<1, MCS_SCAN_THREADS, 0, s>>>(wg_n, nullptr, (int)L.n_wg, wg_off, nullptr, total);
    HN_LAUNCH_CHECK();
    k_mcs_mask_emit<<<(unsigned)L.n_wg, MCS_THREADS, 0, s>>>(mask, n, wg_off, list, table);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcs_brick_points(const int* list, long long slot_begin, long long slot_end, int nx, int ny, int nz, int block, int* indices,
                        hn_stream_t stream) {
    McsGrid g;
    HN_TRY_RC(mcs_grid("hn_mcs_brick_points", nx, ny, nz, block, g));
    HN_REQUIRE(slot_begin >= 0 && slot_begin <= slot_end && slot_end <= mcs_blocks(g), "hn_mcs_brick_points: slots [%lld, %lld) outside the %lld blocks",
               slot_begin, slot_end, mcs_blocks(g));
    if (slot_begin == slot_end) return HN_OK;
    HN_REQUIRE(list && indices, "hn_mcs_brick_points: NULL list / indices");
    const long long P = (long long)(block + 1) * (block + 1) * (block + 1), n_pts = (slot_end - slot_begin) * P;
    HN_REQUIRE(n_pts < (1LL << 31) * MCS_THREADS, "hn_mcs_brick_points: %lld points in one call", n_pts);
    if (block == 8)
        k_mcs_brick_points<8><<<grid_of(n_pts, MCS_THREADS), MCS_THREADS, 0, (hipStream_t)stream>>>(list, slot_begin, n_pts, g, indices);
    else
        k_mcs_brick_points<4><<<grid_of(n_pts, MCS_THREADS), MCS_THREADS, 0, (hipStream_t)stream>>>(list, slot_begin, n_pts, g, indices);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcs_leaks(const float* bricks, const int* list, const int* table, long long n_slots, int nx, int ny, int nz, int block, float threshold,
                 unsigned char* mask, long long* added, hn_stream_t stream) {
    McsGrid g;
    HN_TRY_RC(mcs_grid("hn_mcs_leaks", nx, ny, nz, block, g));
    const long long n = mcs_blocks(g);
    HN_REQUIRE(n_slots >= 0 && n_slots <= n, "hn_mcs_leaks: n_slots = %lld outside [0, %lld blocks]", n_slots, n);
    HN_REQUIRE(table && mask && added, "hn_mcs_leaks: NULL table / mask / added");
    HN_REQUIRE(n_slots == 0 || (bricks && list), "hn_mcs_leaks: NULL bricks / list");
    hipStream_t s = (hipStream_t)stream;
    HN_CHECK_HIP(hipMemsetAsync(added, 0, sizeof(long long), s));
    if (n_slots == 0) return HN_OK;
    if (block == 8)
        k_mcs_leak_mark<8><<<(unsigned)n_slots, BrickCfg<8>::NT, 0, s>>>(bricks, list, table, g, threshold, mask);
    else
        k_mcs_leak_mark<4><<<(unsigned)n_slots, BrickCfg<4>::NT, 0, s>>>(bricks, list, table, g, threshold, mask);
    HN_LAUNCH_CHECK();
    k_mcs_leak_count<<<grid_of(n, MCS_PPB), MCS_THREADS, 0, s>>>(mask, table, n, (unsigned long long*)added);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcs_count(const float* bricks, const int* list, long long n_slots, int nx, int ny, int nz, int block, float threshold, long long* totals,
                 void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    McsGrid g;
    McsLayout L;
    HN_TRY_RC(mcs_grid("hn_mcs_count", nx, ny, nz, block, g));
    HN_TRY_RC(mcs_layout("hn_mcs_count", g, n_slots, L));
    HN_REQUIRE(totals, "hn_mcs_count: NULL totals");
    hipStream_t s = (hipStream_t)stream;
    if (n_slots == 0) {
        HN_CHECK_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(long long), s));
        return HN_OK;
    }
    HN_REQUIRE(bricks && list && workspace, "hn_mcs_count: NULL bricks / list / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_mcs_count: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_mcs_count: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    int* brk_v = (int*)(ws + L.brk_v);
    int* brk_t = (int*)(ws + L.brk_t);
    if (block == 8)
        k_mcs_brick_count<8><<<(unsigned)n_slots, BrickCfg<8>::NT, 0, s>>>(bricks, list, g, threshold, brk_v, brk_t);
    else
        k_mcs_brick_count<4><<<(unsigned)n_slots, BrickCfg<4>::NT, 0, s>>>(bricks, list, g, threshold, brk_v, brk_t);
    HN_LAUNCH_CHECK();
    k_mcs_scan<<<1, MCS_SCAN_THREADS, 0, s>>>(brk_v, brk_t, (int)n_slots, (long long*)(ws + L.off_v), (long long*)(ws + L.off_t), totals);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_mcs_emit(const float* bricks, const int* list, const int* table, long long n_slots, int nx, int ny, int nz, int block, float threshold,
                void* workspace, size_t workspace_bytes, long long n_verts, long long n_tris, float* vertices, long long* vertex_keys,
                long long* triangles, long long* triangle_keys, hn_stream_t stream) {
    McsGrid g;
    McsLayout L;
    HN_TRY_RC(mcs_grid("hn_mcs_emit", nx, ny, nz, block, g));
    HN_TRY_RC(mcs_layout("hn_mcs_emit", g, n_slots, L));
    HN_REQUIRE(n_verts >= 0 && n_tris >= 0 && n_verts < (1LL << 31) && n_tris < (1LL << 31),
               "hn_mcs_emit: bad sizes V = %lld, T = %lld (vertex ids are int32 in the workspace)", n_verts, n_tris);
    if (n_slots == 0 || n_verts == 0 || n_tris == 0) return HN_OK;   // no crossing: nothing to launch
    HN_REQUIRE(bricks && list && table && workspace, "hn_mcs_emit: NULL bricks / list / table / workspace");
    HN_REQUIRE(vertices && vertex_keys && triangles && triangle_keys, "hn_mcs_emit: NULL vertices / vertex_keys / triangles / triangle_keys");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_mcs_emit: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_mcs_emit: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const long long* off_v = (const long long*)(ws + L.off_v);
    const long long* off_t = (const long long*)(ws + L.off_t);
    int* vbase = (int*)(ws + L.vbase);
    unsigned char* flags = (unsigned char*)(ws + L.flags);
    if (block == 8) {
        k_mcs_verts<8><<<(unsigned)n_slots, BrickCfg<8>::NT, 0, s>>>(bricks, list, g, threshold, off_v, vbase, flags, vertices, vertex_keys, n_verts);
        HN_LAUNCH_CHECK();
        k_mcs_tris<8><<<(unsigned)n_slots, BrickCfg<8>::NT, 0, s>>>(bricks, list, table, g, threshold, off_t, vbase, flags, triangles,
                                                                   triangle_keys, n_tris);
    } else {
        k_mcs_verts<4><<<(unsigned)n_slots, BrickCfg<4>::NT, 0, s>>>(bricks, list, g, threshold, off_v, vbase, flags, vertices, vertex_keys, n_verts);
        HN_LAUNCH_CHECK();
        k_mcs_tris<4><<<(unsigned)n_slots, BrickCfg<4>::NT, 0, s>>>(bricks, list, table, g, threshold, off_t, vbase, flags, triangles,
                                                                   triangle_keys, n_tris);
    }
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
