// Connected components of a triangle mesh on the device: label them, measure each, keep some.  The step behind marching cubes that
// trimesh's Trimesh.split / .area / .volume / .is_watertight make on the host.  DESIGN.md 3.23 is the contract; tests/meshcc_cases.py
// restates it in numpy.
//
// Semantics:
//   * two triangles belong to the same component when they share a vertex INDEX, transitively.  This is vertex connectivity; trimesh's
//     split joins faces over shared edges.  The two differ only at pinch vertices (two fans meeting in one vertex and no edge): one
//     component here, two there;
//   * a component's LABEL is the smallest vertex index any of its triangles uses;
//   * vertex_label[v] (int32) is that label, -1 for a vertex no triangle uses; face_label[f] is the label of its vertices;
//   * a triangle with a repeated index is a face like any other;
//   * a triangle with an index outside [0, n_verts) is never dereferenced, joins nothing and gets face_label -1 (hn_meshcast_prepare's
//     rule);
//   * components are numbered 0 .. C-1 in ascending label order: the component INDEX.  vertex_component / face_component (int32, -1
//     as above) carry it, label[i] is the label of component i;
//   * every output is the same bits on every run, whatever the schedule.
//
// Labelling is a lock-free union-find over the vertex array (ws: parent[V]).  One thread per triangle: unite(a, b), unite(b, c).  A
// link is made only from a root to a SMALLER root, by a compare-and-swap on the larger root's own slot, so
//   parent[x] <= x always; every find walk strictly descends (at most x steps); a failed swap means another thread linked that root,
//   and at most V - 1 links succeed in all, so every retry loop is bounded; the final root of a component is its smallest index.
// Inside the linking launch parent[] is touched ONLY by agent-scope relaxed atomics (load, compare-exchange, min): a plain load may be
// served from an XCD's own L2 and never see another XCD's link.  A stale value is harmless (it is an older ancestor, still >= the
// root); the walk is shortened by path halving with atomicMin, which can only move a pointer to a smaller member of the same tree
// and never undoes a link, as a plain store could.  Flattening (find for every vertex, plain loads) is a launch of its own.
//
// Passes of hn_meshcc_label:   k_cc_init -> k_cc_link -> k_cc_flatten (labels, root counts per block) -> k_cc_scan (block offsets,
//   C) -> k_cc_rank (root -> index, label[]) -> k_cc_finish (vertex_component, face_label, face_component).
// Passes of hn_meshcc_measure: k_cc_zero -> k_cc_count (integer atomics, one per wave where the wave is uniform) -> k_cc_segments
//   (one workgroup: where each component's faces start in `face_order`, its chunks of 256 faces) -> k_cc_terms (one workgroup per
//   chunk: the 256 faces' fp64 terms reduced by a fixed tree) -> k_cc_sum (one workgroup per component: its chunks' partial sums in
//   ascending order, thread t adding chunks t, t + 256, .., then the same tree).  `face_order` lists the faces by component, each
//   component's in ascending face order (a stable sort of face_component), so a component's sum has one association, fixed by the
//   mesh.  No float atomics.  Terms, from the vertices converted to fp64 and with -ffp-contract=off:
//     area   0.5 * sqrt((nx nx + ny ny) + nz nz), n = (b - a) x (c - a);     volume  ((a0 x0 + a1 x1) + a2 x2) / 6, x = b x c.
// Passes of the compaction: count (k_cc_keep_count, k_cc_scan twice -> totals {V', T'}), then emit (k_cc_emit_verts, k_cc_emit_faces):
//   kept vertices and faces in their original order, rows copied bit for bit, triangles re-indexed through vertex_map.
#include "hn_common.h"

namespace hn {
namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_CHUNK = 256;                          // faces per chunk of k_cc_terms: one workgroup
constexpr int CC_PART = 8;                             // doubles per chunk: area, volume, lo[3], hi[3]
constexpr long long CC_MAX = (1LL << 31) - 256;

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct CcLayout {                                      // hn_meshcc_label and the compaction
    long long nbv = 0, nbt = 0;
    size_t parent = 0, used = 0, rank = 0, blk_v = 0, off_v = 0, blk_t = 0, off_t = 0, bytes = 0;
};

int cc_layout(long long n_verts, long long n_tris, CcLayout& L) {
    HN_REQUIRE(n_verts >= 0 && n_verts < CC_MAX, "hn_meshcc: n_verts = %lld outside [0, 2^31 - 256)", n_verts);
    HN_REQUIRE(n_tris >= 0 && n_tris < CC_MAX, "hn_meshcc: n_tris = %lld outside [0, 2^31 - 256)", n_tris);
    L.nbv = (n_verts + CC_THREADS - 1) / CC_THREADS;
    L.nbt = (n_tris + CC_THREADS - 1) / CC_THREADS;
    size_t at = 0;
    L.parent = at, at = align256(at + sizeof(int) * (size_t)n_verts);
    L.used = at, at = align256(at + sizeof(int) * (size_t)n_verts);
    L.rank = at, at = align256(at + sizeof(int) * (size_t)n_verts);
    L.blk_v = at, at = align256(at + sizeof(int) * (size_t)L.nbv);
    L.off_v = at, at = align256(at + sizeof(int) * (size_t)L.nbv);
    L.blk_t = at, at = align256(at + sizeof(int) * (size_t)L.nbt);
    L.off_t = at, at = align256(at + sizeof(int) * (size_t)L.nbt);
    L.bytes = at > 256 ? at : 256;
    return HN_OK;
}

struct CmLayout {                                      // hn_meshcc_measure
    long long max_chunks = 0;
    size_t fcnt = 0, seg = 0, chunk = 0, part = 0, bytes = 0;
};

int cm_layout(long long n_tris, long long n_comp, CmLayout& L) {
    HN_REQUIRE(n_tris >= 0 && n_tris < CC_MAX, "hn_meshcc_measure: n_tris = %lld outside [0, 2^31 - 256)", n_tris);
    HN_REQUIRE(n_comp >= 0 && n_comp < CC_MAX, "hn_meshcc_measure: n_comp = %lld outside [0, 2^31 - 256)", n_comp);
    L.max_chunks = n_tris / CC_CHUNK + n_comp;         // sum over components of ceil(n_c / 256) <= T / 256 + C
    size_t at = 0;
    L.fcnt = at, at = align256(at + sizeof(int) * (size_t)(n_comp + 1));
    L.seg = at, at = align256(at + sizeof(int) * (size_t)(n_comp + 1));
    L.chunk = at, at = align256(at + sizeof(int) * (size_t)(n_comp + 1));
    L.part = at, at = align256(at + sizeof(double) * CC_PART * (size_t)L.max_chunks);
    L.bytes = at > 256 ? at : 256;
    return HN_OK;
}

unsigned grid_of(long long n) { return (unsigned)(n > 0 ? (n + CC_THREADS - 1) / CC_THREADS : 1); }

// ---- small reductions ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// Exclusive scan of one int per thread over the workgroup; `total` receives the workgroup's sum (hn_mcubes.hip's).
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int& total) {
    constexpr int NW = CC_THREADS / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        const int s = lds[u];
        before += u < w ? s : 0;
        total += s;
    }
    __syncthreads();   // lds may be written again by the caller's next scan
    return before + incl - v;
}

__device__ __forceinline__ int block_sum(int v, int* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int u = 0; u < CC_THREADS / 64; ++u) s += lds[u];
    __syncthreads();
    return s;
}

// The fixed tree of the fp64 sums: lanes pairwise at distance 32, 16, .., 1, then the four waves in order.  Valid in thread 0.
__device__ __forceinline__ double block_tree_sum(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    __syncthreads();
    return s;
}

__device__ __forceinline__ double block_min(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = fmin(fmin(lds[0], lds[1]), fmin(lds[2], lds[3]));
    __syncthreads();
    return s;
}

__device__ __forceinline__ double block_max(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
    __syncthreads();
    return s;
}

// ---- labelling -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_load(int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as seen now.  parent[y] <= y: the walk strictly descends.  Path halving: x is pointed at its grandparent with an
// atomic min, which only ever lowers a pointer, to a member of the same tree.
__device__ __forceinline__ int cc_find(int* parent, int x) {
    int p = cc_load(parent, x);
    while (p != x) {
        const int g = cc_load(parent, p);
        if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b, b = s;
        }
        int expected = a;                              // a > b: link the larger root under the smaller, if it still is a root
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_init(int* __restrict__ parent, int* __restrict__ used, int n_verts) {
    const int v = blockIdx.x * CC_THREADS + threadIdx.x;
    if (v < n_verts) {
        parent[v] = v;
        used[v] = 0;
    }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_link(const long long* __restrict__ tris, int n_tris, long long n_verts, int* parent,
                                                        int* __restrict__ used) {
    const int f = blockIdx.x * CC_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    const long long i0 = tris[3LL * f], i1 = tris[3LL * f + 1], i2 = tris[3LL * f + 2];
    if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return;   // never dereferenced, joins nothing
    const int a = (int)i0, b = (int)i1, c = (int)i2;
    used[a] = 1, used[b] = 1, used[c] = 1;             // (the same value from every writer; read by the next launch)
    cc_unite(parent, a, b);
    cc_unite(parent, b, c);
}

// After the linking launch: plain loads, nobody writes parent[].
__global__ void __launch_bounds__(CC_THREADS) k_cc_flatten(const int* __restrict__ parent, const int* __restrict__ used, int n_verts,
                                                           int* __restrict__ vertex_label, int* __restrict__ blk) {
    __shared__ int lds[CC_THREADS / 64];
    const int v = blockIdx.x * CC_THREADS + threadIdx.x;
    int root_here = 0;
    if (v < n_verts) {
        int lab = -1;
        if (used[v]) {
            int x = v, p = parent[x];
            while (p != x) x = p, p = parent[x];       // strictly descending
            lab = x;
        }
        vertex_label[v] = lab;
        root_here = lab == v;
    }
    const int s = block_sum(root_here, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = s;
}

// One workgroup: exclusive scan of nb block sums (their total is below 2^31: a count of vertices or faces) -> offsets, total.
__global__ void __launch_bounds__(CC_THREADS) k_cc_scan(const int* __restrict__ blk, int nb, int* __restrict__ off, long long* __restrict__ total) {
    __shared__ int lds[CC_THREADS / 64];
    int carry = 0;
    for (int base = 0; base < nb; base += CC_THREADS * 4) {
        const int b0 = base + threadIdx.x * 4;
        int v[4], sv = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = b0 + u < nb ? blk[b0 + u] : 0;
            sv += v[u];
        }
        int tot;
        int e = carry + block_excl_scan(sv, lds, tot);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b0 + u < nb) off[b0 + u] = e;
            e += v[u];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_rank(const int* __restrict__ vertex_label, int n_verts, const int* __restrict__ off,
                                                        int* __restrict__ rank, int* __restrict__ label) {
    __shared__ int lds[CC_THREADS / 64];
    const int v = blockIdx.x * CC_THREADS + threadIdx.x;
    const int root_here = v < n_verts && vertex_label[v] == v;
    int total;
    const int r = off[blockIdx.x] + block_excl_scan(root_here, lds, total);
    if (root_here) {
        rank[v] = r;
        label[r] = v;                                  // r < C <= n_verts
    }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_finish(const long long* __restrict__ tris, int n_tris, int n_verts, const int* __restrict__ vertex_label,
                                                          const int* __restrict__ rank, int* __restrict__ vertex_component,
                                                          int* __restrict__ face_label, int* __restrict__ face_component) {
    const int i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < n_verts) {
        const int lab = vertex_label[i];
        vertex_component[i] = lab >= 0 ? rank[lab] : -1;
    }
    if (i < n_tris) {
        const long long i0 = tris[3LL * i], i1 = tris[3LL * i + 1], i2 = tris[3LL * i + 2];
        int lab = -1;
        if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) lab = vertex_label[i0];
        face_label[i] = lab;
        face_component[i] = lab >= 0 ? rank[lab] : -1;
    }
}

// ---- measures ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) k_cc_zero(int* __restrict__ fcnt, unsigned long long* __restrict__ vcount, int n_comp) {
    const int i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i <= n_comp) fcnt[i] = 0;
    if (i < n_comp) vcount[i] = 0ULL;
}

// One integer add per wave where every lane of the wave counts into the same slot (the usual case: neighbours share a component).
template <typename T>
__device__ __forceinline__ void wave_count(T* slots, int slot, bool active) {
    const unsigned long long m = __ballot(active);
    if (m == 0ULL) return;
    const int first = __shfl(slot, __ffsll((long long)m) - 1, 64);
    const bool uniform = __ballot(active && slot != first) == 0ULL;
    if (uniform) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(slots + slot, (T)__popcll(m));
    } else if (active) {
        atomicAdd(slots + slot, (T)1);
    }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_count(const int* __restrict__ vertex_component, int n_verts, const int* __restrict__ face_component,
                                                         int n_tris, int n_comp, int* __restrict__ fcnt, unsigned long long* __restrict__ vcount) {
    const int i = blockIdx.x * CC_THREADS + threadIdx.x;
    int fc = 0;
    if (i < n_tris) {
        const int c = face_component[i];
        fc = c >= 0 && c < n_comp ? c + 1 : 0;        // slot 0: the faces of no component, in front of all others in face_order
    }
    wave_count(fcnt, fc, i < n_tris);
    int vc = -1;
    if (i < n_verts) vc = vertex_component[i];
    const bool counted = vc >= 0 && vc < n_comp;
    wave_count(vcount, counted ? vc : 0, counted);
}

// One workgroup: seg[c] = where component c's faces start in face_order, chunk[c] = its first chunk; seg[C], chunk[C] the ends.
__global__ void __launch_bounds__(CC_THREADS) k_cc_segments(const int* __restrict__ fcnt, int n_comp, int* __restrict__ seg, int* __restrict__ chunk,
                                                            long long* __restrict__ faces) {
    __shared__ int lds[CC_THREADS / 64];
    int carry_f = fcnt[0], carry_c = 0;
    for (int base = 0; base < n_comp; base += CC_THREADS) {
        const int c = base + threadIdx.x;
        const int n = c < n_comp ? fcnt[c + 1] : 0;
        const int k = (n + CC_CHUNK - 1) / CC_CHUNK;
        int tot_f, tot_c;
        const int ef = carry_f + block_excl_scan(n, lds, tot_f);
        const int ec = carry_c + block_excl_scan(k, lds, tot_c);
        if (c < n_comp) {
            seg[c] = ef;
            chunk[c] = ec;
            faces[c] = n;
        }
        carry_f += tot_f;
        carry_c += tot_c;
    }
    if (threadIdx.x == 0) {
        seg[n_comp] = carry_f;
        chunk[n_comp] = carry_c;
    }
}

template <typename VT>
__global__ void __launch_bounds__(CC_THREADS) k_cc_terms(const VT* __restrict__ verts, long long n_verts, const long long* __restrict__ tris, int n_tris,
                                                         const int* __restrict__ face_component, const long long* __restrict__ face_order, int n_comp,
                                                         const int* __restrict__ seg, const int* __restrict__ chunk, int max_chunks,
                                                         double* __restrict__ part) {
    __shared__ double lds[CC_THREADS / 64];
    const int q = blockIdx.x;
    if (q >= chunk[n_comp] || q >= max_chunks) return;   // (the same decision in every thread: the grid is the host's upper bound)
    int lo = 0, hi = n_comp;                             // the c with chunk[c] <= q < chunk[c + 1]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (chunk[mid] <= q) lo = mid;
        else hi = mid;
    }
    const int c = lo;
    const int j = (q - chunk[c]) * CC_CHUNK + threadIdx.x;
    const int n = seg[c + 1] - seg[c];
    const double inf = __builtin_inf();
    double area = 0.0, vol = 0.0, mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    if (j < n) {
        const long long pos = (long long)seg[c] + j;
        const long long f = pos < n_tris ? face_order[pos] : -1;
        if (f >= 0 && f < n_tris && face_component[f] == c) {
            const long long i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
            if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {
                double a[3], b[3], d[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    a[u] = (double)verts[3 * i0 + u];
                    b[u] = (double)verts[3 * i1 + u];
                    d[u] = (double)verts[3 * i2 + u];
                    mn[u] = fmin(a[u], fmin(b[u], d[u]));
                    mx[u] = fmax(a[u], fmax(b[u], d[u]));
                }
                const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
                const double e2x = d[0] - a[0], e2y = d[1] - a[1], e2z = d[2] - a[2];
                const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
                area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
                const double x0 = b[1] * d[2] - b[2] * d[1], x1 = b[2] * d[0] - b[0] * d[2], x2 = b[0] * d[1] - b[1] * d[0];
                vol = ((a[0] * x0 + a[1] * x1) + a[2] * x2) / 6.0;
            }
        }
    }
    area = block_tree_sum(area, lds);
    vol = block_tree_sum(vol, lds);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        mn[u] = block_min(mn[u], lds);
        mx[u] = block_max(mx[u], lds);
    }
    if (threadIdx.x == 0) {
        double* p = part + (size_t)CC_PART * q;
        p[0] = area, p[1] = vol;
        p[2] = mn[0], p[3] = mn[1], p[4] = mn[2];
        p[5] = mx[0], p[6] = mx[1], p[7] = mx[2];
    }
}

template <typename VT>
__global__ void __launch_bounds__(CC_THREADS) k_cc_sum(const double* __restrict__ part, const int* __restrict__ chunk, int n_comp, int max_chunks,
                                                       double* __restrict__ area_out, double* __restrict__ volume_out, VT* __restrict__ bounds) {
    __shared__ double lds[CC_THREADS / 64];
    const int c = blockIdx.x;
    if (c >= n_comp) return;
    const int q0 = chunk[c];
    int q1 = chunk[c + 1];
    q1 = q1 < max_chunks ? q1 : max_chunks;
    const double inf = __builtin_inf();
    double area = 0.0, vol = 0.0, mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (int q = q0 + (int)threadIdx.x; q < q1; q += CC_THREADS) {   // thread t: chunks t, t + 256, .. in ascending order
        const double* p = part + (size_t)CC_PART * q;
        area = area + p[0];
        vol = vol + p[1];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            mn[u] = fmin(mn[u], p[2 + u]);
            mx[u] = fmax(mx[u], p[5 + u]);
        }
    }
    area = block_tree_sum(area, lds);
    vol = block_tree_sum(vol, lds);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        mn[u] = block_min(mn[u], lds);
        mx[u] = block_max(mx[u], lds);
    }
    if (threadIdx.x == 0) {
        area_out[c] = area;
        volume_out[c] = vol;
#pragma unroll
        for (int u = 0; u < 3; ++u) {                  // (exact: the values are the caller's own, converted up and back)
            bounds[6LL * c + u] = (VT)mn[u];
            bounds[6LL * c + 3 + u] = (VT)mx[u];
        }
    }
}

// ---- compaction ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_kept(const int* comp, int i, int n, const unsigned char* keep, int n_comp) {
    if (i >= n) return 0;
    const int c = comp[i];
    return c >= 0 && c < n_comp && keep[c] != 0;
}

// Workgroups [0, nbv) count kept vertices, [nbv, nbv + nbt) kept faces.
__global__ void __launch_bounds__(CC_THREADS) k_cc_keep_count(const int* __restrict__ vertex_component, int n_verts, const int* __restrict__ face_component,
                                                              int n_tris, const unsigned char* __restrict__ keep, int n_comp, int nbv,
                                                              int* __restrict__ blk_v, int* __restrict__ blk_t) {
    __shared__ int lds[CC_THREADS / 64];
    const bool faces = (int)blockIdx.x >= nbv;
    const int b = faces ? blockIdx.x - nbv : blockIdx.x;
    const int i = b * CC_THREADS + threadIdx.x;
    const int k = faces ? cc_kept(face_component, i, n_tris, keep, n_comp) : cc_kept(vertex_component, i, n_verts, keep, n_comp);
    const int s = block_sum(k, lds);
    if (threadIdx.x == 0) (faces ? blk_t : blk_v)[b] = s;
}

template <typename VT>
__global__ void __launch_bounds__(CC_THREADS) k_cc_emit_verts(const VT* __restrict__ verts, int n_verts, const int* __restrict__ vertex_component,
                                                              const unsigned char* __restrict__ keep, int n_comp, const int* __restrict__ off_v,
                                                              int n_out, VT* __restrict__ verts_out, int* __restrict__ vertex_map) {
    __shared__ int lds[CC_THREADS / 64];
    const int v = blockIdx.x * CC_THREADS + threadIdx.x;
    const int k = cc_kept(vertex_component, v, n_verts, keep, n_comp);
    int total;
    const int at = off_v[blockIdx.x] + block_excl_scan(k, lds, total);
    if (v >= n_verts) return;
    const bool write = k && at < n_out;
    vertex_map[v] = write ? at : -1;
    if (write) {
#pragma unroll
        for (int u = 0; u < 3; ++u) verts_out[3LL * at + u] = verts[3LL * v + u];
    }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_emit_faces(const long long* __restrict__ tris, int n_tris, int n_verts,
                                                              const int* __restrict__ face_component, const unsigned char* __restrict__ keep, int n_comp,
                                                              const int* __restrict__ off_t, const int* __restrict__ vertex_map, int n_out,
                                                              long long* __restrict__ tris_out, int* __restrict__ face_map) {
    __shared__ int lds[CC_THREADS / 64];
    const int f = blockIdx.x * CC_THREADS + threadIdx.x;
    const int k = cc_kept(face_component, f, n_tris, keep, n_comp);
    int total;
    const int at = off_t[blockIdx.x] + block_excl_scan(k, lds, total);
    if (f >= n_tris) return;
    const bool write = k && at < n_out;
    face_map[f] = write ? at : -1;
    if (write) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const long long i = tris[3LL * f + u];
            tris_out[3LL * at + u] = i >= 0 && i < n_verts ? (long long)vertex_map[i] : -1LL;
        }
    }
}

}  // namespace
}  // namespace hn

using namespace hn;

extern "C" {

size_t hn_meshcc_workspace_bytes(long long n_verts, long long n_tris) {
    CcLayout L;
    return cc_layout(n_verts, n_tris, L) == HN_OK ? L.bytes : 0;
}

size_t hn_meshcc_measure_workspace_bytes(long long n_tris, long long n_comp) {
    CmLayout L;
    return cm_layout(n_tris, n_comp, L) == HN_OK ? L.bytes : 0;
}

int hn_meshcc_label(const long long* triangles, long long n_verts, long long n_tris, int* vertex_label, int* face_label, int* vertex_component,
                    int* face_component, int* label, long long* total, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    CcLayout L;
    HN_TRY_RC(cc_layout(n_verts, n_tris, L));
    if (n_tris == 0) return HN_OK;                       // nothing to launch: the caller fills the outputs
    HN_REQUIRE(triangles && face_label && face_component && total && workspace, "hn_meshcc_label: NULL triangles / face outputs / total / workspace");
    HN_REQUIRE(n_verts == 0 || (vertex_label && vertex_component && label), "hn_meshcc_label: NULL vertex_label / vertex_component / label");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshcc_label: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshcc_label: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int *parent = (int*)(ws + L.parent), *used = (int*)(ws + L.used), *rank = (int*)(ws + L.rank), *blk = (int*)(ws + L.blk_v), *off = (int*)(ws + L.off_v);
    const int V = (int)n_verts, T = (int)n_tris;
    if (V > 0) {
        k_cc_init<<<grid_of(V), CC_THREADS, 0, s>>>(parent, used, V);
        HN_LAUNCH_CHECK();
        k_cc_link<<<grid_of(T), CC_THREADS, 0, s>>>(triangles, T, n_verts, parent, used);
        HN_LAUNCH_CHECK();
        k_cc_flatten<<<(unsigned)L.nbv, CC_THREADS, 0, s>>>(parent, used, V, vertex_label, blk);
        HN_LAUNCH_CHECK();
    }
    k_cc_scan<<<1, CC_THREADS, 0, s>>>(blk, (int)L.nbv, off, total);
    HN_LAUNCH_CHECK();
    if (V > 0) {
        k_cc_rank<<<(unsigned)L.nbv, CC_THREADS, 0, s>>>(vertex_label, V, off, rank, label);
        HN_LAUNCH_CHECK();
    }
    k_cc_finish<<<grid_of(V > T ? V : T), CC_THREADS, 0, s>>>(triangles, T, V, vertex_label, rank, vertex_component, face_label, face_component);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_meshcc_measure(const void* vertices, int vertices_f64, long long n_verts, const long long* triangles, long long n_tris, const int* vertex_component,
                      const int* face_component, const long long* face_order, long long n_comp, long long* faces, long long* vertices_used, double* area,
                      double* volume, void* bounds, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    CmLayout L;
    HN_TRY_RC(cm_layout(n_tris, n_comp, L));
    HN_REQUIRE(n_verts >= 0 && n_verts < CC_MAX, "hn_meshcc_measure: n_verts = %lld outside [0, 2^31 - 256)", n_verts);
    if (n_tris == 0 || n_comp == 0) return HN_OK;        // nothing to launch
    HN_REQUIRE(vertices && triangles && vertex_component && face_component && face_order,
               "hn_meshcc_measure: NULL vertices / triangles / vertex_component / face_component / face_order");
    HN_REQUIRE(faces && vertices_used && area && volume && bounds && workspace, "hn_meshcc_measure: NULL output / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshcc_measure: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshcc_measure: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int *fcnt = (int*)(ws + L.fcnt), *seg = (int*)(ws + L.seg), *chunk = (int*)(ws + L.chunk);
    double* part = (double*)(ws + L.part);
    const int V = (int)n_verts, T = (int)n_tris, C = (int)n_comp, Q = (int)L.max_chunks;
    k_cc_zero<<<grid_of(C + 1), CC_THREADS, 0, s>>>(fcnt, (unsigned long long*)vertices_used, C);
    HN_LAUNCH_CHECK();
    k_cc_count<<<grid_of(V > T ? V : T), CC_THREADS, 0, s>>>(vertex_component, V, face_component, T, C, fcnt, (unsigned long long*)vertices_used);
    HN_LAUNCH_CHECK();
    k_cc_segments<<<1, CC_THREADS, 0, s>>>(fcnt, C, seg, chunk, faces);
    HN_LAUNCH_CHECK();
    if (vertices_f64) {
        k_cc_terms<double><<<(unsigned)Q, CC_THREADS, 0, s>>>((const double*)vertices, n_verts, triangles, T, face_component, face_order, C, seg, chunk, Q, part);
        HN_LAUNCH_CHECK();
        k_cc_sum<double><<<(unsigned)C, CC_THREADS, 0, s>>>(part, chunk, C, Q, area, volume, (double*)bounds);
    } else {
        k_cc_terms<float><<<(unsigned)Q, CC_THREADS, 0, s>>>((const float*)vertices, n_verts, triangles, T, face_component, face_order, C, seg, chunk, Q, part);
        HN_LAUNCH_CHECK();
        k_cc_sum<float><<<(unsigned)C, CC_THREADS, 0, s>>>(part, chunk, C, Q, area, volume, (float*)bounds);
    }
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_meshcc_compact_count(const int* vertex_component, long long n_verts, const int* face_component, long long n_tris, const unsigned char* keep,
                            long long n_comp, long long* totals, void* workspace, size_t workspace_bytes, hn_stream_t stream) {
    CcLayout L;
    HN_TRY_RC(cc_layout(n_verts, n_tris, L));
    HN_REQUIRE(n_comp >= 0 && n_comp < CC_MAX, "hn_meshcc_compact_count: n_comp = %lld outside [0, 2^31 - 256)", n_comp);
    if (n_tris == 0) return HN_OK;                       // nothing to launch: {V', T'} = {0, 0} is the caller's
    HN_REQUIRE(face_component && totals && workspace && (n_verts == 0 || vertex_component) && (n_comp == 0 || keep),
               "hn_meshcc_compact_count: NULL vertex_component / face_component / keep / totals / workspace");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshcc_compact_count: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshcc_compact_count: workspace not 16-byte aligned");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int *blk_v = (int*)(ws + L.blk_v), *off_v = (int*)(ws + L.off_v), *blk_t = (int*)(ws + L.blk_t), *off_t = (int*)(ws + L.off_t);
    k_cc_keep_count<<<(unsigned)(L.nbv + L.nbt), CC_THREADS, 0, s>>>(vertex_component, (int)n_verts, face_component, (int)n_tris, keep, (int)n_comp,
                                                                    (int)L.nbv, blk_v, blk_t);
    HN_LAUNCH_CHECK();
    k_cc_scan<<<1, CC_THREADS, 0, s>>>(blk_v, (int)L.nbv, off_v, totals);
    HN_LAUNCH_CHECK();
    k_cc_scan<<<1, CC_THREADS, 0, s>>>(blk_t, (int)L.nbt, off_t, totals + 1);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

int hn_meshcc_compact_emit(const void* vertices, int vertices_f64, long long n_verts, const long long* triangles, long long n_tris,
                           const int* vertex_component, const int* face_component, const unsigned char* keep, long long n_comp, const void* workspace,
                           size_t workspace_bytes, long long n_verts_out, long long n_tris_out, void* vertices_out, long long* triangles_out,
                           int* vertex_map, int* face_map, hn_stream_t stream) {
    CcLayout L;
    HN_TRY_RC(cc_layout(n_verts, n_tris, L));
    HN_REQUIRE(n_comp >= 0 && n_comp < CC_MAX, "hn_meshcc_compact_emit: n_comp = %lld outside [0, 2^31 - 256)", n_comp);
    HN_REQUIRE(n_verts_out >= 0 && n_verts_out <= n_verts && n_tris_out >= 0 && n_tris_out <= n_tris,
               "hn_meshcc_compact_emit: n_verts_out = %lld, n_tris_out = %lld outside [0, n_verts], [0, n_tris]", n_verts_out, n_tris_out);
    if (n_tris == 0) return HN_OK;
    HN_REQUIRE(triangles && face_component && face_map && workspace && (n_comp == 0 || keep),
               "hn_meshcc_compact_emit: NULL triangles / face_component / face_map / keep / workspace");
    HN_REQUIRE(n_verts == 0 || (vertices && vertex_component && vertex_map), "hn_meshcc_compact_emit: NULL vertices / vertex_component / vertex_map");
    HN_REQUIRE((n_verts_out == 0 || vertices_out) && (n_tris_out == 0 || triangles_out), "hn_meshcc_compact_emit: NULL vertices_out / triangles_out");
    HN_REQUIRE(workspace_bytes >= L.bytes, "hn_meshcc_compact_emit: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    HN_REQUIRE(((uintptr_t)workspace & 15) == 0, "hn_meshcc_compact_emit: workspace not 16-byte aligned");
    const char* ws = (const char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int *off_v = (const int*)(ws + L.off_v), *off_t = (const int*)(ws + L.off_t);
    const int V = (int)n_verts, T = (int)n_tris, C = (int)n_comp;
    if (V > 0) {
        if (vertices_f64)
            k_cc_emit_verts<double><<<(unsigned)L.nbv, CC_THREADS, 0, s>>>((const double*)vertices, V, vertex_component, keep, C, off_v, (int)n_verts_out,
                                                                          (double*)vertices_out, vertex_map);
        else
            k_cc_emit_verts<float><<<(unsigned)L.nbv, CC_THREADS, 0, s>>>((const float*)vertices, V, vertex_component, keep, C, off_v, (int)n_verts_out,
                                                                         (float*)vertices_out, vertex_map);
        HN_LAUNCH_CHECK();
    }
    k_cc_emit_faces<<<(unsigned)L.nbt, CC_THREADS, 0, s>>>(triangles, T, V, face_component, keep, C, off_t, vertex_map, (int)n_tris_out, triangles_out, face_map);
    HN_LAUNCH_CHECK();
    return HN_OK;
}

}  // extern "C"
