"""Cases of the mesh components kernels (ho-nerf_amd/csrc/hn_meshcc.hip) and the rule of DESIGN.md 3.23 in numpy.  A plain module, in
the manner of meshcast_cases: tests/test_meshcc_cpu.py (is the restatement sound?) and tests/test_gpu_meshcc.py (is the device the
restatement?) both import it.

The rule.  Two triangles belong to the same component when they share a vertex index, transitively.  A component's label is the
smallest vertex index its triangles use; vertex_label[v] is that label (-1 for a vertex no triangle uses), face_label[f] the label of
its vertices; components are numbered 0 .. C-1 in ascending label order.  A triangle with an index outside [0, V) joins nothing and
gets -1.  `np_components` is a sequential union-find that links the larger root under the smaller; `bfs_labels` is the independent
check (a breadth-first search over vertex adjacency).  Measures are float64 with math.fsum for the sums (`np_measure`, the exact
side of the summation bound); `np_keep` is the stable filter and re-index.

Meshes come from tests/test_mesh_cpu.py's numpy marching cubes, in index space (fp32) unless a case says otherwise."""
import functools
import math

import numpy as np

from test_mesh_cpu import noise_volume, np_marching_cubes, sphere_volume, torus_volume

BLOBS = ((-0.45, 0.0, 0.0, 0.4), (0.5, 0.1, 0.0, 0.3), (0.0, 0.7, 0.7, 0.12))     # centre, radius on a 24^3 grid over [-1, 1]^3
BLOBS_RES = 24


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def valid_faces(tris, n_verts):
    t = np.asarray(tris).reshape(-1, 3)
    return ((t >= 0) & (t < n_verts)).all(1) if len(t) else np.zeros(0, bool)


def np_components(tris, n_verts):
    """-> dict: n, label [C], vertex_label, vertex_component [V], face_label, face_component [T], all int32 (n an int)."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(t, n_verts)
    parent = list(range(n_verts))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    used = np.zeros(n_verts, bool)
    for a, b, c in t[ok].tolist():
        used[[a, b, c]] = True
        unite(a, b)
        unite(b, c)
    vl = np.full(n_verts, -1, np.int32)
    for v in np.nonzero(used)[0].tolist():
        vl[v] = find(v)
    label = np.unique(vl[vl >= 0]).astype(np.int32)
    rank = np.full(n_verts + 1, -1, np.int32)
    rank[label] = np.arange(len(label), dtype=np.int32)
    fl = np.full(len(t), -1, np.int32)
    fl[ok] = vl[t[ok, 0]]
    return dict(n=len(label), label=label, vertex_label=vl, vertex_component=rank[vl], face_label=fl, face_component=rank[fl])


def bfs_labels(tris, n_verts):
    """vertex_label by a breadth-first search over vertex adjacency, from the smallest unvisited used vertex upward."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    t = t[valid_faces(t, n_verts)]
    adj = [[] for _ in range(n_verts)]
    for a, b, c in t.tolist():
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    vl = np.full(n_verts, -1, np.int32)
    for s in sorted(set(t.reshape(-1).tolist())):
        if vl[s] >= 0:
            continue
        vl[s] = s
        queue = [s]
        while queue:
            nxt = []
            for x in queue:
                for y in adj[x]:
                    if vl[y] < 0:
                        vl[y] = s
                        nxt.append(y)
            queue = nxt
    return vl


def np_is_closed(tris):
    """interaction.is_closed's rule: every directed edge used by exactly one face, its reverse by exactly one other."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return False
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(t.max()) + 1
    code, rev = d[:, 0] * n + d[:, 1], d[:, 1] * n + d[:, 0]
    u, cnt = np.unique(code, return_counts=True)
    return bool((cnt == 1).all() and np.isin(rev, u).all())


def face_terms(verts, tris):
    """(area terms, volume terms) float64 [T]: 0.5 sqrt((nx nx + ny ny) + nz nz) with n = (b - a) x (c - a), and
    ((a0 x0 + a1 x1) + a2 x2) / 6 with x = b x c -- the kernel's expressions, every operation rounded once."""
    v = np.asarray(verts).astype(np.float64)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    x0 = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    x1 = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    x2 = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    vol = ((a[:, 0] * x0 + a[:, 1] * x1) + a[:, 2] * x2) / 6.0
    return area, vol


def np_measure(verts, tris, comps=None):
    """Per component -> dict: faces, vertices int64; area, volume float64 (math.fsum of the face terms: the exact sums, rounded once);
    area_abs, volume_abs (fsum of |term|, what the summation bound is relative to); bounds [C, 6] in verts' dtype; closed bool."""
    verts = np.asarray(verts)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    comps = comps or np_components(t, len(verts))
    C = comps['n']
    fc, vc = comps['face_component'], comps['vertex_component']
    at, vt = face_terms(verts, t[fc >= 0]) if len(t) else (np.zeros(0), np.zeros(0))
    fcv = fc[fc >= 0]
    out = dict(faces=np.bincount(fcv, minlength=C).astype(np.int64), vertices=np.bincount(vc[vc >= 0], minlength=C).astype(np.int64),
               area=np.zeros(C), volume=np.zeros(C), area_abs=np.zeros(C), volume_abs=np.zeros(C), bounds=np.zeros((C, 6), verts.dtype),
               closed=np.zeros(C, bool))
    for c in range(C):
        sel = fcv == c
        out['area'][c], out['volume'][c] = math.fsum(at[sel]), math.fsum(vt[sel])
        out['area_abs'][c], out['volume_abs'][c] = math.fsum(np.abs(at[sel])), math.fsum(np.abs(vt[sel]))
        used = verts[vc == c]
        out['bounds'][c] = np.concatenate([used.min(0), used.max(0)])
        out['closed'][c] = np_is_closed(t[fc == c])
    return out


def np_select(meas, largest=None, min_faces=None, min_area_fraction=None, closed_only=False, mask=None):
    """The keep mask over components: the criteria combine with AND; largest = the k components with the most faces, ties to the
    smaller label."""
    C = len(meas['faces'])
    sel = np.ones(C, bool)
    if mask is not None:
        sel &= np.asarray(mask, bool)
    if largest is not None:
        top = np.argsort(-meas['faces'], kind='stable')[:largest]
        pick = np.zeros(C, bool)
        pick[top] = True
        sel &= pick
    if min_faces is not None:
        sel &= meas['faces'] >= min_faces
    if min_area_fraction is not None:
        sel &= meas['area'] >= min_area_fraction * meas['area'].sum()
    if closed_only:
        sel &= meas['closed']
    return sel


def np_keep(verts, tris, sel, comps=None):
    """Stable filter and re-index -> (vertices', triangles' int64, vertex_map int32 [V], face_map int32 [T], kept int64)."""
    verts = np.asarray(verts)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    comps = comps or np_components(t, len(verts))
    sel = np.asarray(sel, bool)
    pad = np.concatenate([sel, [False]])                 # component -1 -> not kept
    kv, kf = pad[comps['vertex_component']], pad[comps['face_component']]
    vmap = np.full(len(verts), -1, np.int32)
    vmap[kv] = np.arange(int(kv.sum()), dtype=np.int32)
    fmap = np.full(len(t), -1, np.int32)
    fmap[kf] = np.arange(int(kf.sum()), dtype=np.int32)
    return verts[kv].copy(), vmap[t[kf]].astype(np.int64).reshape(-1, 3), vmap, fmap, np.nonzero(sel)[0].astype(np.int64)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def blob_volume(blobs=BLOBS, res=BLOBS_RES):
    ax = np.linspace(-1.0, 1.0, res)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    d = [np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r for cx, cy, cz, r in blobs]
    return np.minimum.reduce(d).astype(np.float32)


def blob_world(v, res=BLOBS_RES):
    """Index space -> [-1, 1]^3, float64."""
    return v.astype(np.float64) * (2.0 / (res - 1)) - 1.0


def sphere_mesh(center, r, res, v_dtype=np.float32):
    """A marching-cubes sphere in world units in a box of 1.25 r around its centre."""
    c = np.asarray(center, np.float64)
    ax = [np.linspace(c[i] - 1.25 * r, c[i] + 1.25 * r, res) for i in range(3)]
    x, y, z = np.meshgrid(*ax, indexing='ij')
    v, t = np_marching_cubes((np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32), 0.0)
    return (v.astype(np.float64) * (2.5 * r / (res - 1.0)) + (c - 1.25 * r)[None]).astype(v_dtype), t


def concat(*meshes):
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def strip(n=4096, seed=3):
    """n triangles in one chain (i, i + 1, i + 2), the vertex ids randomly permuted: deep trees, long find walks, links in adversarial
    order."""
    rs = np.random.RandomState(seed)
    perm = rs.permutation(n + 2)
    i = np.arange(n)
    t = perm[np.stack([i, i + 1, i + 2], 1)].astype(np.int64)
    return rs.rand(n + 2, 3).astype(np.float32), t


def fan(n=4096, hub_high=True, seed=4):
    """n triangles that all share one vertex: the highest index (every union starts at the same node) or index 0."""
    rs = np.random.RandomState(seed)
    V = n + 2
    hub = V - 1 if hub_high else 0
    rim = np.arange(n + 1) + (0 if hub_high else 1)
    t = np.stack([np.full(n, hub), rim[:-1], rim[1:]], 1).astype(np.int64)
    return rs.rand(V, 3).astype(np.float32), t


def pinch():
    """Two tetrahedra sharing vertex 0 and no edge."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [0, 4, 5], [0, 6, 4], [0, 5, 6], [4, 6, 5]], np.int64)
    return v, t


def soup(n, gaps=False, extras=False, seed=6):
    """n disjoint triangles over 3 n vertices.  gaps: 5 unreferenced vertices interleaved.  extras: one degenerate (a, a, b) face and
    one duplicated face appended."""
    rs = np.random.RandomState(seed)
    ids = np.arange(3 * n)
    if gaps:
        holes = np.array([0, 7, 3 * n // 2, 3 * n - 2, 3 * n + 4])       # positions, in the final numbering, that nothing uses
        ids = np.setdiff1d(np.arange(3 * n + 5), holes)
    t = ids.reshape(n, 3).astype(np.int64)
    if extras:
        t = np.concatenate([t, [[t[5, 0], t[5, 0], t[9, 1]]], t[11:12]])
    return rs.rand(3 * n + (5 if gaps else 0), 3).astype(np.float32), t


def floater_in_object():
    """-> (hand mesh, object mesh, hand without its floater): a hand sphere, an object sphere disjoint from it, and a small sphere that
    belongs to the HAND mesh and sits inside the object.  float64 world metres."""
    big = sphere_mesh((0.0, 0.0, 0.9), 0.05, 14, np.float64)
    floater = sphere_mesh((0.2, 0.0, 0.9), 0.012, 7, np.float64)
    obj = sphere_mesh((0.2, 0.0, 0.9), 0.06, 14, np.float64)
    return concat(big, floater), obj, big


NAMES = ('blobs24', 'noise', 'sphere20', 'torus24', 'strip', 'fan_high', 'fan_low', 'pinch', 'soup255', 'soup256', 'soup257', 'soup_gaps',
         'soup_extras', 'empty', 'empty_v0', 'single', 'floater')


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (vertices [V, 3] float32 (float64 for 'floater'), triangles int64 [T, 3])."""
    if name == 'blobs24':
        return np_marching_cubes(blob_volume())
    if name == 'noise':
        return np_marching_cubes(noise_volume())
    if name == 'sphere20':
        return np_marching_cubes(sphere_volume(20))
    if name == 'torus24':
        return np_marching_cubes(torus_volume(24))
    if name == 'strip':
        return strip()
    if name in ('fan_high', 'fan_low'):
        return fan(hub_high=name == 'fan_high')
    if name == 'pinch':
        return pinch()
    if name in ('soup255', 'soup256', 'soup257'):
        return soup(int(name[4:]))
    if name == 'soup_gaps':
        return soup(257, gaps=True)
    if name == 'soup_extras':
        return soup(257, gaps=True, extras=True)
    if name == 'empty':
        return np.random.RandomState(1).rand(5, 3).astype(np.float32), np.zeros((0, 3), np.int64)
    if name == 'empty_v0':
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    if name == 'single':
        return np.random.RandomState(2).rand(4, 3).astype(np.float32), np.array([[3, 0, 2]], np.int64)
    if name == 'floater':
        return floater_in_object()[0]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def comps(name):
    v, t = mesh(name)
    return np_components(t, len(v))


@functools.lru_cache(maxsize=None)
def measures(name):
    v, t = mesh(name)
    return np_measure(v, t, comps(name))
