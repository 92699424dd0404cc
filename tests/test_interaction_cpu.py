"""CPU checks of the hand-object interaction metrics (hn_interact.hip, honerf_amd.interaction): a float64 numpy restatement of the
contract of DESIGN.md 3.14 (trimesh's voxelized / contains / closest_point as analys_interaction.py calls them), checked on its own
against analytic answers; the metrics it gives on two marching-cubes spheres; pci; and the C ABI.  tests/test_interaction.py holds
the device to this restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_mesh_cpu import np_marching_cubes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROUNDS = 10          # this project's cap: 10 rounds of splitting allowed, an 11th refused; trimesh may refuse at 10


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def np_subdivide(tri, pitch):
    """tri [T, 3, 3] float64 -> (leaf triangles [L, 3, 3], rounds used).  A triangle with an edge length sqrt((dx^2 + dy^2) + dz^2)
    > pitch / 2 is split 4-way at (a + b) / 2; each child is judged again; ValueError when round MAX_ROUNDS + 1 would be needed."""
    max_edge = pitch / 2.0
    cur = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    done = []
    for r in range(MAX_ROUNDS + 1):
        d = cur[:, [1, 2, 0]] - cur
        length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        long_ = (length > max_edge).any(axis=1)
        done.append(cur[~long_])
        if not long_.any():
            return np.concatenate(done), r
        if r == MAX_ROUNDS:
            raise ValueError('a triangle needs more than %d rounds of splitting' % MAX_ROUNDS)
        t = cur[long_]
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        m01, m12, m20 = (a + b) / 2.0, (b + c) / 2.0, (c + a) / 2.0
        cur = np.concatenate([np.stack(x, 1) for x in ((a, m01, m20), (m01, b, m12), (m20, m12, c), (m01, m12, m20))])
    raise AssertionError('unreachable')


def np_voxel_keys(verts, tris, pitch):
    """Trimesh.voxelized(pitch): the integer keys k = rint(v / pitch) of every leaf vertex, unique, sorted (x, y, z) -> int64 [N, 3]."""
    leaves, _ = np_subdivide(np.asarray(verts, np.float64)[np.asarray(tris)], pitch)
    if len(leaves) == 0:
        return np.zeros((0, 3), np.int64)
    return np.unique(np.rint(leaves.reshape(-1, 3) / pitch).astype(np.int64), axis=0)


def np_winding(verts, tris, pts, chunk=1 << 21):
    """Generalized winding number (float64): sum over the triangles of atan2(det, den) / (2 pi) (half the Van Oosterom-Strackee
    solid angle over 2 pi); 0 for points outside the mesh's bounds (not evaluated)."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris)
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    w = np.zeros(len(p))
    if len(t) == 0 or len(p) == 0:
        return w
    lo, hi = v.min(0), v.max(0)
    live = np.nonzero(((p >= lo) & (p <= hi)).all(1))[0]
    a, b, c = (v[t[:, k]].T.copy() for k in range(3))        # [3, T]: one row per axis
    step = max(1, chunk // len(t))
    for s in range(0, len(live), step):
        idx = live[s:s + step]
        q = p[idx]
        ax, ay, az = (a[k][None] - q[:, k:k + 1] for k in range(3))
        bx, by, bz = (b[k][None] - q[:, k:k + 1] for k in range(3))
        cx, cy, cz = (c[k][None] - q[:, k:k + 1] for k in range(3))
        la, lb, lc = np.sqrt(ax * ax + ay * ay + az * az), np.sqrt(bx * bx + by * by + bz * bz), np.sqrt(cx * cx + cy * cy + cz * cz)
        det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
        den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb
        w[idx] = np.arctan2(det, den).sum(1) / (2 * np.pi)
    return w


def np_contains(verts, tris, pts):
    return np.abs(np_winding(verts, tris, pts)) > 0.5


def np_distance(verts, tris, pts, chunk=1 << 20):
    """Unsigned distance to the nearest triangle (float64): Ericson's closest point on a triangle, region by region."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris)
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.full(len(p), np.inf)
    if len(t) == 0:
        return out
    a = v[t[:, 0]].T.copy()
    ab, ac = (v[t[:, 1]] - v[t[:, 0]]).T.copy(), (v[t[:, 2]] - v[t[:, 0]]).T.copy()
    step = max(1, chunk // len(t))
    for s in range(0, len(p), step):
        q = p[s:s + step]
        ap = [q[:, k:k + 1] - a[k][None] for k in range(3)]                 # p - a; p - b = ap - ab, p - c = ap - ac
        dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
        abq, acq = [ab[k][None] for k in range(3)], [ac[k][None] for k in range(3)]
        bp = [ap[k] - abq[k] for k in range(3)]
        cp = [ap[k] - acq[k] for k in range(3)]
        d1, d2, d3, d4, d5, d6 = dot(abq, ap), dot(acq, ap), dot(abq, bp), dot(acq, bp), dot(abq, cp), dot(acq, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(divide='ignore', invalid='ignore'):
            den = va + vb + vc
            fv, fw = vb / den, vc / den
            e43, e56 = d4 - d3, d5 - d6
            conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                     (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
            bw = e43 / (e43 + e56)
            vv = np.select(conds, [0.0, 1.0, d1 / (d1 - d3), 0.0, 0.0, 1.0 - bw], fv)
            ww = np.select(conds, [0.0, 0.0, 0.0, 1.0, d2 / (d2 - d6), bw], fw)
        r = [ap[k] - abq[k] * vv - acq[k] * ww for k in range(3)]            # p - (a + ab v + ac w)
        out[s:s + step] = np.nanmin(np.sqrt(dot(r, r)), axis=1)
    return out


def np_solid_points(obj, hand, pitch):
    """The lattice points k * pitch in the overlap of the two meshes' bounds (intersection_volume(..., solid=True))."""
    lo = np.maximum(obj[0].min(0), hand[0].min(0))
    hi = np.minimum(obj[0].max(0), hand[0].max(0))
    klo, khi = np.ceil(lo / pitch).astype(np.int64), np.floor(hi / pitch).astype(np.int64)
    if (khi < klo).any():
        return np.zeros((0, 3))
    ax = [np.arange(klo[i], khi[i] + 1, dtype=np.float64) * pitch for i in range(3)]
    return np.stack([x.reshape(-1) for x in np.meshgrid(*ax, indexing='ij')], 1)


def np_metrics(hand, obj, pitch=0.005):
    """interaction_metrics' numbers: int_vol (cm^3, the shell count of the reference) and pen_dep (mm), with the counts."""
    keys = np_voxel_keys(obj[0], obj[1], pitch)
    inside = np_contains(hand[0], hand[1], keys * pitch)
    n_in = int(inside.sum())
    hin = np_contains(obj[0], obj[1], hand[0])
    pen = float(np_distance(obj[0], obj[1], hand[0][hin]).max()) if hin.any() else 0.0
    return dict(int_vol=n_in * pitch ** 3 * 1e6, pen_dep=pen * 1000.0, n_obj_voxels=len(keys), n_obj_voxels_inside=n_in,
                n_hand_verts_inside=int(hin.sum()))


def np_solid_volume(obj, hand, pitch):
    pts = np_solid_points(obj, hand, pitch)
    in_hand = np_contains(hand[0], hand[1], pts)
    return int(np_contains(obj[0], obj[1], pts[in_hand]).sum()) * pitch ** 3


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def mc_sphere(center, r, res, margin=1.15):
    """A marching-cubes sphere in world metres: (vertices float64 [V, 3], triangles int64 [T, 3], grid spacing)."""
    c = np.asarray(center, np.float64)
    bmin, bmax = c - margin * r, c + margin * r
    ax = [np.linspace(bmin[i], bmax[i], res) for i in range(3)]
    x, y, z = np.meshgrid(*ax, indexing='ij')
    vol = (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)
    v, t = np_marching_cubes(vol, 0.0)
    h = (bmax - bmin) / (res - 1.0)
    return v.astype(np.float64) * h[None] + bmin[None], t, float(h.max())


def lens_volume(R, r, d):
    return np.pi * (R + r - d) ** 2 * (d * d + 2 * d * r - 3 * r * r + 2 * d * R + 6 * r * R - 3 * R * R) / (12 * d)


# ---- contract 1: voxelization -------------------------------------------------------------------------------------------------
def test_lone_triangle_splits_four_rounds():
    p = 0.005
    tri = np.array([[[0.0, 0.0, 0.0], [4 * p, 0.0, 0.0], [0.0, 4 * p, 0.0]]])
    leaves, rounds = np_subdivide(tri, p)
    assert rounds == 4 and len(leaves) == 4 ** 4
    assert len(np.unique(leaves.reshape(-1, 3), axis=0)) == 17 * 18 // 2
    keys = np_voxel_keys(tri[0], np.array([[0, 1, 2]]), p)
    assert len(keys) > 0 and keys.min() >= 0 and keys.max() <= 4


def test_too_large_triangle_is_refused():
    tri = np.array([[[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]]])    # 13 rounds at a 5 mm pitch
    with pytest.raises(ValueError):
        np_subdivide(tri, 0.005)


def test_round_cap_boundary():
    """Legs of 300 pitches need exactly 10 rounds (allowed); 400 pitches need 11 (refused)."""
    p = 0.005
    leaves, rounds = np_subdivide(np.array([[[0.0, 0, 0], [300 * p, 0, 0], [0, 300 * p, 0]]]), p)
    assert rounds == 10 and len(leaves) == 4 ** 10
    with pytest.raises(ValueError):
        np_subdivide(np.array([[[0.0, 0, 0], [400 * p, 0, 0], [0, 400 * p, 0]]]), p)


def test_sphere_shell_hugs_the_mesh():
    p = 0.005
    v, t, h = mc_sphere((0.01, -0.02, 0.9), 0.05, 24)
    keys = np_voxel_keys(v, t, p)
    pts = keys * p
    d = np_distance(v, t, pts)
    assert d.max() <= p * np.sqrt(3) / 2 + 1e-12, d.max()
    own = {tuple(k) for k in np.rint(v / p).astype(np.int64)}
    assert own <= {tuple(k) for k in keys}
    # a hollow shell: the centre is not a voxel point
    assert tuple(np.rint(np.array([0.01, -0.02, 0.9]) / p).astype(np.int64)) not in {tuple(k) for k in keys}


# ---- contracts 2 and 3: containment and distance ------------------------------------------------------------------------------
def test_containment_on_a_sphere_and_flipped():
    r = 0.05
    v, t, h = mc_sphere((0.0, 0.0, 0.0), r, 24)
    rng = np.random.RandomState(3)
    pts = rng.uniform(-1.3 * r, 1.3 * r, size=(3000, 3))
    rad = np.linalg.norm(pts, axis=1)
    far = np.abs(rad - r) >= 2 * h
    inside = np_contains(v, t, pts)
    assert far.sum() > 1500
    assert np.array_equal(inside[far], rad[far] < r)
    assert np.array_equal(np_contains(v, t[:, ::-1], pts), inside)
    w = np_winding(v, t, pts[far])
    assert np.abs(np.abs(w) - (rad[far] < r)).max() < 1e-9


def test_distance_on_a_sphere_and_against_dense_sampling():
    r = 0.05
    v, t, h = mc_sphere((0.0, 0.0, 0.0), r, 24)
    rng = np.random.RandomState(4)
    pts = rng.uniform(-1.5 * r, 1.5 * r, size=(800, 3))
    d = np_distance(v, t, pts)
    assert np.abs(d - np.abs(np.linalg.norm(pts, axis=1) - r)).max() <= h
    # dense barycentric samples of every triangle: the exact distance is never above them and within their spacing of them
    n = 24
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    keep = i + j <= n
    u, w = i[keep] / n, j[keep] / n
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    samples = (a[:, None] + (b - a)[:, None] * u[None, :, None] + (c - a)[:, None] * w[None, :, None]).reshape(-1, 3)
    edge = np.linalg.norm(np.concatenate([b - a, c - b, a - c]), axis=1).max()
    for q in pts[:6]:
        dense = np.sqrt(((samples - q) ** 2).sum(1)).min()
        e = np_distance(v, t, q[None])[0]
        assert e <= dense + 1e-12 and dense - e <= edge / n


# ---- the metrics on two spheres -----------------------------------------------------------------------------------------------
R_HAND, R_OBJ = 0.05, 0.06


def _pair(d, res=24):
    hand = mc_sphere((0.0, 0.0, 0.0), R_HAND, res)
    obj = mc_sphere((d, 0.0, 0.0), R_OBJ, res)
    return hand, obj


def test_disjoint_spheres_give_zero():
    (hv, ht, _), (ov, ot, _) = _pair(0.2)
    m = np_metrics((hv, ht), (ov, ot))
    assert m['int_vol'] == 0 and m['pen_dep'] == 0 and m['n_hand_verts_inside'] == 0 and m['n_obj_voxels'] > 0


def test_overlapping_spheres_penetration_and_shell():
    d = 0.08
    (hv, ht, hh), (ov, ot, ho) = _pair(d)
    m = np_metrics((hv, ht), (ov, ot))
    assert m['n_hand_verts_inside'] > 0
    assert abs(m['pen_dep'] / 1000.0 - (R_HAND + R_OBJ - d)) <= max(hh, ho)
    assert 0 < m['n_obj_voxels_inside'] < m['n_obj_voxels']
    assert 0 < m['int_vol'] <= m['n_obj_voxels'] * 0.005 ** 3 * 1e6


def test_solid_volume_approaches_the_lens():
    """solid=True against the lens volume of the two true spheres.  The bound is derived here, at the chosen pitch: the lattice
    count of the TRUE lens (analytic inside test) gives the lattice error, and the meshes' largest inward gap from their spheres
    times the lens's surface gives what the marching-cubes facets can move."""
    d, pitch = 0.08, 0.0035
    (hv, ht, _), (ov, ot, _) = _pair(d, res=28)
    exact = lens_volume(R_OBJ, R_HAND, d)
    pts = np_solid_points((ov, ot), (hv, ht), pitch)
    true_count = ((np.linalg.norm(pts, axis=1) < R_HAND) & (np.linalg.norm(pts - [d, 0, 0], axis=1) < R_OBJ)).sum()
    e_lattice = abs(true_count * pitch ** 3 - exact) / exact

    def gap(v, t, c, r):      # deepest point of a facet below the sphere: its centroid bounds it from below, the vertices from above
        cen = v[t].mean(1)
        return max(r - np.linalg.norm(cen - c, axis=1).min(), np.abs(np.linalg.norm(v - c, axis=1) - r).max())
    delta = max(gap(hv, ht, np.zeros(3), R_HAND), gap(ov, ot, np.array([d, 0, 0]), R_OBJ))
    a = (d * d + R_OBJ ** 2 - R_HAND ** 2) / (2 * d)
    area = 2 * np.pi * R_OBJ * (R_OBJ - a) + 2 * np.pi * R_HAND * (R_HAND - (d - a))
    bound = e_lattice + 1.5 * area * delta / exact
    assert bound <= 0.05, bound
    got = np_solid_volume((ov, ot), (hv, ht), pitch)
    assert abs(got - exact) / exact <= bound, (got, exact, bound)


def test_lens_formula():
    assert abs(lens_volume(0.06, 0.05, 0.08) * 1e6 - 69.8) < 0.1
    # a limiting case: d = R - r, the small ball inside the large one
    assert abs(lens_volume(0.06, 0.05, 0.01 + 1e-12) - 4 / 3 * np.pi * 0.05 ** 3) < 1e-9


# ---- pci and the closed-mesh check --------------------------------------------------------------------------------------------
def test_pci():
    from honerf_amd.interaction import pci
    assert pci([1, 2, 3, 4], [3, 4, 5, 6]) == pytest.approx(2 / 6, rel=1e-6)
    assert pci(np.array([5, 5, 7]), np.array([7, 5])) == pytest.approx(1.0, rel=1e-6)
    assert pci([], []) == 0.0
    assert pci([1, 2], []) == 0.0


def test_is_closed():
    import torch
    from honerf_amd.interaction import is_closed
    _, t, _ = mc_sphere((0.0, 0.0, 0.0), 0.05, 16)
    assert is_closed(torch.from_numpy(t))
    assert not is_closed(torch.from_numpy(t[1:]))                    # a hole
    flip = t.copy()
    flip[0] = flip[0, ::-1]
    assert not is_closed(torch.from_numpy(flip))                     # one face against its neighbours
    assert not is_closed(torch.zeros(0, 3, dtype=torch.long))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
NAMES = {'hn_voxelize_workspace_bytes', 'hn_voxelize_count', 'hn_voxelize_emit', 'hn_interact_workspace_bytes', 'hn_winding_contains',
         'hn_closest_distance'}


def test_header_and_library_carry_the_interaction_entry_points():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'honerf.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(hn_(?:voxelize|interact|winding|closest)[a-z0-9_]*)\s*\(', src))
    assert names == NAMES, names
    from honerf_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(cdll, n), n
        assert n in lib.SIGNATURES, n
    assert lib.HN_VERSION == 121
    L = lib.load()
    assert L.hn_voxelize_workspace_bytes(1000) >= 1000 * 4
    assert L.hn_voxelize_workspace_bytes(0) > 0
    assert L.hn_voxelize_workspace_bytes(-1) == 0
    assert L.hn_voxelize_workspace_bytes(1 << 31) == 0
    assert L.hn_interact_workspace_bytes(5000, 70000) >= 5000 * 4
    assert L.hn_interact_workspace_bytes(0, 0) > 0
    assert L.hn_interact_workspace_bytes(-1, 10) == 0
    assert L.hn_interact_workspace_bytes(10, -1) == 0
    assert L.hn_interact_workspace_bytes(1 << 31, 10) == 0
    assert L.hn_interact_workspace_bytes(10, 1 << 31) == 0


def test_interaction_source_has_no_scalar_memory_writes():
    src = open(os.path.join(ROOT, 'ho-nerf_amd', 'csrc', 'hn_interact.hip')).read().lower()
    for w in ('s_' + 'store', 's_' + 'buffer', 's_' + 'scratch', 's_' + 'atomic', 's_' + 'dcache'):
        assert w not in src, w


def test_module_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, 'ho-nerf_amd', 'interaction.py')).read()
    assert 'oracle' not in re.sub(r'""".*?"""', '', src, flags=re.S)
