"""The numpy restatement of the mesh distance contract (tests/mesh_distance_cases.py) against shapes whose answers are
known in closed form, and the choice of the GPU tests' sampler inputs.  No GPU."""
import numpy as np
import pytest

import mesh_distance_cases as C


# ---- point-triangle distance ---------------------------------------------------------------------------------------------------------
TRI = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32), np.array([[0, 1, 2]], np.int64))
# query (x, y), the closest point in the plane: one per region of the triangle (0,0) (1,0) (0,1), computed by hand
REGIONS = {'face': ((0.25, 0.25), (0.25, 0.25)), 'vertex A': ((-1.0, -1.0), (0.0, 0.0)), 'vertex B': ((2.0, -0.5), (1.0, 0.0)),
           'vertex C': ((-0.5, 2.0), (0.0, 1.0)), 'edge AB': ((0.5, -1.0), (0.5, 0.0)), 'edge AC': ((-1.0, 0.5), (0.0, 0.5)),
           'edge BC': ((1.0, 1.0), (0.5, 0.5))}


@pytest.mark.parametrize('z', [0.0, 0.3, -2.0])
def test_one_triangle_in_each_of_the_seven_regions(z):
    for name, ((x, y), (qx, qy)) in REGIONS.items():
        d, f, q = C.np_closest(*TRI, np.array([[x, y, z]]))
        want = np.sqrt((x - qx) ** 2 + (y - qy) ** 2 + z * z)
        assert abs(d[0] - want) < 1e-12 and f[0] == 0, (name, d[0], want)
        assert np.abs(q[0] - np.array([qx, qy, 0.0])).max() < 1e-12, (name, q[0])
        d1, q1 = C.np_tri_closest(*TRI, np.array([[x, y, z]]), [0])
        assert d1[0] == d[0] and np.array_equal(q1[0], q[0])


def test_degenerate_triangles_have_a_distance():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]], np.float32)
    for tri, p, want in (((0, 1, 2), (1.5, 1.0, 0.0), 1.0), ((0, 1, 2), (3.0, 0.0, 4.0), np.sqrt(17.0)), ((0, 2, 2), (0.5, -2.0, 0.0), 2.0),
                         ((1, 1, 1), (1.0, 3.0, 4.0), 5.0)):
        d, f, _ = C.np_closest(v, np.array([tri], np.int64), np.array([p]))
        assert abs(d[0] - want) < 1e-12 and f[0] == 0, (tri, p, d[0])
    vn = v.copy()
    vn[1, 1] = np.nan
    d, f, q = C.np_closest(vn, np.array([[0, 1, 2]], np.int64), np.array([[0.0, 1.0, 0.0]]))
    assert np.isinf(d[0]) and f[0] == -1 and not q.any()


def test_uv_sphere_distances():
    r = 0.3
    v, t = C.uv_sphere(r)
    s = C.sagitta(v, t, r)
    assert 0 < s < 0.05 * r * 2
    u = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    for rho in (1.5 * r, 1.01 * r, 3.0 * r):              # outside, along a vertex direction: the vertex itself is nearest
        d, _, q = C.np_closest(v, t, rho * u)
        assert np.abs(d - (rho - r)).max() < 1e-6
        assert np.abs(q - v.astype(np.float64)).max() < 1e-6
    rs = np.random.RandomState(0)
    w = rs.standard_normal((400, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    for rho in (0.2 * r, 0.8 * r, 1.2 * r, 2.5 * r):      # any direction, and inside: within the facets' sagitta
        for dirs in (u, w):
            d, _, _ = C.np_closest(v, t, rho * dirs)
            assert (np.abs(d - abs(rho - r)) <= s + 1e-6).all(), (rho, np.abs(d - abs(rho - r)).max(), s)
    d, f, _ = C.np_closest(v, t, np.zeros((1, 3)))
    assert abs(d[0] - (r - s)) < 1e-6                     # the centre: the nearest facet's plane


def test_smallest_face_among_equal_distances():
    v, t = C.uv_sphere(0.3)
    q = C.query_set(v, t, 'random', 200)
    d1, f1, _ = C.np_closest(v, np.concatenate([t, t]), q)
    d0, f0, _ = C.np_closest(v, t, q)
    assert np.array_equal(d0, d1) and np.array_equal(f0, f1) and (f1 < len(t)).all()


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------
def _metrics(pred, gt, n, seed=0, taus=(0.005, 0.010)):
    pp, _, pn = C.np_sample(*pred, n, seed)
    gp, _, gn = C.np_sample(*gt, n, seed + 1)
    return C.np_surface_metrics(pred, gt, pp, pn, gp, gn, taus)


def test_a_mesh_against_itself():
    m = C.uv_sphere(0.05)
    r = _metrics(m, m, 500)
    assert r['chamfer_l1'] < 1e-12 and r['chamfer_l2'] < 1e-24 and r['hausdorff'] < 1e-12
    assert r['precision@0.005'] == r['recall@0.005'] == r['fscore@0.005'] == 1.0
    assert r['normal_consistency'] > 0.99 and r['n'] == 500 and r['pred_area'] == r['gt_area']
    assert abs(r['pred_area'] - 4 * np.pi * 0.05 ** 2) < 0.05 * 4 * np.pi * 0.05 ** 2


def test_concentric_spheres():
    r1, r2 = 0.05, 0.06
    a, b = C.uv_sphere(r1, 24, 32), C.uv_sphere(r2, 24, 32)
    s = max(C.sagitta(*a, r1), C.sagitta(*b, r2))
    gap = r2 - r1
    assert s < 0.1 * gap
    lo, hi = 0.8 * gap, 1.2 * gap
    assert lo < gap - s and hi > gap + s
    r = _metrics(a, b, 800, taus=(lo, hi))
    assert abs(r['accuracy'] - gap) <= s + 1e-7 and abs(r['completeness'] - gap) <= s + 1e-7
    assert abs(r['chamfer_l1'] - gap) <= s + 1e-7 and abs(r['hausdorff'] - gap) <= s + 1e-7
    assert r['fscore@%g' % lo] == 0.0 and r['precision@%g' % lo] == 0.0 and r['recall@%g' % lo] == 0.0
    assert r['fscore@%g' % hi] == 1.0
    assert r['normal_consistency'] > 0.98


# ---- sampler ---------------------------------------------------------------------------------------------------------------------------
def test_the_hash_is_pinned():
    # splitmix64's published outputs for the state 0, then counters written out here
    assert [C.mix64((j + 1) * C.GAMMA) for j in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert C.draws24(0, 0) == (14819496, 7239838, 443485)
    assert C.draws24(0, 1) == (9505325, 12512141, 16290722)
    assert C.draws24(1, 0) == (12856410, 3648863, 11491223)
    assert C.draws24(7, 4098) == (11630154, 12443409, 4160184)
    assert C.draws24(4294967295, 2147483582) == (15066360, 14976917, 15709406)
    r = C.draws(7, 4099)
    assert np.array_equal(r[4098] * 16777216.0 - 0.5, np.array([11630154.0, 12443409.0, 4160184.0]))
    assert np.array_equal(C.draws(0, 2)[1] * 16777216.0 - 0.5, np.array([9505325.0, 12512141.0, 16290722.0]))
    assert (r > 0).all() and (r < 1).all()


@pytest.mark.parametrize('name, n', [('torus24', 20000), ('sphere16+flat', 5000), ('one', 17)])
def test_stratified_counts_per_face(name, n):
    """Sample i lies in stratum [i, i + 1) / n of the cumulative area, so a face that spans L = n A_t / A strata holds every stratum
    that lies wholly inside it (more than L - 2 of them) and at most the two it shares with its neighbours: floor(L) - 1 <= count <=
    ceil(L) + 1, whatever the draws.  No statistical bound."""
    v, t = C.sampler_mesh(name)
    pts, f, nrm = C.np_sample(v, t, n, 5)
    area, _ = C.np_face_areas(v, t)
    L = n * area / area.sum()
    cnt = np.bincount(f, minlength=len(t))
    assert cnt.sum() == n
    assert (cnt >= np.maximum(np.floor(L) - 1, 0)).all() and (cnt <= np.ceil(L) + 1).all()
    assert (cnt[area == 0] == 0).all()
    whole = L >= 2                                        # faces hit by at least one whole stratum
    if whole.any():
        assert (np.abs(cnt[whole] - L[whole]) < 2).all()
    assert (np.diff(f) >= 0).all()                        # stratified: the faces come in order


def test_samples_lie_in_their_triangles():
    v, t = C.sampler_mesh('torus24')
    pts, f, nrm = C.np_sample(v, t, 3000, 2)
    r = C.draws(2, 3000)
    s = np.sqrt(r[:, 1])
    for w in (1 - s, s * (1 - r[:, 2]), s * r[:, 2]):
        assert (w >= 0).all() and (w <= 1).all()
    d, q = C.np_tri_closest(v, t, pts, f)
    assert d.max() < 1e-12
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-12
    again = C.np_sample(v, t, 3000, 2)
    assert all(np.array_equal(x, y) for x, y in zip((pts, f, nrm), again))
    other = C.np_sample(v, t, 3000, 3)
    assert not np.array_equal(other[0], pts)


@pytest.mark.parametrize('name, n, seed', C.SAMPLER_CASES)
def test_no_sampler_case_of_the_gpu_tests_sits_on_a_knot(name, n, seed):
    """A sample within 1e-9 A_total of a cumulative-area knot may land in the neighbouring triangle when the cumulative sum is made in
    another order (the device's scan).  The GPU tests' inputs are chosen with none."""
    v, t = C.sampler_mesh(name)
    assert int(C.knot_gap(v, t, n, seed).sum()) == 0


def test_mesh_counts_and_query_sets():
    for T in C.T_EDGES:
        v, t = C.mesh_T(T)
        assert len(t) == T and t.max() < len(v)
    v, t = C.mesh_T(65)
    for kind in C.QUERY_KINDS:
        for n in (1, 257):
            q = C.query_set(v, t, kind, n)
            assert q.shape == (n, 3) and q.dtype == np.float32 and np.isfinite(q).all()
    d, _, _ = C.np_closest(v, t, C.query_set(v, t, 'surface', 300))
    assert d.max() < 1e-6
    d, _, _ = C.np_closest(v, t, C.query_set(v, t, 'far', 5))
    assert d.min() > 99.0


# ---- the build -----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_queries_and_one_point_triangle_header():
    import os
    from honerf_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = lib.load()
    for name in ('hn_meshdist_workspace_bytes', 'hn_meshdist_prepare', 'hn_meshdist_closest', 'hn_mesh_face_areas', 'hn_mesh_sample'):
        assert hasattr(L, name) and name in lib.SIGNATURES
    assert L.hn_meshdist_workspace_bytes(0) == 256
    # the layout: 64 slots of three float4 per block, a box per block, a box per group, then prepare's scratch
    al = lambda x: (x + 255) & ~255
    for T in (1, 64, 65, 2049):
        nb = (T + 63) // 64
        ng = (nb + 31) // 32
        assert L.hn_meshdist_workspace_bytes(T) == al(48 * 64 * nb) + al(32 * nb) + al(32 * ng) + al(4 * T) + 256
    assert L.hn_meshdist_workspace_bytes(-1) == 0 and L.hn_meshdist_workspace_bytes(2 ** 31 - 65) == 0
    assert L.hn_meshdist_workspace_bytes(2 ** 31 - 66) > 0
    csrc = os.path.join(root, 'ho-nerf_amd', 'csrc')
    src = {f: open(os.path.join(csrc, f)).read() for f in ('hn_interact.hip', 'hn_meshdist.hip', 'hn_tridist.h')}
    assert 'float tri_dist2(' in src['hn_tridist.h'] and 'float tri_dist2(' not in src['hn_interact.hip']
    assert all('#include "hn_tridist.h"' in src[f] for f in ('hn_interact.hip', 'hn_meshdist.hip'))
