"""The mesh distance queries on the device (hn_meshdist.hip, honerf_amd.mesh_distance) against the brute force of hn_interact.hip (the
bits of every distance) and the float64 restatement of tests/mesh_distance_cases.py (faces, points, samples, metrics)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_distance_cases as C
from helpers import bounded, cu, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6                                               # m: the project's distance bound (tests/test_interaction.py)
KEYS = ('dist', 'face', 'point', 'bary')


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _bits(out):
    return {k: _np(out[k]).tobytes() for k in KEYS}


def _dev(mesh):
    return torch.from_numpy(mesh[0]).cuda(), torch.from_numpy(mesh[1]).cuda()


def _sets(T):
    """The query sets of the mesh of T triangles: every kind, its point count walking through P_EDGES, and 1000 random points."""
    v, t = C.mesh_T(T)
    k0 = C.T_EDGES.index(T)
    out = [(kind, C.query_set(v, t, kind, C.P_EDGES[(k0 + k) % len(C.P_EDGES)], seed=k0)) for k, kind in enumerate(C.QUERY_KINDS)]
    if C.P_EDGES[(k0 + 4) % len(C.P_EDGES)] != 1000:
        out.append(('random', C.query_set(v, t, 'random', 1000, seed=100 + k0)))
    return out


@functools.lru_cache(maxsize=None)
def results(T):
    """Computed once per mesh and shared, never changed: [(kind, queries, device result as numpy, brute-force distance)]."""
    from honerf_amd.interaction import closest_distance
    from honerf_amd.mesh_distance import MeshIndex
    mesh = _dev(C.mesh_T(T))
    index = MeshIndex(mesh)
    out = []
    for kind, q in _sets(T):
        r = index.closest(q)
        out.append((kind, q, {k: _np(r[k]) for k in KEYS}, _np(closest_distance(mesh, q))))
    return out


# ---- 1: the distance is the brute force's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', C.T_EDGES)
def test_distance_equals_the_brute_force(T):
    for kind, q, r, brute in results(T):
        assert r['dist'].tobytes() == brute.tobytes(), (T, kind, len(q), int((r['dist'] != brute).sum()))
        assert r['dist'].shape == (len(q),) and r['face'].dtype == np.int32 and r['point'].shape == (len(q), 3) and r['bary'].shape == (len(q), 2)
        assert (r['face'] >= 0).all() and (r['face'] < T).all() and np.isfinite(r['dist']).all()
    kinds = {kind: r['dist'] for kind, q, r, _ in results(T)}
    # on the surface d^2 is 0 or a rounding error of the fmaf chains, a few eps x edge^2 (edges of 0.05 at most): d = its root
    assert kinds['far'].min() > 99.0 and kinds['surface'].max() < 0.05 * np.sqrt(16 * 6e-8)


# ---- 2: nothing but the mesh and the point decides ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', C.T_EDGES)
def test_invariance(T):
    from honerf_amd.mesh_distance import MeshIndex
    mesh = _dev(C.mesh_T(T))
    morton, identity = MeshIndex(mesh, order='morton'), MeshIndex(mesh, order='identity')
    rev = MeshIndex(mesh, order=torch.arange(T - 1, -1, -1, dtype=torch.int32))
    for kind, q, r, _ in results(T):
        want = {k: r[k].tobytes() for k in KEYS}
        what = (T, kind, len(q))
        for index in (morton, identity, rev):
            for cull in (True, False):
                for sort in (True, False):
                    assert _bits(index.closest(q, cull=cull, sort=sort)) == want, what + (cull, sort)
        back = morton.closest(q[::-1].copy())
        assert {k: np.ascontiguousarray(_np(back[k])[::-1]).tobytes() for k in KEYS} == want, what
        parts = [identity.closest(q[s:s + 100]) for s in range(0, len(q), 100)]
        assert {k: np.concatenate([_np(p[k]) for p in parts]).tobytes() for k in KEYS} == want, what
        assert _bits(morton.closest(q)) == want, what
        only = morton.closest(q, want=('face',))
        assert list(only) == ['face'] and _np(only['face']).tobytes() == want['face']


# ---- 3: the face attains the distance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', C.T_EDGES)
def test_the_face_attains_the_distance(T):
    """In float64: the triangle `face` is as near as the nearest (within 1e-6 m), `point` is that far from the query and lies on the
    triangle, at the barycentrics returned.  No query is excluded, the nearly tied centre set included.  The bound is 1e-6 m on every
    set of the scene's own scale; the set 100 m away is held to 1e-6 of its distance (1e-4 m): there the fp32 difference a - p, the
    first operation of the query as of the brute force, already rounds by 3.8e-6 m per coordinate, so no fp32 query can promise 1e-6 m
    absolute, and the bits of those distances are the brute force's (test 1)."""
    v, t = C.mesh_T(T)
    v64 = v.astype(np.float64)
    for kind, q, r, _ in results(T):
        tol = TOL * (100.0 if kind == 'far' else 1.0)
        what = 'T=%d %s x %d' % (T, kind, len(q))
        dmin, _, _ = C.np_closest(v, t, q)
        dface, _ = C.np_tri_closest(v, t, q, r['face'])
        bounded(what + ': distance to `face` over the minimum (m)', (dface - dmin).max(), tol, kind='abs')
        record(what + ': dist against the minimum (m)', np.abs(r['dist'] - dmin).max(), 0, kind='value')     # (the brute force's bits: test 1)
        bounded(what + ': | |point - query| - dist | (m)', np.abs(np.linalg.norm(r['point'].astype(np.float64) - q, axis=1) - r['dist']).max(), tol,
                kind='abs')
        tri = t[r['face']]
        bv, bw = r['bary'][:, 0].astype(np.float64), r['bary'][:, 1].astype(np.float64)
        rec = (1 - bv - bw)[:, None] * v64[tri[:, 0]] + bv[:, None] * v64[tri[:, 1]] + bw[:, None] * v64[tri[:, 2]]
        bounded(what + ': point against its barycentric reconstruction (m)', np.abs(rec - r['point']).max(), tol, kind='abs')
        assert min(bv.min(), bw.min(), (1 - bv - bw).min()) >= -1e-6, what


# ---- 4: ties go to the smallest face ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [64, 2049])
def test_tie_break(T):
    from honerf_amd.mesh_distance import MeshIndex
    v, t = C.mesh_T(T)
    q = np.concatenate([C.query_set(v, t, kind, 257, seed=9) for kind in ('surface', 'near', 'centre', 'random')])
    single = MeshIndex(_dev((v, t))).closest(q)
    for order in ('morton', 'identity'):
        twice = MeshIndex(_dev(C.doubled(v, t)), order=order).closest(q)
        assert (_np(twice['face']) < T).all()
        assert _bits(twice) == _bits(single)                                       # the copy behind never wins: the single mesh's answer
        first = MeshIndex(_dev(C.doubled(v, t, copies_first=True)), order=order).closest(q)
        f = _np(first['face'])
        assert (f < T).all()                                                       # the copy in front wins over its original at T + i
        assert _np(first['dist']).tobytes() == _np(single['dist']).tobytes()
        # where no OTHER triangle ties (the query is nearest to one triangle alone), it is the copy of the single mesh's face
        alone = np.zeros(len(q), bool)
        sf, sd = _np(single['face']), _np(single['dist'])
        for k in range(0, len(q), len(q) // 64):
            d_other, _, _ = C.np_closest(v, np.delete(t, sf[k], axis=0), q[k:k + 1])
            alone[k] = d_other[0] > sd[k] + 1e-5
        assert alone.sum() > 8
        assert np.array_equal(f[alone], T - 1 - _np(single['face'])[alone])


# ---- 5: edge inputs -----------------------------------------------------------------------------------------------------------------------
def test_empty_inputs():
    from honerf_amd.mesh_distance import MeshIndex, vertex_distance
    v, t = C.mesh_T(65)
    none = np.zeros((0, 3), np.int64)
    r = MeshIndex((v, none)).closest(v)
    assert torch.isinf(r['dist']).all() and (r['face'] == -1).all() and not r['point'].any() and not r['bary'].any()
    r = MeshIndex((v, t)).closest(np.zeros((0, 3), np.float32))
    assert r['dist'].shape == (0,) and r['face'].shape == (0,) and r['point'].shape == (0, 3) and r['bary'].shape == (0, 2)
    assert vertex_distance(v[:5], (v, none)).tolist() == [float('inf')] * 5
    assert MeshIndex((v, none)).face_normals.shape == (0, 3)


def test_null_outputs_are_not_written():
    from honerf_amd import lib
    L = lib.load()
    v, t = C.mesh_T(65)
    q = C.query_set(v, t, 'random', 300)
    dv, dt, dq = cu(v), cu(t), cu(q)
    ws = cu(np.zeros(L.hn_meshdist_workspace_bytes(65), np.uint8))
    order = cu(np.arange(65, dtype=np.int32))
    s = lib.stream_ptr()
    assert L.hn_meshdist_prepare(lib.ptr(dv), len(v), lib.ptr(dt), 65, lib.ptr(order), lib.ptr(ws), ws.numel(), s) == 0
    full = {k: cu(np.full(shape, 7, dt_)) for k, shape, dt_ in (('dist', 300, np.float32), ('face', 300, np.int32), ('point', (300, 3), np.float32),
                                                                  ('bary', (300, 2), np.float32))}
    assert L.hn_meshdist_closest(lib.ptr(ws), ws.numel(), 65, lib.ptr(dq), 300, 1, *[lib.ptr(full[k]) for k in KEYS], s) == 0
    for k in KEYS:
        part = {j: cu(np.full(tuple(full[j].shape), 7, _np(full[j]).dtype)) for j in KEYS}
        args = [lib.ptr(part[j]) if j == k else None for j in KEYS]
        assert L.hn_meshdist_closest(lib.ptr(ws), ws.numel(), 65, lib.ptr(dq), 300, 1, *args, s) == 0
        torch.cuda.synchronize()
        assert _np(part[k]).tobytes() == _np(full[k]).tobytes()
        assert all((_np(part[j]) == 7).all() for j in KEYS if j != k)
    # n_tris = 0 or n_points = 0: nothing is launched, the outputs stay
    assert L.hn_meshdist_closest(lib.ptr(ws), ws.numel(), 65, lib.ptr(dq), 0, 1, *[lib.ptr(part[j]) for j in KEYS], s) == 0
    assert L.hn_meshdist_closest(None, 0, 0, lib.ptr(dq), 300, 1, *[lib.ptr(part[j]) for j in KEYS], s) == 0
    torch.cuda.synchronize()
    assert all((_np(part[j]) == 7).all() for j in KEYS if j != 'bary')       # (`part` is the last round's: only its bary was written)


def test_zero_area_and_nan_triangles():
    from honerf_amd.interaction import closest_distance
    from honerf_amd.mesh_distance import MeshIndex
    v, t = C.mesh_T(2049)
    n = len(v)
    # a zero-area triangle (a segment) 1 cm outside the mesh's bounds, a point triangle, and a triangle with a NaN vertex beside them
    far = v.max(0) + np.float32(0.01)
    extra = np.array([far, far + np.float32([0.02, 0.0, 0.0]), far + np.float32([0.0, 0.03, 0.0]), [np.nan, far[1], far[2]]], np.float32)
    vv = np.concatenate([v, extra])
    tt = np.concatenate([t[:1000], np.array([[n, n + 1, n + 1], [n + 2, n + 2, n + 2], [n + 3, n, n + 1]], np.int64), t[1000:]])
    q = np.concatenate([extra[:3] + np.float32([0.0, 0.0, 0.004]), (0.5 * (extra[0] + extra[1]))[None], C.query_set(v, t, 'random', 500, seed=3)])
    q = np.ascontiguousarray(q, np.float32)
    mesh = _dev((vv, tt))
    brute = _np(closest_distance(mesh, q))
    for order in ('morton', 'identity'):
        for cull in (True, False):
            r = MeshIndex(mesh, order=order).closest(q, cull=cull)
            assert _np(r['dist']).tobytes() == brute.tobytes()
            f = _np(r['face'])
            assert f[0] == 1000 and f[1] == 1000 and f[2] == 1001 and f[3] == 1000      # the segment and the point win where they are nearest
            assert (f != 1002).all()                                                      # the NaN triangle never
            assert np.isfinite(_np(r['point'])).all() and np.isfinite(_np(r['bary'])).all()
    # (on the segment itself the selects of a triangle with b = c divide rounding residues: the brute force's distance there is some
    # point of the segment's, not 0; the query gives its bits, and the segment still wins)
    assert abs(brute[0] - 0.004) < 1e-6 and brute[3] <= 0.01 + 1e-6
    # the others are unaffected: the mesh without the three gives the same answer wherever none of them is the winner
    plain = MeshIndex(_dev((v, t))).closest(q)
    keep = f < 1000
    assert keep.sum() > 100 and _np(plain['dist'])[keep].tobytes() == brute[keep].tobytes()
    assert np.array_equal(_np(plain['face'])[keep], f[keep])
    # only NaN triangles: no distance
    r = MeshIndex(_dev((vv, np.array([[n + 3, n, n + 1]], np.int64)))).closest(q[:70])
    assert torch.isinf(r['dist']).all() and (r['face'] == -1).all() and not r['point'].any()
    assert torch.isinf(closest_distance((vv, np.array([[n + 3, n, n + 1]], np.int64)), q[:70])).all()


def test_refusals():
    from honerf_amd import lib
    from honerf_amd.mesh_distance import MeshIndex, sample_surface, surface_metrics, vertex_distance
    L = lib.load()
    v, t = C.mesh_T(65)
    dv, dt, dq = cu(v), cu(t), cu(C.query_set(v, t, 'random', 10))
    need = L.hn_meshdist_workspace_bytes(65)
    ws = cu(np.zeros(need, np.uint8))
    s = lib.stream_ptr()
    order = cu(np.arange(65, dtype=np.int32))
    out = cu(np.zeros(10, np.float32))
    EINVAL = -1

    def refused(rc, word):
        assert rc == EINVAL and word in L.hn_last_error().decode(), (rc, L.hn_last_error())
    for bad in (-1, 2 ** 31 - 65, 2 ** 31):
        assert L.hn_meshdist_workspace_bytes(bad) == 0
        refused(L.hn_meshdist_prepare(lib.ptr(dv), len(v), lib.ptr(dt), bad, lib.ptr(order), lib.ptr(ws), need, s), 'n_tris')
        refused(L.hn_meshdist_closest(lib.ptr(ws), need, bad, lib.ptr(dq), 10, 1, lib.ptr(out), None, None, None, s), 'n_tris')
        refused(L.hn_meshdist_closest(lib.ptr(ws), need, 65, lib.ptr(dq), bad, 1, lib.ptr(out), None, None, None, s), 'n_points')
        refused(L.hn_mesh_sample(lib.ptr(dv), len(v), lib.ptr(dt), 65, lib.ptr(ws), bad, 0, None, None, None, s), 'n = ')
        refused(L.hn_mesh_face_areas(lib.ptr(dv), len(v), lib.ptr(dt), bad, None, None, s), 'n_tris')
    refused(L.hn_meshdist_prepare(lib.ptr(dv), len(v), lib.ptr(dt), 65, lib.ptr(order), lib.ptr(ws), need - 1, s), 'workspace')
    refused(L.hn_meshdist_closest(lib.ptr(ws), need - 1, 65, lib.ptr(dq), 10, 1, lib.ptr(out), None, None, None, s), 'workspace')
    refused(L.hn_meshdist_prepare(None, len(v), lib.ptr(dt), 65, lib.ptr(order), lib.ptr(ws), need, s), 'NULL')
    refused(L.hn_meshdist_closest(lib.ptr(ws), need, 65, None, 10, 1, lib.ptr(out), None, None, None, s), 'NULL')
    for wrong in (np.zeros(65, np.int32), np.r_[np.arange(64), 63].astype(np.int32), np.r_[np.arange(64), 65].astype(np.int32),
                  np.r_[-1, np.arange(64)].astype(np.int32)):
        refused(L.hn_meshdist_prepare(lib.ptr(dv), len(v), lib.ptr(dt), 65, lib.ptr(cu(wrong)), lib.ptr(ws), need, s), 'permutation')
    assert L.hn_meshdist_prepare(lib.ptr(dv), len(v), lib.ptr(dt), 65, lib.ptr(cu(np.arange(64, -1, -1, dtype=np.int32))), lib.ptr(ws), need, s) == 0
    # Python
    tv, tt = torch.from_numpy(v), torch.from_numpy(t)
    for make in (lambda: MeshIndex((tv, tt)), lambda: MeshIndex((v, t)).closest(tv), lambda: MeshIndex((v, t), order='sorted'),
                 lambda: MeshIndex((v, t), order=np.zeros(65, np.int64)), lambda: MeshIndex((v, t), order=np.arange(64)),
                 lambda: MeshIndex((v, t.astype(np.float32))), lambda: MeshIndex((v[:, :2], t)), lambda: MeshIndex((v, t + len(v))),
                 lambda: MeshIndex((v, t)).closest(v[:, :2]), lambda: MeshIndex((v, t)).closest(v.astype(np.float16)),
                 lambda: MeshIndex((tv.cuda().requires_grad_(), tt.cuda())), lambda: MeshIndex((v, t)).closest(tv.cuda().requires_grad_()),
                 lambda: vertex_distance(tv, (v, t)), lambda: sample_surface((tv, tt), 10), lambda: sample_surface((v, t), -1),
                 lambda: sample_surface((v, t), 10, seed=-1), lambda: surface_metrics((v, t), (v, t), n=0),
                 lambda: surface_metrics((v, t), (tv, tt), n=10)):
        with pytest.raises(ValueError):
            make()


# ---- 6: the sampler -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, n, seed', C.SAMPLER_CASES)
def test_sampler_matches_the_restatement(name, n, seed):
    from honerf_amd.mesh_distance import sample_surface
    v, t = C.sampler_mesh(name)
    pts, face, nrm = sample_surface((v, t), n, seed)
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and face.shape == (n,) and face.dtype == torch.int32 and nrm.shape == (n, 3)
    rp, rf, rn = C.np_sample(v, t, n, seed)
    exempt = C.knot_gap(v, t, n, seed)
    assert exempt.sum() <= 1e-3 * n                       # (the inputs are chosen with none: test_mesh_distance_cpu.py)
    ok = ~exempt
    assert np.array_equal(_np(face)[ok].astype(np.int64), rf[ok])
    bounded('%s n=%d: sample points against float64' % (name, n), np.abs(_np(pts)[ok] - rp[ok]).max(), 1e-6, kind='abs')
    bounded('%s n=%d: sample normals against float64' % (name, n), np.abs(_np(nrm)[ok] - rn[ok]).max(), 1e-6, kind='abs')
    again = sample_surface(_dev((v, t)), n, seed)
    assert all(_np(a).tobytes() == _np(b).tobytes() for a, b in zip((pts, face, nrm), again))
    if n > 1:
        assert _np(sample_surface((v, t), n, seed + 1)[0]).tobytes() != _np(pts).tobytes()


def test_sampler_refuses_a_mesh_without_area():
    from honerf_amd.mesh_distance import sample_surface, surface_metrics
    v, t = C.mesh_T(65)
    flat = np.stack([t[:, 0], t[:, 0], t[:, 1]], 1)
    for mesh in ((v, flat), (v, np.zeros((0, 3), np.int64))):
        with pytest.raises(ValueError, match='area'):
            sample_surface(mesh, 10)
        with pytest.raises(ValueError, match='area'):
            surface_metrics((v, t), mesh, n=10)
    assert sample_surface((v, t), 0)[0].shape == (0, 3)


# ---- 7: the metrics -----------------------------------------------------------------------------------------------------------------------
def _hand(res):
    from test_interaction import hand_object
    (hv, ht), _ = hand_object(res)
    return _np(hv).astype(np.float32), _np(ht)


@pytest.mark.parametrize('case', ['spheres', 'hand'])
def test_surface_metrics_match_the_restatement(case):
    from honerf_amd.mesh_distance import MeshIndex, surface_metrics
    if case == 'spheres':
        pred, gt, n = C.sphere_mesh((0.0, 0.0, 0.0), 0.05, 16), C.sphere_mesh((0.0, 0.0, 0.0), 0.06, 20), 200
    else:
        pred, gt, n = _hand(16), _hand(24), 600
    got = {}
    surface_metrics(pred, gt, n=n, seed=4, samples=got)
    s = {k: _np(x) for k, x in got.items()}
    # the normal consistency is that of the faces the device found (test 3: each attains the distance); where several faces are equally
    # near, a sample on a ridge of the other mesh, float64 might name another and its normal
    faces = (_np(MeshIndex(gt).closest(s['pred_points'])['face']), _np(MeshIndex(pred).closest(s['gt_points'])['face']))
    _, acc, comp = C.np_surface_metrics(pred, gt, s['pred_points'], s['pred_normals'], s['gt_points'], s['gt_normals'], detail=True)
    # thresholds inside the distribution (between its 5 % and 95 % quantiles), in the middle of its two widest gaps: no distance
    # within 1e-6 of either
    both = np.sort(np.concatenate([acc, comp]))
    mid = both[len(both) // 20: 19 * len(both) // 20]
    gaps = np.diff(mid)
    taus = tuple(float(mid[k] + 0.5 * gaps[k]) for k in np.argsort(gaps)[-2:])
    for tau in taus:
        band = int((np.abs(both - tau) <= TOL).sum())
        record('%s: distances within 1e-6 of tau = %.6f' % (case, tau), band, 0, kind='count')
        assert band == 0
    m = surface_metrics(pred, gt, n=n, taus=taus, seed=4)
    ref = C.np_surface_metrics(pred, gt, s['pred_points'], s['pred_normals'], s['gt_points'], s['gt_normals'], taus, faces=faces)
    assert set(m) == set(ref) and all(isinstance(x, float) for k, x in m.items() if k != 'n') and m['n'] == n
    for k in ('chamfer_l1', 'hausdorff', 'accuracy', 'completeness'):
        bounded('%s %s (m)' % (case, k), abs(m[k] - ref[k]), TOL, kind='abs')
    bounded('%s chamfer_l2 (m^2)' % case, abs(m['chamfer_l2'] - ref['chamfer_l2']), 2 * TOL * ref['hausdorff'] * 2, kind='abs')
    bounded('%s normal_consistency' % case, abs(m['normal_consistency'] - ref['normal_consistency']), 1e-6, kind='abs')
    for k in ('pred_area', 'gt_area'):
        bounded('%s %s (rel)' % (case, k), abs(m[k] - ref[k]) / ref[k], 1e-12)
    for tau in taus:
        for k in ('precision@%g', 'recall@%g', 'fscore@%g'):
            assert m[k % tau] == ref[k % tau], (k % tau, m[k % tau], ref[k % tau])
        assert 0.0 < m['precision@%g' % tau] < 1.0 or 0.0 < m['recall@%g' % tau] < 1.0
    assert surface_metrics(pred, gt, n=n, taus=taus, seed=4) == m                  # the same bits on every run
    assert surface_metrics(_dev(pred), _dev(gt), n=n, taus=taus, seed=4) == m
    assert surface_metrics(pred, gt, n=n, taus=taus, seed=5) != m


def test_vertex_distance_is_the_plain_query():
    from honerf_amd.interaction import closest_distance
    from honerf_amd.mesh_distance import MeshIndex, vertex_distance
    v, t = C.mesh_T(2049)
    q = C.query_set(v, t, 'random', 700, seed=2)
    d = vertex_distance(q, (v, t))
    assert _np(d).tobytes() == _np(closest_distance((v, t), q)).tobytes()
    n = MeshIndex((v, t)).face_normals
    bounded('face normals against float64', np.abs(_np(n) - C.np_face_areas(v, t)[1]).max(), 1e-6, kind='abs')


# ---- 8: the interaction metrics' opt-in -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['spheres', 'hand_object'])
def test_interaction_opt_in_gives_the_same_bits(case):
    from honerf_amd import interaction as it
    if case == 'spheres':
        from test_interaction_cpu import mc_sphere
        hand, obj = mc_sphere((0.0, 0.0, 0.9), 0.05, 32)[:2], mc_sphere((0.08, 0.0, 0.9), 0.06, 32)[:2]
        pts = hand[0]
    else:
        from test_interaction import hand_object
        hand, obj = hand_object(32)
        pts = hand[0]
    a, b = it.closest_distance(obj, pts), it.closest_distance(obj, pts, culled=True)
    assert _np(a).tobytes() == _np(b).tobytes() and len(_np(a)) > 100
    pa, pb = it.penetration_depth(hand, obj), it.penetration_depth(hand, obj, culled=True)
    assert pa == pb and pa > 0.0
    assert it.interaction_metrics(hand, obj) == it.interaction_metrics(hand, obj, culled=True)
    none = (obj[0], np.zeros((0, 3), np.int64))
    assert torch.isinf(it.closest_distance(none, pts, culled=True)).all() and it.penetration_depth(hand, none, culled=True) == 0.0


# ---- 9: end to end ------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_tool(tmp_path):
    from honerf_amd import harness
    from honerf_amd.mesh_distance import surface_metrics
    pred = {'a.ply': C.sphere_mesh((0.0, 0.0, 0.0), 0.05, 16), 'b.ply': C.sphere_mesh((0.002, 0.0, 0.0), 0.052, 14)}
    gt = C.sphere_mesh((0.0, 0.0, 0.0), 0.05, 20)
    (tmp_path / 'pred').mkdir()
    (tmp_path / 'gt').mkdir()
    for name, m in pred.items():
        harness.write_ply(str(tmp_path / 'pred' / name), *m)
        harness.write_ply(str(tmp_path / 'gt' / name), *gt)
    out_json = tmp_path / 'out.json'
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'mesh_eval.py'), str(tmp_path / 'pred'), str(tmp_path / 'gt'), '--n', '3000', '--tau', '0.001',
           '--tau', '0.003', '--seed', '2', '--json', str(out_json)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out_json.read_text())
    assert [r['name'] for r in res['rows']] == ['a.ply', 'b.ply']
    for r in res['rows']:
        want = surface_metrics(harness.read_ply(str(tmp_path / 'pred' / r['name'])), harness.read_ply(str(tmp_path / 'gt' / r['name'])), n=3000,
                               taus=(0.001, 0.003), seed=2)
        assert {k: x for k, x in r.items() if k != 'name'} == want
        assert ('%.3f' % (want['chamfer_l1'] * 1000)) in out.stdout
    assert res['mean']['chamfer_l1'] == (res['rows'][0]['chamfer_l1'] + res['rows'][1]['chamfer_l1']) / 2
    assert 'mm' in out.stdout and 'mean of 2' in out.stdout
    assert res['rows'][0]['chamfer_l1'] < res['rows'][1]['chamfer_l1'] < 0.01
    # a single ground-truth file for every prediction
    one = subprocess.run(cmd[:3] + [str(tmp_path / 'gt' / 'a.ply')] + cmd[4:], capture_output=True, text=True, timeout=600, env=env)
    assert one.returncode == 0 and json.loads(out_json.read_text())['rows'] == res['rows'], one.stderr[-2000:]
