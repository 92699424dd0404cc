"""The device interaction metrics (hn_interact.hip through honerf_amd.interaction) against the float64 restatement of
tests/test_interaction_cpu.py: voxel key sets exactly, containment flags exactly away from the surface, distances to 1e-6 m, and
interaction_metrics on the synthetic hand and object; same bits on a repeated call; odd sizes; refusals; hand_object_meshes against
extract_geometry(..., mesher='native'); and the driver tool on a tree of PLY files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import bounded, product_modules, record, t
from test_interaction_cpu import (mc_sphere, np_contains, np_distance, np_metrics, np_voxel_keys, np_winding)
from test_mesh_cpu import noise_volume, np_marching_cubes, sphere_volume, torus_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH = 0.005


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def world(vol, side, center=(0.0, 0.0, 0.0)):
    """An index-space marching-cubes mesh of vol placed in a cube of the given side (metres)."""
    v, tr = np_marching_cubes(vol, 0.0)
    h = side / (vol.shape[0] - 1.0)
    return v.astype(np.float64) * h - side / 2 + np.asarray(center), tr


def check_keys(v, tr, what, pitch=PITCH):
    from honerf_amd.interaction import voxelize_surface
    pts = _np(voxelize_surface((v, tr), pitch))
    ref = np_voxel_keys(v, tr, pitch)
    keys = np.rint(pts / pitch).astype(np.int64)
    assert np.array_equal(keys * pitch, pts), what               # the points are k * pitch exactly
    assert keys.shape == ref.shape and np.array_equal(keys, ref), (what, keys.shape, ref.shape)
    return pts


def check_queries(v, tr, pts, what, closed=True):
    """contains and closest_distance of pts against the restatement (only points inside the mesh's bounds are evaluated there).
    No point may lie within 1e-5 m of the surface (the band where fp32 and fp64 may disagree: reported, and asserted empty), and
    every flag must agree.  An open mesh (closed=False) has a non-integer w; its flags are compared too, and w itself to 1e-3."""
    from honerf_amd.interaction import closest_distance, contains, winding_number
    pts = np.asarray(pts, np.float64)
    lo, hi = np.asarray(v, np.float32).min(0), np.asarray(v, np.float32).max(0)
    p32 = pts.astype(np.float32)
    live = ((p32 >= lo) & (p32 <= hi)).all(1)
    got = _np(contains((v, tr), pts))
    assert got.dtype == np.bool_ and got.shape == (len(pts),)
    assert not got[~live].any(), what
    d_ref = np_distance(v, tr, pts[live])
    band = int((d_ref < 1e-5).sum())
    record(what + ' points within 1e-5 m of the surface', band, 0, kind='count')
    assert band == 0, what
    ref = np_contains(v, tr, pts[live])
    assert np.array_equal(got[live], ref), (what, int((got[live] != ref).sum()))
    if not closed:
        w = _np(winding_number((v, tr), pts[live])).astype(np.float64)
        bounded(what + ' winding number', np.abs(w - np_winding(v, tr, pts[live])).max() if live.any() else 0.0, 1e-3, kind='abs')
    d = _np(closest_distance((v, tr), pts[live])).astype(np.float64)
    bounded(what + ' distance', np.abs(d - d_ref).max() if len(d) else 0.0, 1e-6, kind='abs')
    return got


def away(v, tr, pts, closed=True):
    """Random query points without those the restatement puts within 1e-5 m of the surface, or, on an open mesh, within 1e-3 of
    |w| = 1/2 (a sheet that spans the mesh's holes, where a flag rests on the last bits of w).  The drawn points and the kept ones
    are recorded; the scenes made of mesh data (voxel points, hand vertices) are never filtered."""
    pts = np.asarray(pts, np.float64)
    keep = np_distance(v, tr, pts) >= 1e-5
    if not closed:
        keep &= np.abs(np.abs(np_winding(v, tr, pts)) - 0.5) > 1e-3
    record('random points kept of %d' % len(pts), int(keep.sum()), len(pts), kind='count')
    return pts[keep]


def sample(n, lo, hi, seed):
    return np.random.RandomState(seed).uniform(lo, hi, size=(n, 3))


# ---- analytic and noise scenes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [64, 128])
@pytest.mark.parametrize('kind', ['sphere', 'torus'])
def test_analytic_meshes_match_the_restatement(kind, res):
    vol = (sphere_volume if kind == 'sphere' else torus_volume)(res)
    v, tr = world(vol, 0.2, (0.02, -0.01, 0.9))
    what = '%s %d' % (kind, res)
    check_keys(v, tr, what)
    check_queries(v, tr, away(v, tr, sample(2000, v.min(0) - 0.01, v.max(0) + 0.01, res)), what)


def test_noise_mesh_matches_the_restatement():
    vol = noise_volume((23, 19, 17), seed=5)
    v, tr = np_marching_cubes(vol, 0.0)
    v = v.astype(np.float64) * 0.004 + np.array([0.1, -0.05, 0.8])
    check_keys(v, tr, 'noise')
    check_queries(v, tr, away(v, tr, sample(2000, v.min(0), v.max(0), 1), closed=False), 'noise', closed=False)


# ---- the synthetic hand and object ---------------------------------------------------------------------------------------------
def _dual():
    from honerf_amd.renderer import NeuSRenderer_fitting
    m = product_modules()
    return NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)


def hand_object(res, shift=0.0):
    """The synthetic hand (synth_hand_pose(3), box = joints +- 0.08) and the object posed at j[9] (+ shift along x) in a +-0.35 box."""
    from honerf_amd import synth
    from honerf_amd.interaction import hand_object_meshes
    bt, tp, j = synth.synth_hand_pose(3)
    c = j[9] + np.array([shift, 0.0, 0.0], np.float32)
    R, tt = synth.synth_obj_pose(2, center=tuple(c))
    Ro, To = t(R).T.contiguous(), t(tt)
    (hv, ht), (ov, ot) = hand_object_meshes(_dual(), t(j.min(0) - 0.08), t(j.max(0) + 0.08), t(c - 0.35), t(c + 0.35), res, bt, tp, Ro, To)
    return (hv, ht), (ov, ot)


PARTIAL_SHIFT = 0.15      # m along x: the object's surface passes through the hand (test_real_penetration_metrics asserts it)


def partial_shift():
    record('partial pose: object shift along x (m)', PARTIAL_SHIFT, 0, kind='value')
    return PARTIAL_SHIFT


@pytest.mark.parametrize('res', [64, 128])
@pytest.mark.parametrize('pose', ['deep', 'partial'])
def test_hand_object_queries_match_the_restatement(pose, res):
    hand, obj = hand_object(res, 0.0 if pose == 'deep' else partial_shift())
    hv, ht = _np(hand[0]), _np(hand[1])
    ov, ot = _np(obj[0]), _np(obj[1])
    what = 'hand/object %s %d' % (pose, res)
    pts = check_keys(ov, ot, what + ' object keys')
    check_queries(hv, ht, pts, what + ' object voxels in the hand')
    hp = hv if res == 64 else hv[np.random.RandomState(0).choice(len(hv), 2000, replace=False)]
    check_queries(ov, ot, hp, what + ' hand vertices in the object')


@pytest.mark.parametrize('pose', ['deep', 'partial'])
def test_real_penetration_metrics(pose):
    from honerf_amd.interaction import interaction_metrics
    hand, obj = hand_object(64, 0.0 if pose == 'deep' else partial_shift())
    m = interaction_metrics(hand, obj)
    ref = np_metrics((_np(hand[0]), _np(hand[1])), (_np(obj[0]), _np(obj[1])))
    assert m['n_obj_voxels'] == ref['n_obj_voxels'] and m['n_obj_voxels_inside'] == ref['n_obj_voxels_inside']
    assert m['n_hand_verts_inside'] == ref['n_hand_verts_inside'] > 0
    assert m['int_vol'] == ref['int_vol']
    bounded('%s pen_dep (mm)' % pose, abs(m['pen_dep'] - ref['pen_dep']), 1e-3, kind='abs')
    assert m['hand_closed'] and isinstance(m['obj_closed'], bool)
    if pose == 'partial':
        assert 0 < m['n_obj_voxels_inside'] < m['n_obj_voxels']
    record('%s int_vol cm^3' % pose, m['int_vol'], 0, kind='value')
    record('%s pen_dep mm' % pose, m['pen_dep'], 0, kind='value')


def test_repeated_calls_give_the_same_bits():
    from honerf_amd.interaction import closest_distance, interaction_metrics, winding_number
    hand, obj = hand_object(64)
    hv = hand[0]
    a = (winding_number(obj, hv), closest_distance(obj, hv), interaction_metrics(hand, obj))
    b = (winding_number(obj, hv), closest_distance(obj, hv), interaction_metrics(hand, obj))
    assert _np(a[0]).tobytes() == _np(b[0]).tobytes()
    assert _np(a[1]).tobytes() == _np(b[1]).tobytes()
    assert a[2] == b[2]


# ---- sizes, empties, refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_points', [1, 63, 64, 65, 5000])
def test_odd_point_and_triangle_counts(n_points):
    v, tr = mc_sphere((0.0, 0.0, 0.0), 0.05, 13)[:2]
    assert len(tr) % 256 != 0                                                     # not a multiple of the 256-triangle tile
    for tris, seed, closed, what in ((tr, n_points, True, 'sphere 13 (%d tris)' % len(tr)), (tr[:300], n_points + 1, False, '300 tris'),
                                     (tr[:1], n_points + 2, False, '1 tri')):
        q = away(v, tris, sample(n_points + 64, -0.07, 0.07, seed), closed)[:n_points]
        assert len(q) == n_points
        check_queries(v, tris, q, '%s x %d points' % (what, n_points), closed=closed)


def test_empty_inputs_give_zeros():
    from honerf_amd import interaction as it
    v, tr = mc_sphere((0.0, 0.0, 0.0), 0.05, 13)[:2]
    none = np.zeros((0, 3), np.int64)
    no_pts = np.zeros((0, 3))
    assert it.contains((v, tr), no_pts).shape == (0,)
    assert it.closest_distance((v, tr), no_pts).shape == (0,)
    assert not it.contains((v, none), v).any()
    assert torch.isinf(it.closest_distance((v, none), v)).all()
    assert it.voxelize_surface((v, none), PITCH).shape == (0, 3)
    m = it.interaction_metrics((v, none), (v, none))
    assert m['int_vol'] == 0 and m['pen_dep'] == 0 and m['n_obj_voxels'] == 0
    assert it.penetration_depth((v, tr), (v, none)) == 0.0
    assert it.intersection_volume((v, none), (v, tr)) == 0.0


def test_round_cap_and_bad_arguments_are_refused():
    from honerf_amd import interaction as it
    p = PITCH
    ok = (np.array([[0.0, 0, 0], [300 * p, 0, 0], [0, 300 * p, 0]]), np.array([[0, 1, 2]]))    # exactly 10 rounds: allowed
    assert np.array_equal(np.rint(_np(it.voxelize_surface(ok, p)) / p).astype(np.int64), np_voxel_keys(ok[0], ok[1], p))
    big = (np.array([[0.0, 0, 0], [400 * p, 0, 0], [0, 400 * p, 0]]), np.array([[0, 1, 2]]))    # 11 rounds: refused
    with pytest.raises(ValueError, match='rounds'):
        it.voxelize_surface(big, p)
    with pytest.raises(ValueError, match='rounds'):
        it.voxelize_surface((np.array([[0.0, 0, 0], [10.0, 0, 0], [0, 10.0, 0]]), np.array([[0, 1, 2]])), p)
    with pytest.raises(ValueError):
        it.voxelize_surface((np.array([[1e4, 0, 0], [1e4, 0.001, 0], [1e4, 0, 0.001]]), np.array([[0, 1, 2]])), p)   # key range
    v, tr = mc_sphere((0.0, 0.0, 0.0), 0.05, 13)[:2]
    pts = sample(10, -0.05, 0.05, 0)
    with pytest.raises(ValueError):
        it.contains((v.astype(np.float16), tr), pts)                 # dtype
    with pytest.raises(ValueError):
        it.contains((v, tr), pts.reshape(-1))                        # rank
    with pytest.raises(ValueError):
        it.contains((v, tr), pts.astype(np.int32))
    with pytest.raises(ValueError):
        it.closest_distance((torch.from_numpy(v), torch.from_numpy(tr)), pts)   # CPU tensors
    with pytest.raises(ValueError):
        it.contains((v, tr), torch.from_numpy(pts))
    with pytest.raises(ValueError):
        it.contains((v, tr + len(v)), pts)                            # indices
    with pytest.raises(ValueError):
        it.voxelize_surface((v, tr), 0.0)


def test_solid_volume_on_the_device():
    """solid=True on two spheres against the restatement's lattice count (flags may differ only at points within 1e-5 m)."""
    from honerf_amd.interaction import intersection_volume
    from test_interaction_cpu import np_solid_volume
    hand = mc_sphere((0.0, 0.0, 0.0), 0.05, 28)[:2]
    obj = mc_sphere((0.08, 0.0, 0.0), 0.06, 28)[:2]
    got = intersection_volume(obj, hand, 0.0035, solid=True)
    ref = np_solid_volume(obj, hand, 0.0035)
    bounded('solid lens volume rel', abs(got - ref) / ref, 2e-3)
    assert 0 < intersection_volume(obj, hand, PITCH) < got


# ---- meshes of the renderer, and the driver -------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [48, 64])
def test_hand_object_meshes_match_extract_geometry(res):
    from honerf_amd import synth
    from honerf_amd.interaction import hand_object_meshes
    bt, tp, j = synth.synth_hand_pose(3)
    c = j[9]
    R, tt = synth.synth_obj_pose(2, center=tuple(c))
    Ro, To = t(R).T.contiguous(), t(tt)
    dual = _dual()
    hb, ob = (t(j.min(0) - 0.08), t(j.max(0) + 0.08)), (t(c - 0.35), t(c + 0.35))
    (hv, ht), (ov, ot) = hand_object_meshes(dual, hb[0], hb[1], ob[0], ob[1], res, bt, tp, Ro, To)
    assert hv.is_cuda and ov.is_cuda and hv.dtype == torch.float64 and ht.dtype == torch.int64
    for (v, tr), (b0, b1), kind in (((hv, ht), hb, 'hand'), ((ov, ot), ob, 'obj')):
        ev, et = dual.extract_geometry(b0, b1, res, bt, tp, Ro, To, kind, mesher='native')
        assert np.array_equal(_np(tr), et), kind
        bounded('hand_object_meshes %s %d vertices' % (kind, res), np.abs(_np(v) - ev).max(), 1e-6, kind='abs')


def test_interaction_eval_tool(tmp_path):
    from honerf_amd import harness
    d = 0.08
    frames = {('1', 'mesh_1', 0): d, ('1', 'mesh_1', 1): 0.2, ('12', 'mesh_12', 0): 0.09, ('12', 'mesh_12', 1): 0.07}
    expect = {}
    for (fit, sub, fid), dist in frames.items():
        hand = mc_sphere((0.0, 0.0, 0.9), 0.05, 20)[:2]
        obj = mc_sphere((dist, 0.0, 0.9), 0.06, 20)[:2]
        p = tmp_path / fit / 'p1_box' / 'seq0' / sub
        p.mkdir(parents=True, exist_ok=True)
        harness.write_ply(str(p / ('%d_hand.ply' % fid)), hand[0], hand[1])
        harness.write_ply(str(p / ('%d_obj.ply' % fid)), obj[0], obj[1])
        hv, htr = harness.read_ply(str(p / ('%d_hand.ply' % fid)))
        ov, otr = harness.read_ply(str(p / ('%d_obj.ply' % fid)))
        expect[(fit, fid)] = np_metrics((hv.astype(np.float64), htr), (ov.astype(np.float64), otr))
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'interaction_eval.py'), str(tmp_path)], capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    mean = lambda fit, k: (expect[(fit, 0)][k] + expect[(fit, 1)][k]) / 2
    line = 'fit1_int_sum: %.2lf, fit1_dep_sum: %.2lf, fit12_int_sum: %.2lf, fit12_dep_sum: %.2lf' % (
        mean('1', 'int_vol'), mean('1', 'pen_dep'), mean('12', 'int_vol'), mean('12', 'pen_dep'))
    assert 'object class box has 2 frames' in out.stdout, out.stdout
    assert line in out.stdout, (line, out.stdout)
    assert 'object class cup has 0 frames' in out.stdout
    assert mean('1', 'pen_dep') > 0                          # the overlapping frame penetrates
