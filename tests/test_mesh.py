"""The device marching cubes (hn_mcubes.hip through honerf_amd.mesh) against the numpy restatement of tests/test_mesh_cpu.py:
triangles exactly, vertices to a few ulp of the index coordinate; its surfaces on analytic volumes; edge cases; and
extract_geometry(..., mesher='native') of both renderers against the restatement run on extract_fields of the same arguments."""
import numpy as np
import pytest
import torch

from helpers import bounded, product_modules, t
from test_mesh_cpu import (area_volume, cases_present, edge_stats, euler, noise_volume, np_marching_cubes, sphere_volume,
                           torus_volume)

pytestmark = pytest.mark.gpu


def gpu_mesh(vol, threshold=0.0):
    from honerf_amd.mesh import marching_cubes
    v, tr = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), threshold)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and tr.dtype == torch.int64 and v.is_cuda and tr.is_cuda
    return v.cpu().numpy(), tr.cpu().numpy()


def assert_same_mesh(vol, threshold, what):
    v, tr = gpu_mesh(vol, threshold)
    rv, rt = np_marching_cubes(vol, threshold)
    assert v.shape == rv.shape and tr.shape == rt.shape, (what, v.shape, rv.shape, tr.shape, rt.shape)
    assert np.array_equal(tr, rt), what
    ulp = np.spacing(np.abs(rv).astype(np.float32)).astype(np.float64)
    d = (np.abs(v.astype(np.float64) - rv) / ulp).max() if len(v) else 0.0
    bounded(what + ' vertices (ulp)', d, 4.0, kind='ulp')
    return v, tr


@pytest.mark.parametrize('threshold', [0.0, 0.05])
def test_noise_volume_matches_the_restatement_exactly(threshold):
    vol = noise_volume((23, 19, 17), seed=5)
    nontrivial = cases_present(vol, threshold) - {0, 255}
    assert len(nontrivial) >= 250, len(nontrivial)
    v, tr = assert_same_mesh(vol, threshold, 'noise 23x19x17 thr %g' % threshold)
    assert len(v) > 1000 and len(tr) > 1000


@pytest.mark.parametrize('shape', [(2, 2, 2), (2, 3, 4), (5, 2, 9), (8, 12, 16), (31, 17, 5)])
def test_small_and_aligned_shapes_match_the_restatement(shape):
    """nz a multiple of 4 takes the vector-load kernels, other nz the element-wise ones; both against the restatement."""
    vol = noise_volume(shape, seed=sum(shape))
    assert_same_mesh(vol, 0.0, 'noise %s' % (shape,))


@pytest.mark.parametrize('threshold', [0.0, 0.05])
@pytest.mark.parametrize('kind', ['sphere', 'torus'])
def test_analytic_volumes_match_the_restatement_exactly(kind, threshold):
    vol = (sphere_volume if kind == 'sphere' else torus_volume)(64)
    assert_same_mesh(vol, threshold, '%s 64 thr %g' % (kind, threshold))


@pytest.mark.parametrize('res', [64, 128])
def test_sphere_geometry(res):
    r = 0.3
    h = 1.0 / (res - 1)
    v, tr = gpu_mesh(sphere_volume(res, r), 0.0)
    w = v.astype(np.float64) * h - 0.5
    dev = np.abs(np.linalg.norm(w, axis=1) - r).max()
    bounded('sphere %d |v| - r' % res, dev, h * h / (8 * (r - h)) + 1e-6, kind='abs')
    assert euler(v, tr) == 2
    assert edge_stats(tr) == (0, 0)
    area, volume = area_volume(w, tr)
    assert volume > 0
    ea, ev = abs(area / (4 * np.pi * r * r) - 1), abs(volume / (4 / 3 * np.pi * r ** 3) - 1)
    bounded('sphere %d area' % res, ea, 0.02)
    bounded('sphere %d volume' % res, ev, 0.02)
    test_sphere_geometry.errors[res] = (ea, ev)
    if len(test_sphere_geometry.errors) == 2:
        (a64, v64), (a128, v128) = test_sphere_geometry.errors[64], test_sphere_geometry.errors[128]
        assert a128 < a64 and v128 < v64


test_sphere_geometry.errors = {}


def test_torus_topology():
    v, tr = gpu_mesh(torus_volume(64), 0.0)
    assert euler(v, tr) == 0
    assert edge_stats(tr) == (0, 0)
    assert area_volume(v, tr)[1] > 0


@pytest.mark.parametrize('value', [-1.0, 1.0, 0.0])
def test_volume_without_crossing_gives_empty_outputs(value):
    v, tr = gpu_mesh(np.full((9, 8, 7), value, np.float32), 0.0)     # 0.0: every point is outside (not < 0)
    assert v.shape == (0, 3) and tr.shape == (0, 3)


def test_dims_below_two_are_refused():
    from honerf_amd.mesh import marching_cubes
    for shape in [(1, 5, 5), (5, 1, 5), (5, 5, 1)]:
        with pytest.raises(RuntimeError, match='>= 2'):
            marching_cubes(torch.zeros(shape, device='cuda'), 0.0)
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros(4, 4, 4, device='cuda', dtype=torch.float64), 0.0)
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros(4, 4, 4), 0.0)


def test_two_calls_are_bit_identical():
    from honerf_amd.mesh import marching_cubes
    vol = torch.from_numpy(noise_volume((40, 36, 32), seed=9)).cuda()
    a = marching_cubes(vol, 0.02)
    b = marching_cubes(vol, 0.02)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert torch.equal(a[1], b[1])


def test_runs_on_a_non_default_current_stream():
    from honerf_amd.mesh import marching_cubes
    vol_np = sphere_volume(96)
    ref = np_marching_cubes(vol_np, 0.0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        vol = torch.from_numpy(vol_np).cuda(non_blocking=False)
        vol = vol * 1.0                      # produced on the side stream itself
        v, tr = marching_cubes(vol, 0.0)
        vh, th = v.cpu(), tr.cpu()           # copies on the same stream
    s.synchronize()
    assert np.array_equal(th.numpy(), ref[1])
    assert np.abs(vh.numpy() - ref[0]).max() <= 4 * np.spacing(np.float32(96))


# ---- through the renderers ------------------------------------------------------------------------------------------------------
def _world(v, res, bmin, bmax):
    bmin = np.asarray(bmin, dtype=np.float32)
    bmax = np.asarray(bmax, dtype=np.float32)
    return v.astype(np.float64) / (res - 1.0) * (bmax - bmin)[None, :] + bmin[None, :]


def _check_native(extract_geometry, extract_fields, res, bmin, bmax, what):
    u = extract_fields()
    assert u.min() < 0 < u.max(), what                     # the box holds a piece of the surface
    thr = 0.0
    v, tr = extract_geometry(threshold=thr, mesher='native')
    assert isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape[1:] == (3,)
    assert isinstance(tr, np.ndarray) and tr.dtype == np.int64 and tr.shape[1:] == (3,)
    assert len(v) > 0, what
    rv, rt = np_marching_cubes(u, thr)
    assert np.array_equal(tr, rt), what
    bounded(what + ' world vertices', np.abs(v - _world(rv, res, bmin, bmax)).max(), 1e-6, kind='abs')
    with pytest.raises(ValueError):
        extract_geometry(threshold=thr, mesher='pymcubes')
    try:
        import mcubes  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='PyMCubes'):
            extract_geometry(threshold=thr)
    return v, tr


def test_single_renderer_object_field():
    from honerf_amd.renderer import NeuSRenderer
    m = product_modules()
    ren = NeuSRenderer(m['sdf_obj'], m['var_obj'], m['color_obj'], 'obj', 32, 0, 0, 4, 1.0)
    bmin, bmax = torch.tensor([-0.6, -0.5, -0.55]), torch.tensor([0.6, 0.55, 0.5])
    res = 48
    _check_native(lambda **k: ren.extract_geometry(bmin, bmax, res, None, None, None, None, **k),
                  lambda: ren.extract_fields(bmin, bmax, res), res, bmin.numpy(), bmax.numpy(), 'NeuSRenderer obj')


def _dual():
    from honerf_amd.renderer import NeuSRenderer_fitting
    m = product_modules()
    return NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)


def test_fitting_renderer_hand_mesh_and_ply(tmp_path):
    from honerf_amd import harness, synth
    bt, tp, j = synth.synth_hand_pose(3)
    bmin, bmax = j.min(0) - 0.08, j.max(0) + 0.08            # get_res.py's box around the hand
    res = 64
    dual = _dual()
    v, tr = _check_native(lambda **k: dual.extract_geometry(t(bmin), t(bmax), res, bt, tp, None, None, 'hand', **k),
                          lambda: dual.extract_fields(t(bmin), t(bmax), res, bt, tp, None, None, 'hand'), res, bmin, bmax, 'fitting hand')
    assert edge_stats(tr) == (0, 0)                           # watertight, consistently oriented
    p = str(tmp_path / '0_hand.ply')
    harness.write_ply(p, v, tr)
    v2, t2 = harness.read_ply(p)
    assert np.array_equal(t2, tr) and np.array_equal(v2, v.astype(np.float32))


def test_fitting_renderer_object_through_pose():
    from honerf_amd import synth
    from honerf_amd.renderer_batch import NeuSRenderer_fitting as Batched
    bt, tp, j = synth.synth_hand_pose(3)
    R, tt = synth.synth_obj_pose(2, center=tuple(j[9]))
    Ro, To = t(R).T.contiguous(), t(tt)
    c = j[9]
    bmin, bmax = c - 0.35, c + 0.35
    res = 64
    dual = _dual()
    _check_native(lambda **k: dual.extract_geometry(t(bmin), t(bmax), res, bt, tp, Ro, To, 'obj', **k),
                  lambda: dual.extract_fields(t(bmin), t(bmax), res, bt, tp, Ro, To, 'obj'), res, bmin, bmax, 'fitting obj')
    m = product_modules()
    batched = Batched(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)
    a = dual.extract_geometry(t(bmin), t(bmax), 32, bt, tp, Ro, To, 'obj', threshold=0.01, mesher='native')
    b = batched.extract_geometry(t(bmin), t(bmax), 32, bt, tp, Ro, To, 'obj', threshold=0.01, mesher='native')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
