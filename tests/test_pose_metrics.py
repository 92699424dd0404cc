"""The device pose metrics (hn_posemetric.hip through honerf_amd.pose_metrics) against the float64 restatement of
tests/test_pose_metrics_cpu.py: per-point nearest and paired distances, per-frame means and acceleration errors to 1e-6 m, the
15 mm flags exactly (with the count of reference values within 1e-5 m of the threshold recorded and asserted 0, and both outcomes
present in each column); odd sizes, 2-D inputs, the same bits on a repeated call, refusals; and producer to consumer: a two-frame
fit_frames_sharded run with fitting.pose_saver, its files, the restart, and tools/pose_eval.py on the tree.  No frame and no point
is filtered out of any comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import bounded, record
from test_pose_metrics_cpu import (SCENES, THRESHOLD, np_accel, np_accel_metrics, np_add, np_adds, np_nearest, np_pose_metrics, np_posed,
                                   pose_scene)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6          # m: the project's distance contract (tests/test_interaction.py)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max())


def check_method(what, got, ref):
    """One method's dict of pose_metrics against the restatement's."""
    for k in ('joint', 'ad', 'add', 'adds'):
        assert got[k].dtype == np.float64
        bounded('%s per-frame %s (m)' % (what, k), _err(got[k], ref[k]), TOL, kind='abs')
        bounded('%s mean %s (m)' % (what, k), abs(got[k + '_mean'] - ref[k + '_mean']), TOL, kind='abs')
    band = int((np.abs(np.concatenate([ref['add'], ref['adds']]) - THRESHOLD) < 1e-5).sum())
    record('%s reference values within 1e-5 m of the threshold' % what, band, 0, kind='count')
    assert band == 0, what
    for k in ('add_ok', 'adds_ok'):
        assert got[k].dtype == np.bool_ and np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
        assert ref[k].any() and not ref[k].all(), (what, k)          # both outcomes are exercised
        assert got[k[:-3] + '_rate'] == ref[k[:-3] + '_rate']


@pytest.mark.parametrize('V,F,seed', SCENES)
def test_scene_matches_the_restatement(V, F, seed):
    from honerf_amd import pose_metrics as pm
    model, pred, gt, init = pose_scene(V, F, seed)
    what = 'scene V %d F %d' % (V, F)
    ref = np_pose_metrics(model, pred, gt, init)
    both = pm.pose_metrics(model, pred, gt, init)
    assert sorted(both) == ['init', 'ours']
    check_method(what + ' ours', both['ours'], ref['ours'])
    check_method(what + ' init', both['init'], ref['init'])
    alone = pm.pose_metrics(model, pred, gt)                     # without init: the same numbers for 'ours', to the bit
    assert sorted(alone) == ['ours']
    for k, v in both['ours'].items():
        assert np.array_equal(alone['ours'][k], v) if isinstance(v, np.ndarray) else alone['ours'][k] == v, k
    # per point, on the posed float64 clouds (at camera distance: the general entry points centre them before rounding to fp32)
    g_v, p_v = np_posed(model, gt['Ro'], gt['To']), np_posed(model, pred['Ro'], pred['To'])
    nn = _np(pm.nearest_distance(g_v, p_v))
    assert nn.dtype == np.float32 and nn.shape == (F, V)
    bounded(what + ' per-point nearest distance (m)', _err(nn, np.stack([np_nearest(g_v[f], p_v[f]) for f in range(F)])), TOL, kind='abs')
    pd = _np(pm.paired_distance(p_v, g_v))
    bounded(what + ' per-point paired distance (m)', _err(pd, np.linalg.norm(p_v - g_v, axis=2)), TOL, kind='abs')
    # the single-metric entry points, on float64 and on float32 clouds
    for dt in (np.float64, np.float32):
        a, b = p_v.astype(dt), g_v.astype(dt)
        tag = '%s %s' % (what, np.dtype(dt).name)
        bounded(tag + ' add (m)', _err(_np(pm.add(a, b)), [np_add(a[f], b[f]) for f in range(F)]), TOL, kind='abs')
        bounded(tag + ' adds (m)', _err(_np(pm.adds(a, b)), [np_adds(a[f], b[f]) for f in range(F)]), TOL, kind='abs')
    bounded(what + ' joint_error (m)', _err(_np(pm.joint_error(pred['joint3d'], gt['joint3d'])), ref['ours']['joint']), TOL, kind='abs')


@pytest.mark.parametrize('V,F,seed', SCENES[:2])
def test_acceleration_error_matches_the_restatement(V, F, seed):
    from honerf_amd import pose_metrics as pm
    model, pred, gt, init = pose_scene(V, F, seed)
    what = 'accel V %d F %d' % (V, F)
    got = _np(pm.accel_error(gt['joint3d'], pred['joint3d']))
    assert got.dtype == np.float64 and got.shape == (F - 2,)
    bounded(what + ' joints (m)', _err(got, np_accel(gt['joint3d'], pred['joint3d'])), TOL, kind='abs')
    g_v, p_v = np_posed(model, gt['Ro'], gt['To']), np_posed(model, pred['Ro'], pred['To'])
    bounded(what + ' J = V vertices, float64 clouds (m)', _err(_np(pm.accel_error(g_v, p_v)), np_accel(g_v, p_v)), TOL, kind='abs')
    g32, p32 = g_v.astype(np.float32), p_v.astype(np.float32)
    bounded(what + ' J = V vertices, float32 clouds (m)', _err(_np(pm.accel_error(g32, p32)), np_accel(g32, p32)), TOL, kind='abs')
    vis = np.ones(F, dtype=bool)
    vis[F // 2] = False
    kept = _np(pm.accel_error(gt['joint3d'], pred['joint3d'], vis))
    assert kept.shape == (F - 2 - 3,)
    bounded(what + ' joints with a vis mask (m)', _err(kept, np_accel(gt['joint3d'], pred['joint3d'], vis)), TOL, kind='abs')
    assert np.array_equal(kept, _np(pm.accel_error(gt['joint3d'], pred['joint3d'], torch.from_numpy(vis))))
    acc = pm.accel_metrics(model, gt, {'ours': pred, 'init': init})
    ref = np_accel_metrics(model, gt, {'ours': pred, 'init': init})
    for name in ('ours', 'init'):
        for k in ('joint', 'vert'):
            assert acc[name][k].dtype == np.float64
            bounded('%s accel_metrics %s %s (m)' % (what, name, k), _err(acc[name][k], ref[name][k]), TOL, kind='abs')


@pytest.mark.parametrize('F,Nq,Nt', [(3, 1537, 4001), (1, 4001, 1537), (2, 1, 1), (1, 5000, 3), (5, 63, 513)])
def test_nearest_distance_at_odd_sizes(F, Nq, Nt):
    from honerf_amd.pose_metrics import nearest_distance
    r = np.random.RandomState(Nq + Nt)
    q = r.uniform(-0.1, 0.1, size=(F, Nq, 3)) + [0.02, -0.01, 0.9]
    t = r.uniform(-0.1, 0.1, size=(F, Nt, 3)) + [0.02, -0.01, 0.9]
    ref = np.stack([np_nearest(q[f], t[f]) for f in range(F)])
    what = 'nearest %d x %d against %d' % (F, Nq, Nt)
    d = nearest_distance(q, t)
    assert d.is_cuda and d.dtype == torch.float32 and tuple(d.shape) == (F, Nq)
    bounded(what + ' float64 numpy (m)', _err(_np(d), ref), TOL, kind='abs')
    # 2-D inputs are one frame
    bounded(what + ' 2-D (m)', _err(_np(nearest_distance(q[0], t[0])), ref[0]), TOL, kind='abs')
    # float32 tensors, on the host and on the device: against the restatement on the SAME float32 points
    q32, t32 = torch.from_numpy(q.astype(np.float32)), torch.from_numpy(t.astype(np.float32))
    ref32 = np.stack([np_nearest(q32[f].numpy(), t32[f].numpy()) for f in range(F)])
    bounded(what + ' float32 host tensors (m)', _err(_np(nearest_distance(q32, t32)), ref32), TOL, kind='abs')
    bounded(what + ' float32 device tensors (m)', _err(_np(nearest_distance(q32.cuda(), t32.cuda())), ref32), TOL, kind='abs')


def test_repeated_calls_give_the_same_bits():
    from honerf_amd import pose_metrics as pm
    model, pred, gt, init = pose_scene(1537, 7, 1)
    g_v, p_v = np_posed(model, gt['Ro'], gt['To']), np_posed(model, pred['Ro'], pred['To'])
    run = lambda: (_np(pm.nearest_distance(g_v, p_v)), _np(pm.paired_distance(p_v, g_v)), _np(pm.adds(p_v, g_v)),
                   _np(pm.accel_error(g_v, p_v)), pm.pose_metrics(model, pred, gt, init), pm.accel_metrics(model, gt, {'ours': pred}))
    a, b = run(), run()
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    for name in ('ours', 'init'):
        for k, v in a[4][name].items():
            assert v.tobytes() == b[4][name][k].tobytes() if isinstance(v, np.ndarray) else v == b[4][name][k], (name, k)
    for k in ('joint', 'vert'):
        assert a[5]['ours'][k].tobytes() == b[5]['ours'][k].tobytes()


def test_adds_keeps_the_reference_direction():
    """The tree is on pred and gt is queried: a pred that is a strict subset of gt scores > 0, the other way round 0."""
    from honerf_amd.pose_metrics import adds
    gt = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 2.0, 0], [0.0, 0, 4.0]])
    assert float(adds(gt[:2], gt)) == 1.5 and float(adds(gt, gt[:2])) == 0.0
    assert float(adds(gt, gt)) == 0.0


def test_refusals_raise_and_never_fault():
    from honerf_amd import lib, pose_metrics as pm
    model, pred, gt, init = pose_scene(300, 5, 3)
    g_v, p_v = np_posed(model, gt['Ro'], gt['To']), np_posed(model, pred['Ro'], pred['To'])
    empty = np.zeros((5, 0, 3))
    for fn in (pm.nearest_distance, pm.paired_distance, pm.add, pm.adds):
        with pytest.raises(ValueError):
            fn(empty, g_v)                                          # empty clouds
        with pytest.raises(ValueError):
            fn(g_v, empty)
        with pytest.raises(ValueError):
            fn(g_v[:4], p_v)                                        # mismatched frame counts
        with pytest.raises(ValueError):
            fn(g_v[0], p_v)                                         # a 2-D set against a 3-D one
        with pytest.raises(ValueError):
            fn(g_v.astype(np.float16), p_v)
        with pytest.raises(ValueError):
            fn(g_v[..., :2], p_v)
    with pytest.raises(ValueError, match='queries'):
        pm.nearest_distance(np.zeros((0, 7, 3)), np.zeros((0, 7, 3)))
    with pytest.raises(ValueError):
        pm.add(g_v[:, :10], p_v)                                    # paired sets of different sizes
    with pytest.raises(ValueError, match='at least 3'):
        pm.accel_error(g_v[:2], p_v[:2])                            # N = 2
    with pytest.raises(ValueError):
        pm.accel_error(g_v, p_v[:4])
    with pytest.raises(ValueError, match='vis'):
        pm.accel_error(g_v, p_v, np.ones(4, dtype=bool))
    with pytest.raises(ValueError, match='init'):
        pm.pose_metrics(model, pred, gt, {k: v[:3] for k, v in init.items()})
    with pytest.raises(ValueError, match='model_verts'):
        pm.pose_metrics(model[:0], pred, gt)
    with pytest.raises(ValueError, match='pred'):
        pm.pose_metrics(model, {'Ro': pred['Ro']}, gt)
    with pytest.raises(ValueError, match='at least 3'):
        pm.accel_metrics(model, {k: v[:2] for k, v in gt.items()}, {'ours': {k: v[:2] for k, v in pred.items()}})
    # the library itself: status codes with a message, before anything is launched
    L = lib.load()
    assert L.hn_pm_workspace_bytes(0, 10, 10) == 0 and L.hn_pm_workspace_bytes(1, -1, 10) == 0 and L.hn_pm_workspace_bytes(1, 10, 0) == 0
    assert L.hn_pm_workspace_bytes(1 << 20, 1 << 20, 10) == 0       # frames x queries beyond 2^31
    assert L.hn_pm_workspace_bytes(3, 1537, 4001) >= 4 * 3 * 1537
    x = torch.zeros(2, 8, 3, device='cuda')
    d = torch.zeros(2, 8, device='cuda')
    m = torch.zeros(8, dtype=torch.float64, device='cuda')
    ws = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    P, S = lib.ptr, lib.stream_ptr()
    calls = [L.hn_pm_nearest(None, 8, P(x), 8, 2, P(d), P(ws), 4096, S), L.hn_pm_nearest(P(x), 8, P(x), 8, 2, P(d), None, 4096, S),
             L.hn_pm_nearest(P(x), 8, P(x), 8, 2, P(d), P(ws), 8, S),               # a workspace smaller than the query sizes
             L.hn_pm_nearest(P(x), 0, P(x), 8, 2, P(d), P(ws), 4096, S), L.hn_pm_nearest(P(x), 8, P(x), 8, -1, P(d), P(ws), 4096, S),
             L.hn_pm_paired(P(x), None, 2, 8, P(d), S), L.hn_pm_paired(P(x), P(x), 2, 0, P(d), S),
             L.hn_pm_row_mean(None, 2, 8, P(m), S), L.hn_pm_row_mean(P(d), 0, 8, P(m), S),
             L.hn_pm_transform(P(x), 8, None, P(x), P(x), 2, P(x), S), L.hn_pm_transform(P(x), 0, P(x), P(x), P(x), 2, P(x), S),
             L.hn_pm_accel(P(x), P(x), 2, 8, P(m), S), L.hn_pm_accel(P(x), None, 3, 4, P(m), S), L.hn_pm_accel(P(x), P(x), 3, 0, P(m), S)]
    assert calls == [-1] * len(calls), calls
    assert L.hn_last_error()
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0 and float(m.abs().sum()) == 0.0      # nothing was written


def test_fit_to_pose_files_to_pose_eval(tmp_path):
    """Producer to consumer: fit_frames_sharded with fitting.pose_saver on the synthetic scene of tests/test_whole_step.py (two
    frames, two passes over the eight views), the files it leaves, the restart that skips them, and tools/pose_eval.py."""
    import bench
    from honerf_amd import fitting as F, harness
    dev = torch.device('cuda')
    ren, nets, _, _, _ = bench.build_fit(dev, 40, 1, bench.FIT_RAYS, 'f16x3', halo=True)
    gts, verts = {}, {}

    def make_frame(f):
        ch, jf, v = bench.build_fit_data(dev, 40 + f, 1, halo=True)
        # "ground truth": the frame's initial estimate moved by a centimetre (the fit itself is not what is under test)
        gts[f] = dict(joint3d=_np(ch.joints0[0]) + np.float32(0.01), Ro=_np(ch.Ro_pred[0]), To=_np(ch.To_pred[0]) + np.float32(0.01))
        verts[f] = _np(v)
        views = F.synthetic_views(8, 1, bench.FIT_RAYS, 40 + f, jf[9], device=dev)
        torch.manual_seed(9000 + f)
        return views, ch

    base = tmp_path / 'fit_res'
    seq = base / 'view_8' / '12' / 'p1_box' / 'seq0'
    saver = F.pose_saver(str(seq), '12', gt=lambda f: gts[f])
    out = F.fit_frames_sharded(ren, 2, make_frame, bench.NEAR, bench.FAR, '12', n_iters=2, done=saver.done, save=saver)
    assert out['frames'] == 2 and out['steps'] == 2 * 2 * 8
    poses = []
    for f in range(2):
        assert saver.done(f) and saver.path(f) == str(seq / 'pose_12' / ('%d.pickle' % f))
        p = harness.read_pose(saver.path(f))
        assert sorted(p) == ['gt_Ro', 'gt_To', 'gt_joint3d', 'pred_Ro', 'pred_To', 'pred_joint3d']
        assert p['pred_joint3d'].shape == (21, 3) and p['pred_Ro'].shape == (3, 3) and p['pred_To'].shape == (3,)
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in p.values())
        assert p['gt_To'].tobytes() == gts[f]['To'].astype(np.float32).tobytes()
        bounded('pose file %d: pred_Ro orthonormal' % f, np.abs(p['pred_Ro'].astype(np.float64) @ p['pred_Ro'].T - np.eye(3)).max(), 1e-5, kind='abs')
        assert 0 < np.abs(p['pred_To'] - p['gt_To']).max() < 0.05            # near the start, and not the ground truth itself
        poses.append(p)
    again = F.fit_frames_sharded(ren, 2, make_frame, bench.NEAR, bench.FAR, '12', n_iters=2, done=saver.done, save=saver)
    assert again['frames'] == 0 and again['steps'] == 0 and again['rank_frames'] == []
    # one object model for the class, as in the reference's tree (the chains' own vertex sets do not enter the pose files)
    models = tmp_path / 'models' / 'box_cppose'
    models.mkdir(parents=True)
    np.save(str(models / 'box_ours.npy'), verts[0])
    stack = lambda prefix: {k: np.stack([p[prefix + k] for p in poses]) for k in ('joint3d', 'Ro', 'To')}
    ref = np_pose_metrics(verts[0], stack('pred_'), stack('gt_'))['ours']
    torch.cuda.synchronize()
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'pose_eval.py'), str(base), '--view-num', '8', '--fit-type', '12',
                          '--models', str(tmp_path / 'models'), '--model-scale', '1.0'], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    line = 'ours joint: %.2lf, ours ad: %.2lf, ours add: %.2lf, ours adds: %.2lf' % (
        ref['joint_mean'] * 1000, ref['ad_mean'] * 1000, ref['add_rate'] * 100, ref['adds_rate'] * 100)
    assert 'obj_name box has 2 frames' in run.stdout, run.stdout
    assert line in run.stdout, (line, run.stdout)
    assert 'obj_name cup has 0 frames' in run.stdout
    assert ref['ad_mean'] > 0.01                                  # the centimetre the ground truth was moved by shows


def _run_tool(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'pose_eval.py')] + [str(a) for a in args], capture_output=True, text=True,
                         timeout=600, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout


def test_pose_eval_tool_with_init_and_accel(tmp_path):
    """tools/pose_eval.py on a tree written with harness.write_pose from the scene: the init columns (the reference's pickle + 4 x 4
    text files), a model in mm read from a PLY file, two sequences of one class, and --accel over the 12 / 123 / 1234 results."""
    import pickle
    from honerf_amd import harness
    V, F = 600, 7
    model, pred, gt, init = pose_scene(V, F, 1)
    base, models, init_dir = tmp_path / 'fit_res', tmp_path / 'models', tmp_path / 'init'
    (models / 'cup_cppose').mkdir(parents=True)
    mm = (model.astype(np.float64) * 1000.0).astype(np.float32)                 # the reference's models are in mm
    harness.write_ply(str(models / 'cup_cppose' / 'cup_ours.ply'), mm, np.array([[0, 1, 2]]))
    model_m = harness.read_ply(str(models / 'cup_cppose' / 'cup_ours.ply'))[0].astype(np.float64) * 0.001
    methods = {'12': ('pose_12', pred), '123': ('pose_4', init), '1234': ('pose_4', gt)}
    seqs = {'seq0': list(range(0, 4)), 'seq1': list(range(4, 7))}
    for fit, (sub, m) in methods.items():
        for seq, frames in seqs.items():
            d = base / 'view_8' / fit / 'p2_cup' / seq / sub
            d.mkdir(parents=True)
            for cid, f in enumerate(frames):
                harness.write_pose(str(d / ('%d.pickle' % cid)), m['joint3d'][f], m['Ro'][f], m['To'][f], gt['joint3d'][f], gt['Ro'][f], gt['To'][f])
    for seq, frames in seqs.items():
        dj, dp = init_dir / 'p2_cup' / seq / 'pred_joint3d_8view', init_dir / 'p2_cup' / seq / 'pred_objpose_8view'
        dj.mkdir(parents=True)
        dp.mkdir(parents=True)
        for cid, f in enumerate(frames):
            with open(str(dj / ('%d.pickle' % cid)), 'wb') as fh:
                pickle.dump({'pred_joint_3d': init['joint3d'][f].astype(np.float64)}, fh)
            P = np.eye(4)
            P[:3, :3], P[:3, 3] = init['Ro'][f], init['To'][f]
            np.savetxt(str(dp / ('%d.txt' % cid)), P, fmt='%.9e')            # 9 significant digits: a float32 survives the text
    ref = np_pose_metrics(model_m, pred, gt, init)
    o, i = ref['ours'], ref['init']
    out = _run_tool([base, '--view-num', 8, '--fit-type', 12, '--models', models, '--init', init_dir, '--classes', 'cup', 'box'])
    line = ('init joint: %.2lf, ours joint: %.2lf, init ad: %.2lf, init add: %.2lf, init adds: %.2lf, ours ad: %.2lf, ours add: %.2lf, '
            'ours adds: %.2lf' % (i['joint_mean'] * 1000, o['joint_mean'] * 1000, i['ad_mean'] * 1000, i['add_rate'] * 100, i['adds_rate'] * 100,
                                  o['ad_mean'] * 1000, o['add_rate'] * 100, o['adds_rate'] * 100))
    assert 'obj_name cup has %d frames' % F in out and 'obj_name box has 0 frames' in out, out
    assert line in out, (line, out)
    # --accel: per sequence (the second differences do not run across sequences), then the mean over all entries
    acc = {n: {'joint': [], 'vert': []} for n in ('12', '123', '1234')}
    for frames in seqs.values():
        sl = lambda m: {k: v[frames] for k, v in m.items()}
        r = np_accel_metrics(model_m, sl(gt), {n: sl(m) for n, (_, m) in methods.items()})
        for n in acc:
            acc[n]['joint'].append(r[n]['joint'])
            acc[n]['vert'].append(r[n]['vert'])
    mean = lambda n, k: float(np.concatenate(acc[n][k]).mean()) * 1000.0
    out = _run_tool([base, '--view-num', 8, '--models', models, '--accel'])
    line = ('acc_list_1_3_j: %.2lf, acc_list_1_3_v: %.2lf, acc_list_123_j: %.2lf,  acc_list_123_v: %.2lf,  acc_list_1234_j: %.2lf, '
            'acc_list_1234_v: %.2lf' % (mean('12', 'joint'), mean('12', 'vert'), mean('123', 'joint'), mean('123', 'vert'), mean('1234', 'joint'),
                                        mean('1234', 'vert')))
    assert out.splitlines()[0] == str(F), out
    assert line in out, (line, out)
    assert mean('1234', 'joint') == 0.0 and mean('12', 'vert') > 0.0
