"""A float64 numpy restatement of the reference's pose-accuracy scripts (analys_results/analys_hand_obj_pose.py and
analys_acc_err.py), pinned on cases worked by hand, the synthetic scene tests/test_pose_metrics.py holds the device to, and the
pose files (harness.write_pose / read_pose) those scripts read.  No GPU, and the reference is not imported."""
import pickle

import numpy as np
import pytest
from scipy.spatial import cKDTree

THRESHOLD = 0.015


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def np_add(pred_pts, gt_pts):
    """The mean over the points of |pred - gt|, row by row."""
    d = np.asarray(pred_pts, np.float64) - np.asarray(gt_pts, np.float64)
    return float(np.sqrt((d * d).sum(1)).mean())


def np_nearest(queries, targets):
    """The distance from every query to its nearest target (a k-d tree on the targets)."""
    return cKDTree(np.asarray(targets, np.float64)).query(np.asarray(queries, np.float64), k=1)[0]


def np_adds(pred_pts, gt_pts):
    """The tree is built on PRED and queried with GT: the mean over the gt points of the distance to the nearest pred point."""
    return float(np_nearest(gt_pts, pred_pts).mean())


def np_joint_error(pred_joints, gt_joints):
    return np_add(pred_joints, gt_joints)


def np_accel(gt, pred, vis=None):
    """[N, J, 3] x 2 -> the kept entries of [N - 2]: mean_j |(p[i] - 2 p[i+1] + p[i+2]) - (g[i] - 2 g[i+1] + g[i+2])|; an entry is
    dropped when frame i, i + 1 or i + 2 is invisible."""
    g, p = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    ag = g[:-2] - 2 * g[1:-1] + g[2:]
    ap = p[:-2] - 2 * p[1:-1] + p[2:]
    normed = np.linalg.norm(ap - ag, axis=2)
    if vis is None:
        keep = np.ones(len(normed), dtype=bool)
    else:
        inv = np.logical_not(np.asarray(vis, dtype=bool))
        keep = np.logical_not(inv[:-2] | inv[1:-1] | inv[2:])
    return normed[keep].mean(axis=1)


def np_posed(model, Ro, To):
    """[V, 3] through F poses -> float64 [F, V, 3] = v @ R^T + t, from the stored (float32) poses."""
    m, R, t = np.asarray(model, np.float64), np.asarray(Ro, np.float64), np.asarray(To, np.float64)
    return np.einsum('fij,vj->fvi', R, m) + t[:, None, :]


def np_pose_metrics(model, pred, gt, init=None, threshold=THRESHOLD):
    """Per method ('ours', and 'init' when given): per-frame joint, ad, add, adds, the strict < threshold flags and the means."""
    g_v = np_posed(model, gt['Ro'], gt['To'])
    out = {}
    for name, m in (('ours', pred), ('init', init)):
        if m is None:
            continue
        v = np_posed(model, m['Ro'], m['To'])
        F = len(v)
        joint = np.array([np_joint_error(m['joint3d'][f], gt['joint3d'][f]) for f in range(F)])
        ad = np.array([np_add(v[f], g_v[f]) for f in range(F)])
        ads = np.array([np_adds(v[f], g_v[f]) for f in range(F)])
        out[name] = dict(joint=joint, ad=ad, add=ad.copy(), adds=ads, add_ok=ad < threshold, adds_ok=ads < threshold,
                         joint_mean=float(joint.mean()), ad_mean=float(ad.mean()), add_mean=float(ad.mean()), adds_mean=float(ads.mean()),
                         add_rate=float((ad < threshold).mean()), adds_rate=float((ads < threshold).mean()))
    return out


def np_accel_metrics(model, gt, methods):
    g_v = np_posed(model, gt['Ro'], gt['To'])
    return {name: dict(joint=np_accel(gt['joint3d'], m['joint3d']), vert=np_accel(g_v, np_posed(model, m['Ro'], m['To'])))
            for name, m in methods.items()}


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
def rodrigues(axis, angle):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


SCENES = [(4000, 24, 0), (1537, 7, 1), (20000, 5, 2)]            # (V, F, seed)
SCENE_COUNTS = {(4000, 24, 0): (5, 9), (1537, 7, 1): (2, 3), (20000, 5, 2): (1, 3)}   # frames with ADD / ADD-S under 15 mm


def pose_scene(V, F, seed):
    """Points on an ellipsoid (semi-axes 8, 5, 3 cm) as the model; F ground-truth poses about 0.9 m from the origin; predictions whose
    rotation error grows to 0.6 rad and whose translation error grows to 8 cm over the frames, so that both flag columns hold both
    outcomes.  Everything is stored as float32.  Draw order: the model, every frame's ground-truth axis and angle, the ground-truth
    translations, the prediction's axes, its translation directions.  The joints and the `init` method (a second, worse
    prediction) come from generators of their own, so that they do not move those draws.
    -> (model [V, 3], pred, gt, init) with dicts of joint3d [F, 21, 3], Ro [F, 3, 3], To [F, 3]."""
    r = np.random.RandomState(seed)
    u = r.normal(size=(V, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    model = (u * np.array([0.08, 0.05, 0.03])).astype(np.float32)
    Rg = np.stack([rodrigues(r.normal(size=3), r.uniform(0, np.pi)) for _ in range(F)])
    tg = np.stack([np.array([0.02, -0.01, 0.9]) + 0.05 * r.normal(size=3) for _ in range(F)])
    ang = np.linspace(0, 0.6, F)
    Rp = np.stack([rodrigues(r.normal(size=3), ang[f]) @ Rg[f] for f in range(F)])
    off = np.linspace(0, 0.08, F)
    tp = []
    for f in range(F):
        d = r.normal(size=3)
        tp.append(tg[f] + d / np.linalg.norm(d) * off[f])
    tp = np.stack(tp)
    rj = np.random.RandomState(seed + 1000)
    gj = tg[:, None, :] + 0.05 * rj.normal(size=(F, 21, 3))
    pj = gj + 0.008 * rj.normal(size=(F, 21, 3))
    ri = np.random.RandomState(seed + 2000)
    Ri = np.stack([rodrigues(ri.normal(size=3), 0.05) @ Rg[f] for f in range(F)])
    di = ri.normal(size=(F, 3))
    ti = tg + di / np.linalg.norm(di, axis=1, keepdims=True) * np.where(np.arange(F) % 2 == 0, 0.005, 0.045)[:, None]  # 5 mm, 45 mm, ..
    ij = gj + 0.02 * ri.normal(size=(F, 21, 3))
    f32 = lambda *a: [np.ascontiguousarray(x, dtype=np.float32) for x in a]
    pred = dict(zip(('joint3d', 'Ro', 'To'), f32(pj, Rp, tp)))
    gt = dict(zip(('joint3d', 'Ro', 'To'), f32(gj, Rg, tg)))
    init = dict(zip(('joint3d', 'Ro', 'To'), f32(ij, Ri, ti)))
    return model, pred, gt, init


# ---- the restatement on cases worked by hand ----------------------------------------------------------------------------------------
def _cloud(n, seed):
    return np.random.RandomState(seed).uniform(-0.1, 0.1, size=(n, 3))


def test_add_of_a_pure_translation_is_its_length():
    p = _cloud(500, 0)
    d = np.array([0.003, -0.004, 0.012])                  # |d| = 0.013 exactly
    assert np_add(p + d, p) == pytest.approx(0.013, abs=1e-15)
    assert np_add(p, p) == 0.0


def test_adds_of_a_set_against_itself_is_zero():
    p = _cloud(500, 1)
    assert np_adds(p, p) == 0.0
    assert np_adds(p[::-1], p) == 0.0                     # the order of the points does not matter


def test_adds_is_asymmetric_when_pred_is_a_strict_subset_of_gt():
    gt = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 2.0, 0], [0.0, 0, 4.0]])
    pred = gt[:2]
    # the tree on pred, gt queried: the distances are 0, 0, 2 (to the origin), 4 (to the origin)
    assert np_adds(pred, gt) == pytest.approx((0 + 0 + 2 + 4) / 4.0, abs=1e-15)
    assert np_adds(gt, pred) == 0.0                        # the other way round every query finds itself


def test_acceleration_error_of_a_constant_velocity_track_is_zero():
    r = np.random.RandomState(2)
    gt = r.normal(size=(9, 21, 3))
    v = r.normal(size=(1, 21, 3))
    pred = gt + np.arange(9)[:, None, None] * v + r.normal(size=(1, 21, 3))     # a constant velocity and offset on top of gt
    assert np.abs(np_accel(gt, pred)).max() < 1e-13
    assert np_accel(gt, pred).shape == (7,)
    # a quadratic term a i^2 / 2 has the second difference a: the error is the mean norm of a
    a = r.normal(size=(21, 3))
    quad = gt + 0.5 * (np.arange(9) ** 2)[:, None, None] * a[None]
    assert np.allclose(np_accel(gt, quad), np.linalg.norm(a, axis=1).mean(), rtol=0, atol=1e-12)


def test_vis_mask_drops_the_three_entries_around_an_invisible_frame():
    r = np.random.RandomState(3)
    gt, pred = r.normal(size=(10, 5, 3)), r.normal(size=(10, 5, 3))
    full = np_accel(gt, pred)
    vis = np.ones(10, dtype=bool)
    vis[5] = False
    kept = np_accel(gt, pred, vis)
    assert kept.shape == (5,)                              # entries 3, 4, 5 (frames 3..5, 4..6, 5..7) are gone
    assert np.array_equal(kept, full[[0, 1, 2, 6, 7]])
    vis = np.ones(10, dtype=bool)
    vis[9] = False                                         # the last frame touches only the last entry: no wrap-around to entry 0
    assert np.array_equal(np_accel(gt, pred, vis), full[:7])
    vis = np.ones(10, dtype=bool)
    vis[0] = False
    assert np.array_equal(np_accel(gt, pred, vis), full[1:])


@pytest.mark.parametrize('V,F,seed', SCENES)
def test_scene_exercises_both_outcomes_away_from_the_threshold(V, F, seed):
    model, pred, gt, init = pose_scene(V, F, seed)
    assert model.dtype == np.float32 and model.shape == (V, 3) and pred['Ro'].shape == (F, 3, 3)
    ref = np_pose_metrics(model, pred, gt, init)
    o = ref['ours']
    assert (int(o['add_ok'].sum()), int(o['adds_ok'].sum())) == SCENE_COUNTS[(V, F, seed)]
    for name in ('ours', 'init'):
        vals = np.concatenate([ref[name]['add'], ref[name]['adds']])
        assert np.abs(vals - THRESHOLD).min() > 4e-4, (name, np.abs(vals - THRESHOLD).min())
    for col in ('add_ok', 'adds_ok'):
        assert o[col].any() and not o[col].all()
    assert np.array_equal(o['ad'], o['add']) and (o['adds'] <= o['add'] + 1e-15).all()


def test_accel_metrics_restatement_shapes():
    model, pred, gt, init = pose_scene(300, 7, 1)
    acc = np_accel_metrics(model, gt, {'ours': pred, 'init': init, 'gt': gt})
    assert acc['ours']['joint'].shape == acc['ours']['vert'].shape == (5,)
    assert np.abs(acc['gt']['joint']).max() == 0.0 and np.abs(acc['gt']['vert']).max() == 0.0


# ---- the pose files ------------------------------------------------------------------------------------------------------------------
KEYS = ['pred_joint3d', 'pred_Ro', 'pred_To', 'gt_joint3d', 'gt_Ro', 'gt_To']


def _pose_arrays(seed):
    r = np.random.RandomState(seed)
    return [r.normal(size=s).astype(np.float32) for s in ((21, 3), (3, 3), (3,), (21, 3), (3, 3), (3,))]


def test_pose_file_round_trips_the_six_arrays_bit_for_bit(tmp_path):
    from honerf_amd import harness
    arrs = _pose_arrays(0)
    path = str(tmp_path / '7.pickle')
    harness.write_pose(path, *arrs)
    got = harness.read_pose(path)
    assert sorted(got) == sorted(KEYS)
    for k, a in zip(KEYS, arrs):
        assert got[k].dtype == np.float32 and got[k].shape == a.shape and got[k].tobytes() == a.tobytes(), k
    with open(path, 'rb') as f:                             # what the reference's scripts do with the file
        raw = pickle.load(f)
    assert isinstance(raw, dict) and sorted(raw) == sorted(KEYS)
    assert all(type(v) is np.ndarray and v.dtype == np.float32 for v in raw.values())


def test_pose_file_without_ground_truth_has_the_pred_keys_only(tmp_path):
    import torch
    from honerf_amd import harness
    arrs = _pose_arrays(1)
    path = str(tmp_path / '0.pickle')
    # tensors, float64, and a leading frame axis of one are taken too; the file holds float32 [21, 3], [3, 3], [3]
    harness.write_pose(path, torch.from_numpy(arrs[0])[None].double(), arrs[1][None], torch.from_numpy(arrs[2]))
    got = harness.read_pose(path)
    assert sorted(got) == sorted(KEYS[:3])
    for k, a in zip(KEYS[:3], arrs[:3]):
        assert got[k].dtype == np.float32 and got[k].tobytes() == a.tobytes(), k
    with pytest.raises(ValueError, match='go together'):
        harness.write_pose(path, *arrs[:3], gt_Ro=arrs[4])
    with pytest.raises(ValueError, match='pred_Ro'):
        harness.write_pose(path, arrs[0], arrs[1][:2], arrs[2])


def test_pose_file_lacking_pred_Ro_is_refused(tmp_path):
    from honerf_amd import harness
    arrs = _pose_arrays(2)
    path = str(tmp_path / 'bad.pickle')
    with open(path, 'wb') as f:
        pickle.dump({k: a for k, a in zip(KEYS, arrs) if k != 'pred_Ro'}, f)
    with pytest.raises(ValueError, match='pred_Ro'):
        harness.read_pose(path)
    with open(path, 'wb') as f:
        pickle.dump([1, 2, 3], f)
    with pytest.raises(ValueError, match='not a pose file'):
        harness.read_pose(path)


def test_pose_saver_names_its_files(tmp_path):
    from honerf_amd import fitting
    saver = fitting.pose_saver(str(tmp_path), '12', name=lambda f: '%04d' % f)
    assert saver.path(3) == str(tmp_path / 'pose_12' / '0003.pickle')
    assert not saver.done(3)
