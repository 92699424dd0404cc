"""Pose-accuracy metrics on the device (hn_posemetric.hip): analys_results/analys_hand_obj_pose.py and analys_acc_err.py without
scipy, batched over the frames.

The reference scores the pose pickles of fitting_single.py (`harness.write_pose` writes them) frame by frame on the CPU:
  joint  the mean over the 21 joints of |pred - gt| (analys_hand_obj_pose.py:97);
  ad     the mean over the object model's vertices of |(R_pred v + t_pred) - (R_gt v + t_gt)| (:102-106);
  add    the same number (`add`, :17-19), counted when < 15 mm (:111-113);
  adds   `adi` (:21-25): a cKDTree on the PREDICTED vertices queried with the GROUND-TRUTH vertices, the mean over the gt vertices of
         the distance to the nearest predicted vertex, counted when < 15 mm.  The direction matters once the two sets differ (a
         prediction that covers only part of the object scores badly, one that adds points far away does not): it is kept;
  accel  compute_error_accel (analys_acc_err.py:22-49): the mean over the points of the norm of the difference of the second
         differences p[i] - 2 p[i+1] + p[i+2] of prediction and ground truth, per entry i.
DESIGN.md 3.15 is the contract.  Here the posed clouds are evaluated in fp64 and stored in fp32 RELATIVE TO THE FRAME'S GROUND-TRUTH
TRANSLATION (object-sized coordinates: ulp 7e-9 m instead of 6e-8 m at camera distance), the nearest-point search is brute force
over all pairs of a frame, and the means are accumulated in fp64.

Arguments are numpy arrays or torch tensors, on either device, float32 or float64; they are moved to the current CUDA device.
`nearest_distance`, `paired_distance`, `add`, `adds`, `joint_error` and `accel_error` return device tensors; `pose_metrics` and
`accel_metrics`, the summaries, read everything back once and return numpy arrays and floats.

The benchmarks' aligned numbers (FreiHAND / HO-3D / DexYCB): `pa_joint_error` and `pa_add` score the prediction after a
similarity Procrustes onto the ground truth (`alignment.procrustes`), `pck_auc` is the PCK curve and its area, `hand_metrics` the
summary of both, raw and aligned.
"""
import numpy as np
import torch

from . import lib as _lib
from .interaction import _check, _device

_FLOATS = (torch.float32, torch.float64)


def _tensor(x, what, tail, dims, dtypes=_FLOATS):
    """x -> a detached tensor on the current device; its rank must be one of dims and its last axes `tail`."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError('%s: expected a numpy array or a torch tensor, got %s' % (what, type(x).__name__))
    if x.dtype not in dtypes:
        raise ValueError('%s: dtype %s, expected one of %s' % (what, x.dtype, ', '.join(str(d) for d in dtypes)))
    if x.dim() not in dims or tuple(x.shape[x.dim() - len(tail):]) != tuple(tail):
        raise ValueError('%s: shape %s, expected %s axes ending in [%s]' % (what, tuple(x.shape), ' or '.join(str(d) for d in dims),
                                                                            ', '.join(str(d) for d in tail)))
    if x.numel() == 0:
        raise ValueError('%s: shape %s is empty' % (what, tuple(x.shape)))
    return x.detach().to(_device())


def _clouds(a, b, what_a, what_b, same_points):
    """Two point sets [F, N, 3] or [N, 3] (both of one rank) -> ([F, Na, 3], [F, Nb, 3], was 2-D)."""
    a, b = _tensor(a, what_a, (3,), (2, 3)), _tensor(b, what_b, (3,), (2, 3))
    if a.dim() != b.dim():
        raise ValueError('%s is %d-D and %s is %d-D: pass both as [N, 3] or both as [F, N, 3]' % (what_a, a.dim(), what_b, b.dim()))
    flat = a.dim() == 2
    if flat:
        a, b = a[None], b[None]
    if a.shape[0] != b.shape[0]:
        raise ValueError('%s has %d frames and %s has %d' % (what_a, a.shape[0], what_b, b.shape[0]))
    if same_points and a.shape[1] != b.shape[1]:
        raise ValueError('%s has %d points per frame and %s has %d' % (what_a, a.shape[1], what_b, b.shape[1]))
    return a, b, flat


def _centred(a, b):
    """Both sets relative to b's first point of each frame, formed in float64 and rounded once to fp32 (distances are unchanged)."""
    c = b[:, :1].double()
    return (a.double() - c).float().contiguous(), (b.double() - c).float().contiguous()


def _pair_inputs(a, b):
    """What the kernels that take their differences in fp64 are handed: fp32 sets as they are (nothing is lost), else centred."""
    if a.dtype == b.dtype == torch.float32:
        return a.contiguous(), b.contiguous()
    return _centred(a, b)


# ---- private passes on checked fp32 device tensors -----------------------------------------------------------------------------------
def _nearest(q, t, ws=None):
    """q [F, Nq, 3], t [F, Nt, 3] fp32 contiguous -> [F, Nq] fp32."""
    F, Nq, Nt = q.shape[0], q.shape[1], t.shape[1]
    L = _lib.load()
    with torch.cuda.device(q.device):
        need = int(L.hn_pm_workspace_bytes(F, Nq, Nt))
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=q.device)
        d = torch.empty(F, Nq, dtype=torch.float32, device=q.device)
        _check(L.hn_pm_nearest(_lib.ptr(q), Nq, _lib.ptr(t), Nt, F, _lib.ptr(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'nearest_distance')
    return d


def _paired(a, b):
    F, N = a.shape[0], a.shape[1]
    with torch.cuda.device(a.device):
        d = torch.empty(F, N, dtype=torch.float32, device=a.device)
        _check(_lib.load().hn_pm_paired(_lib.ptr(a), _lib.ptr(b), F, N, _lib.ptr(d), _lib.stream_ptr()), 'paired distance')
    return d


def _row_mean(x):
    F, N = x.shape
    with torch.cuda.device(x.device):
        m = torch.empty(F, dtype=torch.float64, device=x.device)
        _check(_lib.load().hn_pm_row_mean(_lib.ptr(x), F, N, _lib.ptr(m), _lib.stream_ptr()), 'row mean')
    return m


def _transform(verts, R, t, c, out=None):
    """verts [V, 3], R [K, 3, 3], t, c [K, 3] fp32 contiguous -> [K, V, 3] fp32 = R_k v + t_k - c_k."""
    K, V = R.shape[0], verts.shape[0]
    with torch.cuda.device(verts.device):
        if out is None:
            out = torch.empty(K, V, 3, dtype=torch.float32, device=verts.device)
        _check(_lib.load().hn_pm_transform(_lib.ptr(verts), V, _lib.ptr(R), _lib.ptr(t), _lib.ptr(c), K, _lib.ptr(out), _lib.stream_ptr()),
               'pose transform')
    return out


def _accel(gt, pred):
    N, J = gt.shape[0], gt.shape[1]
    with torch.cuda.device(gt.device):
        out = torch.empty(max(N - 2, 0), dtype=torch.float64, device=gt.device)
        _check(_lib.load().hn_pm_accel(_lib.ptr(gt), _lib.ptr(pred), N, J, _lib.ptr(out), _lib.stream_ptr()), 'accel_error')
    return out


def _f32(x):
    return x.to(torch.float32).contiguous()


# ---- public queries ------------------------------------------------------------------------------------------------------------------
def nearest_distance(queries, targets):
    """The Euclidean distance from every query to the nearest target of the same frame: queries [F, Nq, 3], targets [F, Nt, 3] ->
    float32 [F, Nq] on the device ([Nq, 3], [Nt, 3] -> [Nq]).  Brute force over all pairs: exact, no index, no tie rule."""
    q, t, flat = _clouds(queries, targets, 'queries', 'targets', same_points=False)
    d = _nearest(*_centred(q, t))
    return d[0] if flat else d


def paired_distance(a, b):
    """|a - b| row by row: [F, N, 3] x 2 -> float32 [F, N] on the device ([N, 3] x 2 -> [N])."""
    a, b, flat = _clouds(a, b, 'a', 'b', same_points=True)
    d = _paired(*_pair_inputs(a, b))
    return d[0] if flat else d


def add(pred_pts, gt_pts):
    """`add` (analys_hand_obj_pose.py:17-19) per frame: the mean over the points of |pred - gt|, row by row -> float64 [F] on the
    device (a 0-d tensor for [N, 3] inputs)."""
    p, g, flat = _clouds(pred_pts, gt_pts, 'pred_pts', 'gt_pts', same_points=True)
    m = _row_mean(_paired(*_pair_inputs(p, g)))
    return m[0] if flat else m


def adds(pred_pts, gt_pts):
    """`adi` (analys_hand_obj_pose.py:21-25) per frame -> float64 [F] on the device.  The reference builds its tree on PRED and queries
    GT: this is the mean over the gt points of the distance to the nearest pred point, NOT the other way round; the two differ as
    soon as the sets do (a pred that is a strict subset of gt scores > 0, a gt that is a strict subset of pred scores 0)."""
    p, g, flat = _clouds(pred_pts, gt_pts, 'pred_pts', 'gt_pts', same_points=False)
    pc, gc = _centred(p, g)
    m = _row_mean(_nearest(gc, pc))
    return m[0] if flat else m


def joint_error(pred_joints, gt_joints):
    """The mean joint distance per frame (analys_hand_obj_pose.py:97): [F, J, 3] x 2 -> float64 [F] on the device."""
    p, g, flat = _clouds(pred_joints, gt_joints, 'pred_joints', 'gt_joints', same_points=True)
    m = _row_mean(_paired(*_pair_inputs(p, g)))
    return m[0] if flat else m


def _pa_distances(pred, gt, what_p, what_g):
    """Per-point distances after the similarity Procrustes of pred onto gt, frame by frame -> (fp32 [F, N], the aligned pred and gt as
    the kernels saw them (fp32; relative to gt's first point for float64 inputs), was 2-D)."""
    from .alignment import procrustes
    p, g, flat = _clouds(pred, gt, what_p, what_g, same_points=True)
    p32, g32 = _pair_inputs(p, g)
    aligned = procrustes(p32, g32, scale=True)['aligned']
    return _paired(aligned, g32), aligned, g32, flat


def pa_joint_error(pred_joints, gt_joints):
    """PA-MPJPE per frame: the mean joint distance after the similarity Procrustes (rotation, scale, translation) of the prediction onto
    the ground truth: [F, J, 3] x 2 -> float64 [F] on the device (a 0-d tensor for [J, 3] inputs)."""
    d, _, _, flat = _pa_distances(pred_joints, gt_joints, 'pred_joints', 'gt_joints')
    m = _row_mean(d)
    return m[0] if flat else m


def pa_add(pred_pts, gt_pts):
    """`add` after the similarity Procrustes of pred onto gt (PA-MPVPE for hand vertices): [F, N, 3] x 2 -> float64 [F] on the device."""
    d, _, _, flat = _pa_distances(pred_pts, gt_pts, 'pred_pts', 'gt_pts')
    m = _row_mean(d)
    return m[0] if flat else m


def _thresholds(lo, hi, steps):
    lo, hi, steps = float(lo), float(hi), int(steps)
    if not hi > lo or steps < 2:
        raise ValueError('pck_auc: thresholds lo = %r, hi = %r, steps = %r: hi > lo and at least 2 steps' % (lo, hi, steps))
    return np.linspace(lo, hi, steps)


def _pck_counts(errors, thr):
    """errors: a device tensor of any shape, thr float64 numpy [K] -> int64 [K] on the device: the entries <= each threshold."""
    e = errors.reshape(-1).double()
    t = torch.from_numpy(thr).to(e.device)
    counts = torch.zeros(len(thr), dtype=torch.int64, device=e.device)
    for s in range(0, e.shape[0], 1 << 20):                          # (1M entries x K thresholds of booleans at a time)
        counts += (e[s:s + (1 << 20), None] <= t[None]).sum(0)
    return counts


def _auc(pck, thr):
    return float(((pck[1:] + pck[:-1]) * 0.5 * np.diff(thr)).sum() / (thr[-1] - thr[0]))


def pck_auc(errors, lo=0.0, hi=0.05, steps=100):
    """The PCK curve of FreiHAND's evaluation and the area under it: thresholds = linspace(lo, hi, steps), pck[k] = the fraction of ALL
    entries of `errors` (distances, any shape, metres) <= thresholds[k], auc = the trapezoid sum of pck over the thresholds / (hi -
    lo).  -> dict(thresholds, pck: float64 numpy [steps]; auc: float; count: int64 numpy [steps]).  The counts are integers: exact."""
    if isinstance(errors, np.ndarray):
        errors = torch.from_numpy(np.ascontiguousarray(errors))
    if not isinstance(errors, torch.Tensor) or errors.dtype not in _FLOATS or errors.numel() == 0:
        raise ValueError('errors: expected a non-empty float32 or float64 numpy array or torch tensor')
    thr = _thresholds(lo, hi, steps)
    e = errors.detach().to(_device())
    count = _pck_counts(e, thr).cpu().numpy()
    pck = count / float(e.numel())
    return dict(thresholds=thr, pck=pck, auc=_auc(pck, thr), count=count)


def _fscore_counts(a, b, taus):
    """a, b fp32 [F, N, 3] / [F, M, 3] -> float64 [2 len(taus), F]: per tau the a points within tau of b, then the b points within tau of a."""
    da, db = _nearest(a, b), _nearest(b, a)
    rows = []
    for t in taus:
        rows += [(da.double() <= t).sum(1).double(), (db.double() <= t).sum(1).double()]
    return torch.stack(rows)


def hand_metrics(pred_joints, gt_joints, pred_verts=None, gt_verts=None, lo=0.0, hi=0.05, steps=100):
    """The hand benchmarks' table for F frames: mpjpe and pa_mpjpe (the mean over frames and joints of the joint distance, raw and after
    the per-frame similarity Procrustes), auc and pa_auc (`pck_auc` of all F x J joint distances, raw and aligned), and with vertices
    [F, V, 3] mpvpe, pa_mpvpe, f5, f15: the mean over the frames of the F-score at 5 mm and 15 mm between the ALIGNED predicted
    vertices and the ground truth's as point sets (`nearest_distance` both ways: precision = the share of aligned vertices within tau of
    a gt vertex, recall the other way round, 2 p r / (p + r), 0 when both are 0).  Metres; Python floats; one read-back."""
    if (pred_verts is None) != (gt_verts is None):
        raise ValueError('pred_verts and gt_verts: pass both or neither')
    thr = _thresholds(lo, hi, steps)
    K = len(thr)
    pj, gj, _ = _clouds(pred_joints, gt_joints, 'pred_joints', 'gt_joints', same_points=True)
    d_raw = _paired(*_pair_inputs(pj, gj))
    d_pa = _pa_distances(pj, gj, 'pred_joints', 'gt_joints')[0]
    F = d_raw.shape[0]
    parts = [_row_mean(d_raw).mean()[None], _row_mean(d_pa).mean()[None], _pck_counts(d_raw, thr).double(), _pck_counts(d_pa, thr).double()]
    if pred_verts is not None:
        pv, gv, _ = _clouds(pred_verts, gt_verts, 'pred_verts', 'gt_verts', same_points=True)
        if pv.shape[0] != F:
            raise ValueError('pred_verts has %d frames and pred_joints has %d' % (pv.shape[0], F))
        v_raw = _paired(*_pair_inputs(pv, gv))
        v_pa, aligned, g32, _ = _pa_distances(pv, gv, 'pred_verts', 'gt_verts')
        parts += [_row_mean(v_raw).mean()[None], _row_mean(v_pa).mean()[None], _fscore_counts(aligned, g32, (0.005, 0.015)).reshape(-1)]
    host = torch.cat(parts).cpu().numpy()                             # the one read-back
    n = float(d_raw.numel())
    out = dict(mpjpe=float(host[0]), pa_mpjpe=float(host[1]), auc=_auc(host[2:2 + K] / n, thr), pa_auc=_auc(host[2 + K:2 + 2 * K] / n, thr))
    if pred_verts is not None:
        o = 2 + 2 * K
        V = float(v_raw.shape[1])
        c = host[o + 2:].reshape(4, F) / V
        fs = lambda p, r: float(np.where(p + r > 0, 2.0 * p * r / np.where(p + r > 0, p + r, 1.0), 0.0).mean())
        out.update(mpvpe=float(host[o]), pa_mpvpe=float(host[o + 1]), f5=fs(c[0], c[1]), f15=fs(c[2], c[3]))
    return out


def _vis_keep(vis, n):
    """compute_error_accel's mask (analys_acc_err.py:40-47): entry i is dropped when frame i, i + 1 or i + 2 is invisible (the np.roll
    wrap-around is cut off by its [:-2]: a plain shifted OR)."""
    v = torch.as_tensor(np.asarray(vis.detach().cpu() if isinstance(vis, torch.Tensor) else vis)).reshape(-1).bool()
    if v.shape[0] != n:
        raise ValueError('vis: %d entries for %d frames' % (v.shape[0], n))
    inv = ~v
    return ~(inv[:-2] | inv[1:-1] | inv[2:])


def accel_error(gt, pred, vis=None):
    """compute_error_accel (analys_acc_err.py:22-49): gt, pred [N, J, 3] (N >= 3 frames of J points) -> float64 [N - 2] on the device,
    without the entries `vis` (bool [N]) drops."""
    g = _tensor(gt, 'gt', (3,), (3,))
    p = _tensor(pred, 'pred', (3,), (3,))
    if g.shape != p.shape:
        raise ValueError('gt is %s and pred is %s' % (tuple(g.shape), tuple(p.shape)))
    if g.shape[0] < 3:
        raise ValueError('gt: %d frames, the second difference needs at least 3' % g.shape[0])
    keep = None if vis is None else _vis_keep(vis, g.shape[0])
    # float64 input: relative to the ground truth's first point of each frame, the same origin for both, so that the difference of
    # the second differences is unchanged and the fp32 coordinates are as small as the scene allows
    out = _accel(*reversed(_pair_inputs(p, g)))
    return out if keep is None else out[keep.to(out.device)]


def _pose(d, what, n_frames=None):
    if not isinstance(d, dict) or not all(k in d for k in ('joint3d', 'Ro', 'To')):
        raise ValueError("%s: expected a dict with 'joint3d' [F, 21, 3], 'Ro' [F, 3, 3], 'To' [F, 3]" % what)
    j = _tensor(d['joint3d'], what + " 'joint3d'", (21, 3), (3,))
    R = _tensor(d['Ro'], what + " 'Ro'", (3, 3), (3,))
    t = _tensor(d['To'], what + " 'To'", (3,), (2,))
    F = j.shape[0] if n_frames is None else n_frames
    for name, x in (('joint3d', j), ('Ro', R), ('To', t)):
        if x.shape[0] != F:
            raise ValueError("%s '%s' has %d frames, expected %d" % (what, name, x.shape[0], F))
    return _f32(j), _f32(R), _f32(t)


def _model(model_verts):
    return _f32(_tensor(model_verts, 'model_verts', (3,), (2,)))


def pose_metrics(model_verts, pred, gt, init=None, threshold=0.015):
    """The per-frame numbers of analys_hand_obj_pose.py:82-122 for all frames at once.  model_verts [V, 3] (metres); pred, gt and
    init are dicts of 'joint3d' [F, 21, 3], 'Ro' [F, 3, 3], 'To' [F, 3] (the arrays of the pose pickles, stacked).  Returns
    {'ours': m[, 'init': m]} with m = dict of float64 numpy arrays [F] 'joint', 'ad', 'add' (= 'ad', as in the reference), 'adds',
    bool arrays 'add_ok' / 'adds_ok' (< threshold, strictly), and floats 'joint_mean', 'ad_mean', 'add_mean', 'adds_mean' (metres),
    'add_rate', 'adds_rate' (the fraction of frames under the threshold).

    One batched pass: the posed clouds of every method and of the ground truth (relative to the ground truth's translation) are
    written into one workspace, scored, and dropped; one read-back at the end."""
    verts = _model(model_verts)
    gj, gR, gt_t = _pose(gt, 'gt')
    F, V = gj.shape[0], verts.shape[0]
    methods = [('ours', _pose(pred, 'pred', F))] + ([('init', _pose(init, 'init', F))] if init is not None else [])
    M = len(methods)
    dev = verts.device
    L = _lib.load()
    with torch.cuda.device(dev):
        cloud_bytes = 2 * M * F * V * 3 * 4
        nn_bytes = int(L.hn_pm_workspace_bytes(M * F, V, V))
        if nn_bytes == 0:
            raise ValueError('pose_metrics: %d methods x %d frames x %d vertices is beyond what one call takes' % (M, F, V))
        ws = torch.empty(cloud_bytes + 256 + nn_bytes, dtype=torch.uint8, device=dev)
        clouds = ws[:cloud_bytes].view(torch.float32).view(2 * M * F, V, 3)
        nn_ws = ws[(cloud_bytes + 255) // 256 * 256:]
        # rows [0, M F): the methods' clouds; rows [M F, 2 M F): the ground truth's, once per method
        R = torch.cat([m[1][1] for m in methods] + [gR] * M).contiguous()
        t = torch.cat([m[1][2] for m in methods] + [gt_t] * M).contiguous()
        c = gt_t.repeat(2 * M, 1).contiguous()
        _transform(verts, R, t, c, out=clouds)
        p_cl, g_cl = clouds[:M * F], clouds[M * F:]
        ad = _row_mean(_paired(p_cl, g_cl))
        ads = _row_mean(_nearest(g_cl, p_cl, nn_ws))              # the "tree" on pred, queried with gt
        joint = _row_mean(_paired(torch.cat([m[1][0] for m in methods]).contiguous(), gj.repeat(M, 1, 1).contiguous()))
        host = torch.stack([joint, ad, ads]).cpu().numpy().reshape(3, M, F)
    del clouds, p_cl, g_cl, nn_ws, ws
    out = {}
    for k, (name, _) in enumerate(methods):
        j, a, s = host[0, k], host[1, k], host[2, k]
        out[name] = dict(joint=j, ad=a, add=a.copy(), adds=s, add_ok=a < threshold, adds_ok=s < threshold, joint_mean=float(j.mean()),
                         ad_mean=float(a.mean()), add_mean=float(a.mean()), adds_mean=float(s.mean()),
                         add_rate=float((a < threshold).mean()), adds_rate=float((s < threshold).mean()))
    return out


def accel_metrics(model_verts, gt, methods):
    """get_acc_list's numbers (analys_acc_err.py:114-120) for one sequence: gt and every value of the dict `methods` are pose dicts
    as in `pose_metrics`, frames in order.  Returns {name: {'joint': float64 numpy [F - 2], 'vert': float64 numpy [F - 2]}}: the
    acceleration error of the 21 joints and of the posed model vertices."""
    verts = _model(model_verts)
    gj, gR, gt_t = _pose(gt, 'gt')
    F = gj.shape[0]
    if F < 3:
        raise ValueError('gt: %d frames, the second difference needs at least 3' % F)
    if not isinstance(methods, dict) or not methods:
        raise ValueError('methods: expected a non-empty dict of pose dicts')
    g_cl = _transform(verts, gR, gt_t, gt_t)
    out, dev_out = {}, []
    for name, m in methods.items():
        j, R, t = _pose(m, 'methods[%r]' % (name,), F)
        dev_out.append(torch.stack([_accel(gj, j), _accel(g_cl, _transform(verts, R, t, gt_t))]))
    host = torch.stack(dev_out).cpu().numpy()
    for k, name in enumerate(methods):
        out[name] = dict(joint=host[k, 0], vert=host[k, 1])
    return out
