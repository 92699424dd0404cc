"""The alignment kernels on the device (hn_align.hip, honerf_amd.alignment) and what surfaces them (pose_metrics, mesh_distance) against
the float64 restatement of tests/alignment_cases.py."""
import functools

import numpy as np
import pytest
import torch

import alignment_cases as C
from helpers import bounded, record

pytestmark = pytest.mark.gpu
TOL = 1e-6                                               # m: the project's distance bound (tests/test_interaction.py)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _cu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _moments(a, b, w):
    from honerf_amd import alignment
    return alignment._moments(_cu(a), _cu(b), _cu(w))


@functools.lru_cache(maxsize=None)
def results():
    """Computed once and shared, never changed: per case the device's moments and procrustes result, as numpy."""
    from honerf_amd import alignment
    out = []
    for c in C.cases():
        r = alignment.procrustes(c['a'], c['b'], c['w'], scale=c['scale'])
        out.append((c, _np(_moments(c['a'], c['b'], c['w'])), {k: _np(v) for k, v in r.items()}))
    return tuple(out)


def _w(c, f):
    return None if c['w'] is None else c['w'][f]


# ---- 1: moments ------------------------------------------------------------------------------------------------------------------------
def test_chunk_constant_is_the_kernels():
    from honerf_amd import alignment, lib
    assert lib.load().hn_align_chunk() == alignment.CHUNK == C.CHUNK


def test_moments_within_the_summation_bound():
    """Every entry within (N + 8) eps64 sum|terms| of numpy's float64 sum of the same terms.  The device's tree is N / 64 additions per
    lane at most 16 deep, 6 butterfly levels and the chunks in order: far fewer roundings than the N a plain loop makes; + 8 covers the
    products' own roundings, the division of the centroids and numpy's pairwise sum.  The second moments are sums of terms about a
    centroid: they are compared with numpy's sums about the DEVICE's centroid (itself checked, entry by entry, by the same bound), so
    that both add the same terms."""
    worst = 0.0
    for c, m, _ in results():
        N = c['a'].shape[1]
        for f in range(len(m)):
            ref, ab = C.np_moments(c['a'][f], c['b'][f], _w(c, f))
            bound = (N + 8) * C.EPS64 * ab
            assert (np.abs(m[f, :7] - ref[:7]) <= bound[:7]).all(), (c['name'], f, np.abs(m[f, :7] - ref[:7]) / np.maximum(bound[:7], 1e-300))
            ref2, ab2 = C.np_moments(c['a'][f], c['b'][f], _w(c, f), ca=m[f, 1:4], cb=m[f, 4:7])
            bound2 = (N + 8) * C.EPS64 * ab2
            err = np.abs(m[f, 7:] - ref2[7:])
            assert (err <= bound2[7:]).all(), (c['name'], f, err / np.maximum(bound2[7:], 1e-300))
            worst = max(worst, float((np.abs(m[f] - np.concatenate([ref[:7], ref2[7:]])) / np.maximum(np.concatenate([bound[:7], bound2[7:]]), 1e-300)).max()))
            assert np.isfinite(m[f]).all()
    record('moments: largest error / bound', worst, 1.0, kind='ratio')


def test_moments_bits_repeat_and_do_not_depend_on_the_launch():
    for c, m, _ in results():
        a, b, w = c['a'], c['b'], c['w']
        F, N = a.shape[:2]
        assert _np(_moments(a, b, w)).tobytes() == m.tobytes(), c['name']                       # run to run
        if w is None:                                                                           # NULL and explicit ones
            assert _np(_moments(a, b, np.ones((F, N), np.float32))).tobytes() == m.tobytes(), c['name']
        f = F // 2                                                                              # a frame alone
        assert _np(_moments(a[f:f + 1], b[f:f + 1], None if w is None else w[f:f + 1])).tobytes() == m[f:f + 1].tobytes(), c['name']
    # a frame among 64 others, in front, in the middle and at the end
    for N in (21, C.CHUNK, 2 * C.CHUNK + 1):
        rs = np.random.RandomState(N)
        a = (0.8 + 0.05 * rs.uniform(-1, 1, (65, N, 3))).astype(np.float32)
        b = (0.3 + 0.05 * rs.uniform(-1, 1, (65, N, 3))).astype(np.float32)
        w = rs.uniform(0, 1, (65, N)).astype(np.float32)
        alone = _np(_moments(a[:1], b[:1], w[:1])).tobytes()
        for k in (0, 31, 64):
            perm = np.roll(np.arange(65), k)
            assert _np(_moments(a[perm], b[perm], w[perm]))[k].tobytes() == alone, (N, k)


# ---- 2: solve --------------------------------------------------------------------------------------------------------------------------
def test_solve_is_a_proper_rotation_with_the_specified_rank_always():
    for c, _, r in results():
        R = r['R']
        assert all(np.isfinite(r[k]).all() for k in ('R', 's', 't', 'aligned', 'rms')), c['name']
        assert np.abs(np.einsum('fki,fkj->fij', R, R) - np.eye(3)).max() <= 1e-14, c['name']
        assert (np.linalg.det(R) > 0).all(), c['name']
        assert (r['rank'] == c['rank']).all(), (c['name'], r['rank'])
        assert r['rank'].dtype == np.int32 and r['R'].dtype == r['s'].dtype == r['t'].dtype == np.float64 and r['aligned'].dtype == np.float32
        if c['rank'] == 0:
            assert (R == np.eye(3)).all(), c['name']
        if not c['scale']:
            assert (r['s'] == 1.0).all()
        assert (r['s'] >= 0).all()


def test_solve_within_eight_spreads_of_the_float64_restatement():
    """R, s, t of every rank-3 case within 8 x the spread the CPU test measured between the two float64 formulations for that kind
    (alignment_cases.SPREAD), 1e-13 at least."""
    worst = {}
    for c, _, r in results():
        if not C.rank3(c):
            continue
        sp = C.SPREAD[c['kind']]
        for f in range(len(c['a'])):
            R, s, t = C.umeyama_svd(c['a'][f], c['b'][f], _w(c, f), c['scale'])
            e = dict(R=np.abs(r['R'][f] - R).max(), s=abs(r['s'][f] - s), t=np.abs(r['t'][f] - t).max())
            for k, v in e.items():
                worst[(c['kind'], k)] = max(worst.get((c['kind'], k), 0.0), float(v) / max(8.0 * sp[k], C.FLOOR))
    for (kind, k), v in sorted(worst.items()):
        bounded('solve %s %s: error / (8 x spread, floor 1e-13)' % (kind, k), v, 1.0, kind='ratio')


# ---- 3: optimality ---------------------------------------------------------------------------------------------------------------------
def test_no_planted_or_perturbed_transform_has_a_smaller_residual():
    """The weighted residual of the returned transform, in float64 on the host, is at most that of the planted transform and of 32
    perturbations of the returned one (rotations of 1e-6 .. 1e-2 rad, scale changes of 1e-6 .. 1e-2, translations of 1e-9 .. 1e-4 m),
    with a relative slack of 1e-12 and the floor of the float64 evaluation itself, W (8 eps64 max|b|)^2 (src == dst has a planted
    residual of exactly 0)."""
    rs = np.random.RandomState(7)
    for c, _, r in results():
        for f in range(0, len(c['a']), max(1, len(c['a']) // 4)):
            a, b, w = c['a'][f], c['b'][f], _w(c, f)
            R, s, t = r['R'][f], r['s'][f], r['t'][f]
            floor = (1.0 if w is None else float(w.sum()) / len(a)) * len(a) * (8 * C.EPS64 * float(np.abs(b).max())) ** 2
            mine = C.residual(a, b, w, R, s, t) - floor
            if c['planted'] is not None:
                Rp, sp, tp = (x[f] for x in c['planted'])
                assert mine <= C.residual(a, b, w, Rp, sp, tp) * (1 + 1e-12), (c['name'], f)
            ca = C.np_moments(a, b, w)[0][1:4]
            for k in range(32):
                dR = C.rotation(rs.standard_normal(3), 10.0 ** rs.uniform(-6, -2))
                ds = 1.0 + (10.0 ** rs.uniform(-6, -2)) * rs.choice([-1.0, 1.0]) if c['scale'] else 1.0
                dt = rs.standard_normal(3)
                dt *= 10.0 ** rs.uniform(-9, -4) / np.linalg.norm(dt)
                which = k % 4                                                       # one of the three alone, then all together
                if which == 1 and not c['scale']:
                    which = 0                                                       # (a rigid fit has no scale to perturb)
                R2 = dR @ R if which in (0, 3) else R
                s2 = s * ds if which in (1, 3) else s
                # the rotation and the scale are perturbed about the moved source centroid, so that each moves the cloud, not the lever
                t2 = (s * R @ ca + t) - s2 * R2 @ ca + (dt if which in (2, 3) else 0.0)
                assert mine <= C.residual(a, b, w, R2, s2, t2) * (1 + 1e-12), (c['name'], f, k)


# ---- 4: apply and compose --------------------------------------------------------------------------------------------------------------
def test_aligned_is_the_float64_evaluation_rounded_once():
    from honerf_amd import alignment
    for c, _, r in results():
        for f in range(len(c['a'])):
            assert C.np_apply(c['a'][f], r['R'][f], r['s'][f], r['t'][f]).tobytes() == r['aligned'][f].tobytes(), (c['name'], f)
    c, _, r = results()[12]
    again = alignment.transform(c['a'], r['R'], r['s'], r['t'])
    assert _np(again).tobytes() == r['aligned'].tobytes()


def test_broadcast_and_compose():
    from honerf_amd import alignment
    rs = np.random.RandomState(3)
    p = (0.8 + 0.05 * rs.uniform(-1, 1, (5, 300, 3))).astype(np.float32)
    T1 = (C.rotation(rs.standard_normal(3), 0.7), 1.25, rs.standard_normal(3) * 0.1)
    T2 = (C.rotation(rs.standard_normal(3), 2.1), 0.6, rs.standard_normal(3) * 0.3)
    one = _np(alignment.transform(p, *T1))
    rep = _np(alignment.transform(p, np.repeat(T1[0][None], 5, 0), np.full(5, T1[1]), np.repeat(T1[2][None], 5, 0)))
    assert one.tobytes() == rep.tobytes()                                                       # the broadcast form is the repeated form
    for f in range(5):
        assert C.np_apply(p[f], *T1).tobytes() == one[f].tobytes()
    dev = lambda T: (_cu(T[0][None]), _cu(np.array([T[1]])), _cu(T[2][None]))
    Rc, sc, tc = (_np(x)[0] for x in alignment._compose(dev(T2), dev(T1)))
    ref = C.np_compose(T2, T1)
    assert np.abs(Rc - ref[0]).max() < 1e-15 and abs(sc - ref[1]) < 1e-15 and np.abs(tc - ref[2]).max() < 1e-15
    # compose then apply = the two applies made in float64 without the rounding in between, within 1 ulp of fp32
    got = _np(alignment.transform(p, Rc, sc, tc)).astype(np.float64)
    p64 = p.astype(np.float64)
    two = T2[1] * ((T1[1] * (p64 @ T1[0].T) + T1[2]) @ T2[0].T) + T2[2]
    assert (np.abs(got - two) <= np.spacing(np.abs(two).astype(np.float32)).astype(np.float64)).all()


# ---- 5: ICP ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icp_run(motion, outliers=0.0):
    from honerf_amd import alignment
    from honerf_amd.mesh_distance import MeshIndex
    mesh, pts, planted, ref = C.icp_cases(motion, outliers)
    index = MeshIndex((_cu(mesh[0]), _cu(mesh[1])))
    before = alignment.HOST_COPIES
    r = alignment.icp(_cu(pts), index, iters=C.ICP_ITERS, max_distance=0.1 if outliers else None)
    copies = alignment.HOST_COPIES - before
    again = alignment.icp(_cu(pts), index, iters=C.ICP_ITERS, max_distance=0.1 if outliers else None)
    return r, again, copies, ref, pts


def _icp_distance(r, ref, pts):
    """How far the device's final transform is from the float64 reference's: (the largest entry of R - R_ref, |s - s_ref|, the distance
    between the two images of the cloud's centre), with the bounds derived in test_icp_follows_the_float64_reference."""
    p = pts[:2000].astype(np.float64)
    c = p.mean(0)
    ev = np.linalg.eigvalsh(np.cov((p - c).T, bias=True))
    lever = np.sqrt(ev[0] + ev[1])
    R, s, t = _np(r['R']), float(r['s']), _np(r['t'])
    dc = np.linalg.norm((s * R @ c + t) - (ref['s'] * ref['R'] @ c + ref['t']))
    return np.abs(R - ref['R']).max(), abs(s - ref['s']), dc, lever


@pytest.mark.parametrize('motion', sorted(C.MOTIONS))
def test_icp_follows_the_float64_reference(motion):
    """The trace never rises by more than 1e-7 m (a least-squares step and a closest-point step cannot raise the RMS; the applied points
    are rounded to fp32, half an ulp of 0.6 m = 3e-8 m per coordinate, and so are the closest points).

    The final transform against icp_reference.  The device makes the reference's iteration with a perturbation per step: every moved
    point and every closest point is an fp32 point, each within sqrt(3) x 3e-8 m of its float64 value, together e = 1e-7 m per pair.  A
    least-squares fit moves the cloud's centre by no more than e and turns it by no more than e / lever (lever: the root of the two
    smaller eigenvalues of the cloud's covariance); near its fixed point the ICP map does not expand differences (a closest-point
    projection and a least-squares fit), so after k steps the two runs differ by k e at the centre and k e / lever in R at most.  The
    issue words this bound as that of the solve test scaled by the reference's own last step; that reference still moves by 1e-3
    per step at the end (point-to-surface ICP creeps along facets), which would bound nothing, so the derived bound stands here."""
    r, again, copies, ref, pts = icp_run(motion)
    rms = r['rms']
    assert rms.shape == (C.ICP_ITERS + 1,) and rms.dtype == np.float64 and np.isfinite(rms).all()
    print(motion, 'device rms', rms[[0, 1, 2, 5, 10, 20, -2, -1]], 'reference', ref['rms'][[0, 1, 2, 5, 10, 20, -2, -1]])
    bounded('icp %s: largest rise of the rms trace' % motion, float(np.diff(rms).max()), 1e-7, kind='abs')
    dR, ds, dc, lever = _icp_distance(r, ref, pts)
    k = C.ICP_ITERS
    bounded('icp %s: |R - R_ref|' % motion, dR, k * 1e-7 / lever, kind='abs')
    bounded('icp %s: centre image distance' % motion, dc, k * 1e-7, kind='abs')
    assert ds == 0.0 and float(r['s']) == 1.0
    bounded('icp %s: rms trace against the reference' % motion, float(np.abs(rms - ref['rms']).max()), k * 1e-7, kind='abs')
    R = _np(r['R'])
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and np.linalg.det(R) > 0
    assert 0 <= r['converged_at'] <= k
    assert C.np_apply(pts, R, 1.0, _np(r['t'])).tobytes() == _np(r['aligned']).tobytes()
    # no device-to-host copy before the end, and the same bits on a second run
    assert copies == 1
    for key in ('R', 's', 't', 'aligned', 'rms'):
        assert _np(r[key]).tobytes() == _np(again[key]).tobytes(), key


def test_icp_ignores_outliers_beyond_max_distance():
    r, again, copies, ref, pts = icp_run('small', 0.1)
    plain = icp_run('small')[0]
    assert len(pts) == 2200 and copies == 1
    # the same iteration but for the order of the fp64 sums (2 200 points are cut into other chunks than 2 000): the bound of the
    # reference comparison holds between the two device runs as well
    dR, ds, dc, lever = _icp_distance(r, dict(R=_np(plain['R']), s=float(plain['s']), t=_np(plain['t'])), pts)
    bounded('icp outliers: |R - R_plain|', dR, C.ICP_ITERS * 1e-7 / lever, kind='abs')
    bounded('icp outliers: centre image distance', dc, C.ICP_ITERS * 1e-7, kind='abs')
    dR, ds, dc, lever = _icp_distance(r, ref, pts)
    bounded('icp outliers: |R - R_ref|', dR, C.ICP_ITERS * 1e-7 / lever, kind='abs')
    bounded('icp outliers: centre image distance to the reference', dc, C.ICP_ITERS * 1e-7, kind='abs')


def test_icp_similarity_and_init():
    """scale=True on a scene shrunk by 2 %: the scale is found (to the ICP's own creep), and `init` starts from a given transform."""
    from honerf_amd import alignment
    mesh, pts, planted, _ = C.icp_cases('small')
    c = mesh[0].astype(np.float64).mean(0)
    shrunk = (c + (pts.astype(np.float64) - c) / 1.02).astype(np.float32)
    r = alignment.icp(shrunk, (mesh[0], mesh[1]), iters=C.ICP_ITERS, scale=True)
    print('scale found', float(r['s']), 'rms', r['rms'][[0, -1]])
    assert 1.01 < float(r['s']) < 1.03 and r['rms'][-1] < 0.2 * r['rms'][0]
    start = alignment.icp(pts, (mesh[0], mesh[1]), iters=3)
    cont = alignment.icp(pts, (mesh[0], mesh[1]), iters=2, init=start)
    full = alignment.icp(pts, (mesh[0], mesh[1]), iters=5)
    for key in ('R', 't', 'aligned'):
        assert _np(cont[key]).tobytes() == _np(full[key]).tobytes(), key


# ---- 6: metrics ------------------------------------------------------------------------------------------------------------------------
def _hands(F=40, J=21, seed=0):
    rs = np.random.RandomState(seed)
    gt = np.stack([C._cloud(rs, J, size=0.08) for _ in range(F)])
    pred = np.stack([C._image(gt[f], *C._planted(rs, f)) for f in range(F)])
    return pred, gt, rs


def _np_pa_errors(pred, gt):
    out = []
    for p, g in zip(pred, gt):
        R, s, t = C.umeyama_svd(p, g, None, True)
        out.append(np.linalg.norm(s * (p.astype(np.float64) @ R.T) + t - g, axis=1))
    return np.stack(out)


def test_pa_joint_error():
    from honerf_amd import pose_metrics as pm
    pred, gt, rs = _hands()
    e = _np(pm.pa_joint_error(pred, gt))
    assert e.shape == (40,) and e.dtype == np.float64
    bounded('pa_joint_error of similarity images', float(e.max()), 2e-7, kind='abs')
    noisy = (pred.astype(np.float64) + 0.004 * rs.standard_normal(pred.shape)).astype(np.float32)
    ref = _np_pa_errors(noisy, gt).mean(1)
    bounded('pa_joint_error against float64', float(np.abs(_np(pm.pa_joint_error(noisy, gt)) - ref).max()), TOL, kind='abs')
    bounded('pa_add against float64', float(np.abs(_np(pm.pa_add(noisy, gt)) - ref).max()), TOL, kind='abs')
    assert (_np(pm.pa_joint_error(noisy, gt)) < _np(pm.joint_error(noisy, gt))).all()
    one = pm.pa_joint_error(noisy[3], gt[3])
    assert one.dim() == 0 and abs(float(one) - ref[3]) <= TOL
    # float64 inputs at camera distance: centred before the fp32 round, the same number
    bounded('pa_joint_error of float64 inputs', float(np.abs(_np(pm.pa_joint_error(noisy.astype(np.float64), gt.astype(np.float64))) - ref).max()),
            TOL, kind='abs')


def test_pck_auc_counts_are_numpys():
    from honerf_amd import pose_metrics as pm
    rs = np.random.RandomState(1)
    e = np.abs(rs.standard_normal((57, 21)) * 0.02).astype(np.float32)
    thr = np.linspace(0.0, 0.05, 100)
    e[0, :5] = thr[[0, 1, 50, 98, 99]].astype(np.float32)                        # entries at (the fp32 image of) a threshold
    r = pm.pck_auc(e)
    count = (e.astype(np.float64).reshape(-1, 1) <= thr[None]).sum(0)
    assert (r['count'] == count).all() and (r['thresholds'] == thr).all()
    pck = count / e.size
    assert (r['pck'] == pck).all() and r['auc'] == float(((pck[1:] + pck[:-1]) * 0.5 * np.diff(thr)).sum() / 0.05)
    r2 = pm.pck_auc(torch.from_numpy(e).cuda().double(), lo=0.01, hi=0.03, steps=7)
    assert (r2['count'] == (e.astype(np.float64).reshape(-1, 1) <= np.linspace(0.01, 0.03, 7)[None]).sum(0)).all()


def test_hand_metrics_is_its_pieces():
    from honerf_amd import pose_metrics as pm
    pred, gt, rs = _hands(F=12)
    pred = (pred.astype(np.float64) + 0.006 * rs.standard_normal(pred.shape)).astype(np.float32)
    gv = np.stack([C._cloud(rs, 778, size=0.08) for _ in range(12)])
    pv = np.stack([C._image(gv[f], *C._planted(rs, f)) for f in range(12)])
    pv = (pv.astype(np.float64) + 0.006 * rs.standard_normal(pv.shape)).astype(np.float32)
    m = pm.hand_metrics(pred, gt)
    assert sorted(m) == ['auc', 'mpjpe', 'pa_auc', 'pa_mpjpe']
    m = pm.hand_metrics(pred, gt, pv, gv)
    assert sorted(m) == ['auc', 'f15', 'f5', 'mpjpe', 'mpvpe', 'pa_auc', 'pa_mpjpe', 'pa_mpvpe'] and all(isinstance(v, float) for v in m.values())
    from honerf_amd.alignment import procrustes
    assert m['mpjpe'] == float(pm.joint_error(pred, gt).mean()) and m['pa_mpjpe'] == float(pm.pa_joint_error(pred, gt).mean())
    assert m['mpvpe'] == float(pm.add(pv, gv).mean()) and m['pa_mpvpe'] == float(pm.pa_add(pv, gv).mean())
    assert m['auc'] == pm.pck_auc(pm.paired_distance(pred, gt))['auc']
    assert m['pa_auc'] == pm.pck_auc(pm.paired_distance(procrustes(pred, gt)['aligned'], gt))['auc']
    assert m['pa_mpjpe'] < m['mpjpe'] and m['pa_auc'] > m['auc']
    al = _np(procrustes(pv, gv)['aligned']).astype(np.float64)
    for key, tau in (('f5', 0.005), ('f15', 0.015)):
        fs = []
        for f in range(12):
            d = np.linalg.norm(al[f][:, None] - gv[f].astype(np.float64)[None], axis=2)
            p, r = (d.min(1) <= tau).mean(), (d.min(0) <= tau).mean()
            fs.append(2 * p * r / (p + r) if p + r > 0 else 0.0)
        assert abs(m[key] - np.mean(fs)) <= 1.0 / 778, (key, m[key], np.mean(fs))     # (a distance within fp32 rounding of tau may fall either side)
    assert 0 < m['f5'] < m['f15'] <= 1


ITERS_SM = 300


def test_surface_metrics_alignment():
    from honerf_amd.mesh_distance import surface_metrics
    gt = C.blob_mesh()
    n = 4000
    base = surface_metrics(gt, gt, n=n, seed=3)
    assert surface_metrics(gt, gt, n=n, seed=3, align=None) == base and 'transform' not in base        # today's bits
    Rm = C.rotation([0.3, -1.0, 0.5], np.deg2rad(1.0))
    c = gt[0].astype(np.float64).mean(0)
    moved = (((gt[0].astype(np.float64) - c) @ Rm.T) + c + np.array([0.0008, -0.0004, 0.0006])).astype(np.float32), gt[1]
    raw = surface_metrics(moved, gt, n=n, seed=3)
    al = surface_metrics(moved, gt, n=n, seed=3, align='icp', icp_iters=ITERS_SM)
    print('chamfer-L1: unmoved %.3e, moved %.3e, aligned %.3e; icp rms %.3e -> %.3e' % (base['chamfer_l1'], raw['chamfer_l1'], al['chamfer_l1'],
                                                                                      al['icp_rms'][0], al['icp_rms'][-1]))
    assert al['chamfer_l1'] <= raw['chamfer_l1']
    assert sorted(set(al) - set(raw)) == ['icp_rms', 'transform'] and len(al['icp_rms']) == ITERS_SM + 1
    R = np.asarray(al['transform']['R'])
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and al['transform']['s'] == 1.0
    bounded('surface_metrics align=icp: chamfer-L1 against the unmoved copy', abs(al['chamfer_l1'] - base['chamfer_l1']), TOL, kind='abs')
    sc = surface_metrics(moved, gt, n=n, seed=3, align='icp+scale', icp_iters=10)
    assert sc['transform']['s'] != 1.0 and sc['chamfer_l1'] <= raw['chamfer_l1']


# ---- 7: arguments ----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_name_the_argument():
    from honerf_amd import alignment, pose_metrics as pm
    a = np.zeros((4, 10, 3), np.float32)
    mesh = C.blob_mesh()
    for call, name in ((lambda: alignment.procrustes(a[0, :, :2], a[0]), 'src'), (lambda: alignment.procrustes(a, a[0]), 'dst'),
                       (lambda: alignment.procrustes(a, a[:3]), 'dst'), (lambda: alignment.procrustes(a, a[:, :9]), 'dst'),
                       (lambda: alignment.procrustes(a[:, :0], a[:, :0]), 'src'), (lambda: alignment.procrustes(a.astype(np.int32), a), 'src'),
                       (lambda: alignment.procrustes(a, a, weights=-np.ones((4, 10), np.float32)), 'weights'),
                       (lambda: alignment.procrustes(a, a, weights=np.ones((4, 9), np.float32)), 'weights'),
                       (lambda: alignment.procrustes(a, a, weights=np.ones((3, 10), np.float32)), 'weights'),
                       (lambda: alignment.transform(a, np.eye(4), 1.0, np.zeros(3)), 'R'), (lambda: alignment.transform(a, np.eye(3), 1.0, np.zeros(2)), 't'),
                       (lambda: alignment.transform(a, np.repeat(np.eye(3)[None], 3, 0), np.ones(3), np.zeros((3, 3))), 'R'),
                       (lambda: alignment.transform(a[..., :2], np.eye(3), 1.0, np.zeros(3)), 'points'),
                       (lambda: alignment.icp(a, mesh), 'points'), (lambda: alignment.icp(a[0], mesh, iters=0), 'iters'),
                       (lambda: alignment.icp(a[0], mesh, max_distance=-1.0), 'max_distance'), (lambda: alignment.icp(a[0], (mesh[0], mesh[1][:0])), 'target'),
                       (lambda: pm.pa_joint_error(a, a[:3]), 'gt_joints'), (lambda: pm.pa_add(a[0], a), 'gt_pts'),
                       (lambda: pm.pck_auc(np.zeros(0, np.float32)), 'errors'), (lambda: pm.pck_auc(a, lo=0.1, hi=0.1), 'hi'),
                       (lambda: pm.hand_metrics(a, a, a, None), 'gt_verts'), (lambda: pm.hand_metrics(a, a, a[:2], a[:2]), 'pred_verts')):
        with pytest.raises(ValueError, match=name):
            call()
    from honerf_amd.mesh_distance import surface_metrics
    with pytest.raises(ValueError, match='align'):
        surface_metrics(mesh, mesh, n=10, align='procrustes')
    from honerf_amd import lib
    L = lib.load()
    assert L.hn_align_workspace_bytes(0, 5) == 0 and L.hn_align_workspace_bytes(1 << 20, 1 << 12) == 0 and L.hn_align_workspace_bytes(5, 21) > 0


def test_float64_inputs_are_centred_before_the_round():
    """float64 clouds 0.8 m out: R and s are those of the fp32 images centred on dst's first point, to the bit; t is corrected for the
    shift, and the transform is the float64 restatement's to what fp32 centred coordinates allow (ulp 7e-9 m at 0.1 m)."""
    from honerf_amd import alignment
    rs = np.random.RandomState(11)
    a = np.stack([C._cloud(rs, 50) for _ in range(3)]).astype(np.float64) + 1e-9 * rs.standard_normal((3, 50, 3))
    b = np.stack([C._planted(rs, f)[1] * (a[f] @ C._planted(rs, f)[0].T) for f in range(3)]) + 0.3
    r = alignment.procrustes(a, b)
    c = b[:, :1]
    r32 = alignment.procrustes((a - c).astype(np.float32), (b - c).astype(np.float32))
    assert _np(r['R']).tobytes() == _np(r32['R']).tobytes() and _np(r['s']).tobytes() == _np(r32['s']).tobytes()
    for f in range(3):
        R, s, t = C.umeyama_svd(a[f], b[f])
        ca = a[f].mean(0)
        got = float(_np(r['s'])[f]) * _np(r['R'])[f] @ ca + _np(r['t'])[f]
        bounded('float64 procrustes: image of the centroid', float(np.abs(got - (s * R @ ca + t)).max()), 1e-7, kind='abs')
        bounded('float64 procrustes: aligned', float(np.abs(_np(r['aligned'])[f] - b[f]).max()), 2e-7, kind='abs')
