"""The float64 restatement of the alignment contract (tests/alignment_cases.py) checked against itself, without a GPU: two independent
formulations of the Procrustes problem agree, both recover what was planted, and the ICP scene is fair.  The spread between the two
formulations is MEASURED here, per kind of case, and held against the constants alignment_cases.SPREAD, which the device's bound
(tests/test_gpu_alignment.py) is taken from."""
import numpy as np
import pytest

import alignment_cases as C
from helpers import record


def _frames(case):
    for f in range(len(case['a'])):
        yield f, case['a'][f], case['b'][f], None if case['w'] is None else case['w'][f]


def test_cases_cover_the_edges():
    cs = C.cases()
    assert {c['a'].shape[1] for c in cs} >= set(C.N_EDGES) and {c['a'].shape[0] for c in cs} >= set(C.F_EDGES)
    assert {c['kind'] for c in cs} == set(C.RANK3_KINDS) | {'collinear', 'coincident', 'wone'}
    assert {c['rank'] for c in cs} == {0, 1, 3}
    for c in cs:
        assert c['a'].dtype == c['b'].dtype == np.float32 and c['a'].shape == c['b'].shape and np.isfinite(c['a']).all()
        assert c['w'] is None or (c['w'].dtype == np.float32 and (c['w'] >= 0).all())


def test_two_formulations_agree_and_their_spread_is_recorded():
    """On every rank-3 case the SVD form and the quaternion form give the same transform and the same residual.  The largest
    difference per kind is recorded (the parity report) and must stay within 4 x the constants the device's bound is built on (4 x:
    LAPACK picks its kernels by the CPU it runs on, and another kernel rounds differently)."""
    spread = {}
    for c in C.cases():
        if not C.rank3(c):
            continue
        d = spread.setdefault(c['kind'], dict(R=0.0, s=0.0, t=0.0, res=0.0))
        for f, a, b, w in _frames(c):
            R1, s1, t1 = C.umeyama_svd(a, b, w, c['scale'])
            R2, s2, t2 = C.horn_quaternion(a, b, w, c['scale'])
            vb = C.np_moments(a, b, w)[0][17]
            r1, r2 = C.residual(a, b, w, R1, s1, t1), C.residual(a, b, w, R2, s2, t2)
            d['R'] = max(d['R'], float(np.abs(R1 - R2).max()))
            d['s'] = max(d['s'], abs(s1 - s2))
            d['t'] = max(d['t'], float(np.abs(t1 - t2).max()))
            d['res'] = max(d['res'], abs(r1 - r2) / vb)
            for R in (R1, R2):
                assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0
    assert set(spread) == set(C.SPREAD) == set(C.RANK3_KINDS)
    for kind, d in spread.items():
        for k, v in d.items():
            record('spread of the two float64 formulations: %s %s' % (kind, k), v, 4.0 * max(C.SPREAD[kind][k], 1e-16), kind='abs')
            print('%-12s %-4s measured %.3e recorded %.1e' % (kind, k, v, C.SPREAD[kind][k]))
            assert v <= 4.0 * max(C.SPREAD[kind][k], 1e-16), (kind, k, v)


def test_both_recover_the_planted_transform():
    """b = float32(s R a + t): the only difference from the planted transform is the rounding of b, delta = sqrt(3) 2^-24 max|b| per
    point at most.  A least-squares fit moves by no more than its worst coherent perturbation: the translation of the centroid by
    delta, the rotation by delta over the lever the cloud offers, rho = sqrt of the sum of the two smaller eigenvalues of a's weighted
    covariance (the rotation about the cloud's longest axis has the shortest lever) times s, the scale by delta / (s x the cloud's
    RMS radius) relative.  Held to 4 x that (three coordinates, two clouds' roundings of the centroid)."""
    seen = 0
    for c in C.cases():
        if not (C.rank3(c) and c['exact'] and c['planted'] is not None):
            continue
        for f, a, b, w in _frames(c):
            Rp, sp, tp = (x[f] for x in c['planted'])
            wt = np.ones(len(a)) if w is None else w.astype(np.float64)
            a64 = a.astype(np.float64)
            ca = (wt[:, None] * a64).sum(0) / wt.sum()
            ev = np.linalg.eigvalsh(((wt[:, None] * (a64 - ca))[:, :, None] * (a64 - ca)[:, None, :]).sum(0) / wt.sum())
            rho, radius = np.sqrt(ev[0] + ev[1]), np.sqrt(ev.sum())
            delta = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(b).max())
            for form in (C.umeyama_svd, C.horn_quaternion):
                R, s, t = form(a, b, w, c['scale'])
                moved = np.abs((s * R @ ca + t) - (sp * Rp @ ca + tp)).max()        # where the centroid goes: free of the lever |ca|
                assert np.abs(R - Rp).max() <= 4.0 * delta / (sp * rho), (c['name'], f, np.abs(R - Rp).max(), delta / (sp * rho))
                assert abs(s - sp) / sp <= 4.0 * delta / (sp * radius), (c['name'], f)
                assert moved <= 4.0 * delta, (c['name'], f, moved, delta)
                seen += 1
    assert seen > 100


def test_degenerate_cases_have_the_residual_of_the_planted_transform():
    """Collinear points: every rotation that maps the line onto the line is optimal, and both formulations find one."""
    for c in C.cases():
        if c['kind'] != 'collinear':
            continue
        for f, a, b, w in _frames(c):
            Rp, sp, tp = (x[f] for x in c['planted'])
            vb = C.np_moments(a, b, w)[0][17]
            for form in (C.umeyama_svd, C.horn_quaternion):
                R, s, t = form(a, b, w, c['scale'])
                assert C.residual(a, b, w, R, s, t) <= C.residual(a, b, w, Rp, sp, tp) + 1e-12 * vb


@pytest.mark.parametrize('motion', sorted(C.MOTIONS))
def test_icp_reference_descends_on_the_planted_scene(motion):
    """The scene is fair before the device is judged on it: the float64 ICP's RMS trace never rises (each step is a least-squares
    step followed by a closest-point step, neither can raise it; 1e-12 m for the roundings of float64), falls to less than a tenth of
    where it started, and has nearly stopped: the last step lowers it by less than 1 % of the start.  (Point-to-surface ICP converges
    linearly: samples slide along the facets.  The trace is printed.)"""
    mesh, pts, planted, ref = C.icp_cases(motion)
    rms = ref['rms']
    print(motion, 'rms', rms[[0, 1, 2, 5, 10, 20, -2, -1]], 'last step', ref['last_step'])
    assert len(rms) == C.ICP_ITERS + 1 and np.isfinite(rms).all()
    assert (np.diff(rms) <= 1e-12).all(), np.diff(rms).max()
    assert rms[-1] < 0.1 * rms[0] and rms[-2] - rms[-1] < 0.01 * rms[0]
    # the planted motion puts every sample on the surface
    back = planted[1] * (pts.astype(np.float64) @ planted[0].T) + planted[2]
    assert C.np_closest(mesh[0], mesh[1], back)[0].max() < 2e-7


def test_icp_outliers_beyond_max_distance_do_not_move_the_reference():
    _, _, _, ref = C.icp_cases('small')
    _, pts, _, out = C.icp_cases('small', 0.1)
    assert len(pts) == 2200
    assert np.abs(out['R'] - ref['R']).max() < 1e-12 and np.abs(out['t'] - ref['t']).max() < 1e-12 and np.abs(out['rms'] - ref['rms']).max() < 1e-12
