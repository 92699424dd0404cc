"""The pose side of a fitting step, kernel by kernel through the C ABI, against the float64 references of tests/pose_side_cases.py
(where every bound is derived): hn_pose_chain for LEFT hands and mixed launches, hn_pose_chain_bwd, hn_rigid_pose entry by entry,
hn_verts_loss, hn_jacobian_vjp, hn_pose_side_vjp, hn_leaf_rows_gather / _scatter, hn_adam_step, and PoseAdam's version counters.
Outputs are pre-filled with NaN: 'not written' and 'written as zero' are different answers.  Each kernel is launched once, the device
is synchronised, and the result compared."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pose_side_cases as C
from helpers import bounded, cu

pytestmark = pytest.mark.gpu

GOLD_LEFT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_chain_left.npz')
NAN = float('nan')


def _lib():
    from honerf_amd import lib as L
    return L, L.load()


def nans(*shape):
    return cu(torch.full(shape, NAN, dtype=torch.float32))


def f32(a):
    return cu(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))


def refused(rc, lib):
    """A refusal: a non-zero status and a message."""
    msg = lib.hn_last_error()
    return rc != 0 and bool(msg)


def hold(what, got, want, bound):
    """|got - want| <= bound entry by entry (bound: a tensor of the shape, float64; where it is 0 the entries are equal).  The report
    gets the worst observed / bound ratio, held to 1."""
    got, want, bound = C.f64(got).reshape(-1), C.f64(want).reshape(-1), C.f64(bound).reshape(-1)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all(), what + ': not finite'
    err = (got - want).abs()
    zero = bound == 0
    assert float(err[zero].max()) == 0.0 if zero.any() else True, what + ': an entry with no addends is not exactly zero'
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    return bounded(what + ' (observed / bound)', ratio, 1.0, kind='ratio')


def once(what, got, want):
    """The double-then-round-once kernels: per tensor, |got - want| <= 2 U max |want|."""
    got, want = C.f64(got), C.f64(want)
    assert torch.isfinite(got).all(), what + ': not finite'
    scale = float(want.abs().max())
    e = float((got - want).abs().max()) / scale if scale > 0 else float((got - want).abs().max())
    return e


# ---- hn_pose_chain: left hands ---------------------------------------------------------------------------------------------------
_CHAIN = {}


def chain_launches():
    """The fixture's 12 hands through hn_pose_chain once per form, shared by the tests below: flags all 0 (joint launch, values only,
    Jacobian only), NULL flags, mixed flags."""
    if _CHAIN:
        return _CHAIN
    L, lib = _lib()
    g = np.load(GOLD_LEFT)
    ori, bl, prm = (torch.tensor(g[k], dtype=torch.float32).cuda().contiguous() for k in ('ori_pose', 'bone_len', 'params'))
    F = ori.shape[0]
    new = lambda *sh: torch.full(sh, NAN, device='cuda', dtype=torch.float32)
    st = L.stream_ptr()
    mixed = torch.tensor(([1, 0, 255, 0] * 3)[:F], dtype=torch.uint8)
    flags = {'left': torch.zeros(F, dtype=torch.uint8).cuda(), 'null': None, 'mixed': mixed.cuda()}
    out = {'F': F, 'ori': ori, 'bl': bl, 'prm': prm, 'mixed_flags': mixed.numpy(), 'gold': g, 'flags': flags}
    for name, fl in flags.items():
        bt, j3, jac = new(F, 21, 4, 4), new(F, 21, 3), new(F, 399, 36)
        L.check(lib.hn_pose_chain(L.ptr(ori), L.ptr(bl), L.ptr(fl), L.ptr(prm), F, L.ptr(bt), L.ptr(j3), L.ptr(jac), st), 'hn_pose_chain ' + name)
        out[name] = (bt, j3, jac)
    bt, j3, jac = new(F, 21, 4, 4), new(F, 21, 3), new(F, 399, 36)
    L.check(lib.hn_pose_chain(L.ptr(ori), L.ptr(bl), L.ptr(flags['left']), L.ptr(prm), F, L.ptr(bt), L.ptr(j3), None, st), 'values only')
    L.check(lib.hn_pose_chain(L.ptr(ori), L.ptr(bl), L.ptr(flags['left']), L.ptr(prm), F, None, None, L.ptr(jac), st), 'Jacobian only')
    out['left_split'] = (bt, j3, jac)
    torch.cuda.synchronize()
    _CHAIN.update(out)
    return _CHAIN


def test_pose_chain_left_hands_match_the_float64_oracle():
    """(a) flags all 0: values, joints and Jacobian against the host oracle in float64 on the SAME fp32-rounded inputs, is_right = False.
    The kernel computes in double and rounds once: 2 U of each tensor's largest entry, per hand.  Then against the fixture itself (the
    reference's own statements on the fp64 inputs: that comparison carries the inputs' rounding) at the right-hand test's bounds."""
    from oracle.pose_chain import pose_chain
    c = chain_launches()
    bt, j3, jac = (x.cpu().numpy() for x in c['left'])
    wbt, wj3, wjac = pose_chain(c['ori'].cpu().numpy(), c['bl'].cpu().numpy(), c['prm'].cpu().numpy(), is_right=False)
    for name, got, want in (('bt_inv', bt, wbt), ('joint_3d', j3, wj3), ('jacobian', jac, wjac)):
        worst = max(once(name, got[f], want[f]) for f in range(c['F']))
        bounded('left hands, hn_pose_chain vs float64 oracle on the same fp32 inputs, worst hand: ' + name, worst, C.DOUBLE_ONCE)
    g = c['gold']
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
    bounded('left hands, hn_pose_chain vs reference fp64 fixture: bt_inv', rel(bt, g['bt_inv']), 2e-5)
    bounded('left hands, hn_pose_chain vs reference fp64 fixture: joint_3d', rel(j3, g['joint_3d']), 2e-5)
    bounded('left hands, hn_pose_chain vs reference fp64 fixture: jacobian', rel(jac, g['jac']), 1e-5)


def test_pose_chain_mixed_flags_are_indexed_by_frame():
    """(b) flags [1, 0, 255, 0, ...]: a frame with a non-zero byte is the NULL-flag launch's frame, a frame with 0 the all-left launch's,
    bit for bit -- and the two differ, so a flag read from anywhere but the frame's own byte shows."""
    c = chain_launches()
    for f in range(c['F']):
        src = 'null' if c['mixed_flags'][f] else 'left'
        for name, x, y in zip(('bt_inv', 'joint_3d', 'jacobian'), c['mixed'], c[src]):
            assert torch.equal(x[f], y[f]), 'hand %d (flag %d): %s is not the %s launch\'s' % (f, c['mixed_flags'][f], name, src)
        assert not torch.equal(c['null'][0][f], c['left'][0][f])


def test_pose_chain_left_launch_forms_give_the_same_bits():
    """(c) values + Jacobian, values alone, Jacobian alone, for left hands."""
    c = chain_launches()
    for name, x, y in zip(('bt_inv', 'joint_3d', 'jacobian'), c['left'], c['left_split']):
        bad = [f for f in range(c['F']) if not torch.equal(x[f], y[f])]
        assert not bad, '%s: hands %s differ between the launch forms' % (name, bad)
    assert not any(torch.isnan(x).any() for x in c['left'])


def test_pose_chain_no_frames_writes_nothing():
    """(d) n_frames = 0: status 0, nothing written."""
    L, lib = _lib()
    c = chain_launches()
    bt, j3, jac = nans(1, 21, 4, 4), nans(1, 21, 3), nans(1, 399, 36)
    rc = lib.hn_pose_chain(L.ptr(c['ori']), L.ptr(c['bl']), L.ptr(c['flags']['left']), L.ptr(c['prm']), 0, L.ptr(bt), L.ptr(j3), L.ptr(jac), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and all(torch.isnan(x).all() for x in (bt, j3, jac))


def test_pose_chain_bwd_null_branches():
    """hn_pose_chain_bwd on the device's own stored fp32 Jacobian (left hands 0 .. 2), so that the contraction alone is under test: both
    gradients, either one NULL, both NULL (exact zeros).  One chain of 399 fused multiply-adds: K = 400."""
    L, lib = _lib()
    c = chain_launches()
    F = 3
    jac = c['left'][2][:F].contiguous()
    rng = np.random.RandomState(31)
    gb, gj = rng.standard_normal((F, 336)).astype(np.float32), rng.standard_normal((F, 63)).astype(np.float32)
    d_gb, d_gj = f32(gb), f32(gj)
    for name, a, b in (('both', d_gb, d_gj), ('g_bt_inv NULL', None, d_gj), ('g_joint_3d NULL', d_gb, None), ('both NULL', None, None)):
        out = nans(F, 36)
        L.check(lib.hn_pose_chain_bwd(L.ptr(jac), L.ptr(a), L.ptr(b), F, L.ptr(out), L.stream_ptr()), 'hn_pose_chain_bwd')
        torch.cuda.synchronize()
        go = np.concatenate([gb if a is not None else np.zeros_like(gb), gj if b is not None else np.zeros_like(gj)], axis=1)
        want, mag = C.vjp_f64(jac, go)
        hold('hn_pose_chain_bwd, ' + name, out, want, C.K_CHAIN_BWD * C.U * mag)
        if a is None and b is None:
            assert float(out.abs().max()) == 0.0


# ---- hn_rigid_pose ---------------------------------------------------------------------------------------------------------------
def _rigid(lib, L, c, with_palm, want_jac, F):
    out, jac = nans(F, 412), nans(F, 412, 18)
    d = {k: f32(v) for k, v in c.items()}
    rc = lib.hn_rigid_pose(L.ptr(d['bt_inv0']) if with_palm else None, L.ptr(d['joints0']) if with_palm else None, L.ptr(d['Ro_pred']),
                           L.ptr(d['To_pred']), L.ptr(d['params']), F, with_palm, L.ptr(out), L.ptr(jac) if want_jac else None, L.stream_ptr())
    L.check(rc, 'hn_rigid_pose')
    torch.cuda.synchronize()
    return out.cpu(), jac.cpu()


@pytest.mark.parametrize('F', (1, 5))
def test_rigid_pose_entry_by_entry(F):
    """Values and the full [412,18] Jacobian against rigid_pose_f64 on 6-D inputs that are not normalised; the object half alone
    (with_palm = 0): which entries are written, and that they are the full launch's bits; jac = NULL: the values' bits."""
    L, lib = _lib()
    c = C.rigid_case(F, 40 + F)
    want, wjac = C.rigid_pose_f64(c['bt_inv0'], c['joints0'], c['Ro_pred'], c['To_pred'], c['params'], 1, want_jac=True)
    out, jac = _rigid(lib, L, c, 1, True, F)
    for name, a, b in C.RIGID_SEGMENTS:
        worst_v = max(once(name, out[f, a:b], want[f, a:b]) for f in range(F))
        worst_j = max(once(name, jac[f, a:b], wjac[f, a:b]) for f in range(F))
        bounded('hn_rigid_pose F = %d vs float64, worst frame: %s' % (F, name), worst_v, C.DOUBLE_ONCE)
        bounded('hn_rigid_pose F = %d vs float64 autograd, worst frame: d %s / d params' % (F, name), worst_j, C.DOUBLE_ONCE)
    # structure of the Jacobian: the object outputs do not depend on the palm inputs, nor the hand outputs on the object's
    assert float(jac[:, 399:411, 9:18].abs().max()) == 0.0 and float(jac[:, :399, 0:9].abs().max()) == 0.0
    assert float(jac[:, 411, 0:9].abs().max()) == 0.0
    # the object half alone
    out0, jac0 = _rigid(lib, L, c, 0, True, F)
    assert torch.equal(out0[:, 399:411], out[:, 399:411]) and torch.equal(jac0[:, 399:411], jac[:, 399:411])
    assert float(jac0[:, 399:411, 9:18].abs().max()) == 0.0
    assert torch.isnan(out0[:, :399]).all() and torch.isnan(out0[:, 411]).all()
    assert torch.isnan(jac0[:, :399]).all() and torch.isnan(jac0[:, 411]).all()
    # no Jacobian asked for: the same values, the Jacobian buffer untouched
    out1, jac1 = _rigid(lib, L, c, 1, False, F)
    assert torch.equal(out1, out) and torch.isnan(jac1).all()


def test_rigid_pose_initial_state():
    """Identity 6-D blocks and zero translations: the joint loss is exactly 0, its row of the Jacobian exactly 0 (torch's convention for
    norm at 0) and everything finite; bt_inv is bt_inv0 to rounding."""
    L, lib = _lib()
    F = 2
    c = C.rigid_case(F, 50, initial=True)
    out, jac = _rigid(lib, L, c, 1, True, F)
    assert torch.isfinite(out).all() and torch.isfinite(jac).all()
    assert float(out[:, 411].abs().max()) == 0.0, out[:, 411]
    assert float(jac[:, 411].abs().max()) == 0.0
    want, wjac = C.rigid_pose_f64(c['bt_inv0'], c['joints0'], c['Ro_pred'], c['To_pred'], c['params'], 1, want_jac=True)
    for name, a, b in C.RIGID_SEGMENTS[:4]:
        bounded('hn_rigid_pose, initial state vs float64: ' + name, max(once(name, out[f, a:b], want[f, a:b]) for f in range(F)), C.DOUBLE_ONCE)
        bounded('hn_rigid_pose, initial state vs float64: d %s / d params' % name, max(once(name, jac[f, a:b], wjac[f, a:b]) for f in range(F)),
                C.DOUBLE_ONCE)
    bounded('hn_rigid_pose, initial state: bt_inv vs bt_inv0', once('bt_inv0', out[:, :336], c['bt_inv0'].reshape(F, 336)), C.DOUBLE_ONCE)


def test_rigid_pose_refusals():
    L, lib = _lib()
    c = {k: f32(v) for k, v in C.rigid_case(1, 51).items()}
    out, jac = nans(1, 412), nans(1, 412, 18)
    st = L.stream_ptr()
    assert refused(lib.hn_rigid_pose(None, L.ptr(c['joints0']), L.ptr(c['Ro_pred']), L.ptr(c['To_pred']), L.ptr(c['params']), 1, 1, L.ptr(out),
                                     L.ptr(jac), st), lib)
    assert refused(lib.hn_rigid_pose(L.ptr(c['bt_inv0']), L.ptr(c['joints0']), L.ptr(c['Ro_pred']), L.ptr(c['To_pred']), None, 1, 1, L.ptr(out),
                                     L.ptr(jac), st), lib)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(jac).all()


# ---- hn_verts_loss ---------------------------------------------------------------------------------------------------------------
def _verts(lib, L, c, P):
    d = {k: f32(c[k]) for k in ('Ra', 'ta', 'Rb', 'tb', 'verts')}
    loss, gR, gt = nans(P), nans(P, 9), nans(P, 3)
    L.check(lib.hn_verts_loss(L.ptr(d['Ra']), L.ptr(d['ta']), L.ptr(d['Rb']), L.ptr(d['tb']), L.ptr(d['verts']), c['verts'].shape[0], P,
                              L.ptr(loss), L.ptr(gR), L.ptr(gt), L.stream_ptr()), 'hn_verts_loss')
    torch.cuda.synchronize()
    return loss.cpu(), gR.cpu(), gt.cpu()


@pytest.mark.parametrize('P', (1, 3))
@pytest.mark.parametrize('V', (1, 63, 256, 257, 1000))
def test_verts_loss_matches_float64(V, P):
    """Loss, gR, gt against verts_loss_f64 (autograd), through the C ABI and through VertsLossFn (where the gradients of the second pose
    are the negatives).  V < 256 leaves lanes idle in the 13-way reduction, 257 gives one thread a second vertex."""
    from honerf_amd.pose import VertsLossFn
    L, lib = _lib()
    c = C.verts_case(V, P, 100 + V + P)
    wl, wRa, wta, wRb, wtb = C.verts_loss_f64(c['Ra'], c['ta'], c['Rb'], c['tb'], c['verts'], want_grad=True)
    b_loss, b_gR, b_gt, _ = C.verts_bounds(c['Ra'], c['ta'], c['Rb'], c['tb'], c['verts'])
    loss, gR, gt = _verts(lib, L, c, P)
    tag = 'hn_verts_loss V = %d, P = %d: ' % (V, P)
    hold(tag + 'loss', loss, wl, b_loss)
    hold(tag + 'gR', gR, wRa, b_gR)
    hold(tag + 'gt', gt, wta, b_gt)
    x = [f32(c[k]).clone().requires_grad_(True) for k in ('Ra', 'ta', 'Rb', 'tb')]
    out = VertsLossFn.apply(x[0], x[1], x[2], x[3], f32(c['verts']))
    w = torch.arange(1, P + 1, dtype=torch.float32, device='cuda')          # (powers of two up to 2, and 3: the scaling rounds at most once)
    gs = torch.autograd.grad((out * w).sum(), x)
    torch.cuda.synchronize()
    assert torch.equal(out.detach().cpu(), loss)
    w64 = C.f64(w)
    for name, got, want, bnd in (('Ra', gs[0], wRa, b_gR), ('ta', gs[1], wta, b_gt), ('Rb', gs[2], wRb, b_gR), ('tb', gs[3], wtb, b_gt)):
        sh = (P,) + (1,) * (want.dim() - 1)
        hold(tag + 'VertsLossFn d / d ' + name, got, want * w64.reshape(sh), (bnd.reshape(want.shape) + C.U * want.abs()) * w64.reshape(sh))
    assert torch.equal(gs[2], -gs[0]) and torch.equal(gs[3], -gs[1])


def test_verts_loss_exact_zero_residuals():
    """Identical poses: loss and gradients exactly 0 (torch.norm's convention at 0), nothing NaN.  One vertex at the origin with
    ta == tb among ordinary ones: it adds exactly nothing, so the sums are those of the other vertices with the same 1 / V."""
    L, lib = _lib()
    for V in (1, 63, 257):
        c = C.verts_case(V, 3, 7, 'same')
        for x in _verts(lib, L, c, 3):
            assert torch.isfinite(x).all() and float(x.abs().max()) == 0.0, V
    c = C.verts_case(63, 3, 8, 'zero')
    loss, gR, gt = _verts(lib, L, c, 3)
    wl, wRa, wta, _, _ = C.verts_loss_f64(c['Ra'], c['ta'], c['Rb'], c['tb'], c['verts'], want_grad=True)
    b_loss, b_gR, b_gt, _ = C.verts_bounds(c['Ra'], c['ta'], c['Rb'], c['tb'], c['verts'])
    hold('hn_verts_loss, one zero residual among 63: loss', loss, wl, b_loss)
    hold('hn_verts_loss, one zero residual among 63: gR', gR, wRa, b_gR)
    hold('hn_verts_loss, one zero residual among 63: gt', gt, wta, b_gt)
    # the zero vertex sits in lane 0; moving it to the end of the list changes no sum's addends but the exact zero's place
    c2 = dict(c, verts=np.concatenate([c['verts'][1:], c['verts'][:1]]))
    b2 = C.verts_bounds(c2['Ra'], c2['ta'], c2['Rb'], c2['tb'], c2['verts'])
    l2, gR2, gt2 = _verts(lib, L, c2, 3)
    hold('hn_verts_loss, the zero residual last: gt', gt2, wta, b2[2])
    assert torch.isfinite(gR2).all() and torch.isfinite(l2).all()


def test_verts_loss_refuses_no_vertices():
    L, lib = _lib()
    c = {k: f32(v) for k, v in C.verts_case(1, 1, 9).items() if k != 'kappa_max'}
    loss, gR, gt = nans(1), nans(1, 9), nans(1, 3)
    rc = lib.hn_verts_loss(L.ptr(c['Ra']), L.ptr(c['ta']), L.ptr(c['Rb']), L.ptr(c['tb']), L.ptr(c['verts']), 0, 1, L.ptr(loss), L.ptr(gR), L.ptr(gt),
                           L.stream_ptr())
    torch.cuda.synchronize()
    assert refused(rc, lib) and torch.isnan(loss).all() and torch.isnan(gR).all()


# ---- hn_jacobian_vjp ---------------------------------------------------------------------------------------------------------------
VJP_N_OUT = (1, 3, 12, 13, 16, 17, 29, 399, 412)
VJP_N_IN = (1, 18, 36, 64)


@pytest.mark.parametrize('F', (1, 3))
def test_jacobian_vjp_every_loop_exit(F):
    """n_out 1 .. 29 enter and leave the 16-strided loop and the 4-strided tail at every place for all four waves; 399 and 412 are the
    shapes in use.  K = ceil(n_out / 16) + 8.  The output buffer is one row longer than [F, n_in]: that row keeps its NaN."""
    L, lib = _lib()
    rng = np.random.RandomState(60 + F)
    for n_out in VJP_N_OUT:
        worst = 0.0
        for n_in in VJP_N_IN:
            J = rng.standard_normal((F, n_out, n_in)).astype(np.float32)
            g = rng.standard_normal((F, n_out)).astype(np.float32)
            out = nans(F + 1, n_in)
            L.check(lib.hn_jacobian_vjp(L.ptr(f32(J)), L.ptr(f32(g)), F, n_out, n_in, L.ptr(out), L.stream_ptr()), 'hn_jacobian_vjp')
            torch.cuda.synchronize()
            want, mag = C.vjp_f64(J, g)
            got = out.cpu()
            assert torch.isnan(got[F]).all(), 'n_out %d n_in %d: written past [F, n_in]' % (n_out, n_in)
            err = (C.f64(got[:F]) - want).abs()
            assert torch.isfinite(err).all(), (n_out, n_in)
            worst = max(worst, float((err / (C.k_vjp(n_out) * C.U * mag)).max()))
        bounded('hn_jacobian_vjp F = %d, n_out = %d, n_in in %s (observed / bound)' % (F, n_out, VJP_N_IN), worst, 1.0, kind='ratio')


def test_jacobian_vjp_refusals():
    L, lib = _lib()
    J, g, out = f32(np.ones((1, 4, 65))), f32(np.ones((1, 4))), nans(1, 65)
    for n_in in (65, 0):
        assert refused(lib.hn_jacobian_vjp(L.ptr(J), L.ptr(g), 1, 4, n_in, L.ptr(out), L.stream_ptr()), lib), n_in
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- hn_pose_side_vjp --------------------------------------------------------------------------------------------------------------
# (which, then which of g_bt_inv, g_joint_3d, g_obj_r, g_obj_t, g_obj_r2, g_obj_t2 are present)
SIDE_COMBOS = ((3, 'bjrtRT'), (3, 'bjrt'), (3, ''), (1, 'bj'), (1, 'b'), (1, 'j'), (1, ''), (2, 'rt'), (2, 'RT'), (2, 'rT'), (2, 'R'), (2, ''),
               (3, 'jtR'), (1, 'bjrtRT'), (2, 'bjrtRT'))
PREFILL = -7.5


@pytest.mark.parametrize('F', (1, 4))
def test_pose_side_vjp_combinations(F):
    """Both Jacobians filled with distinct random numbers EVERYWHERE (a read from another row or column of the [412,18] block changes the
    answer); each upstream gradient present or NULL; the columns `which` does not select keep their pre-fill; with which = 3 the hand
    half is hn_pose_chain_bwd's answer on the same inputs."""
    L, lib = _lib()
    rng = np.random.RandomState(70 + F)
    jac_h, jac_o = rng.standard_normal((F, 399, 36)).astype(np.float32), rng.standard_normal((F, 412, 18)).astype(np.float32)
    shapes = {'b': 336, 'j': 63, 'r': 9, 't': 3, 'R': 9, 'T': 3}
    ups = {k: rng.standard_normal((F, n)).astype(np.float32) for k, n in shapes.items()}
    d_h, d_o = f32(jac_h), f32(jac_o)
    d_up = {k: f32(v) for k, v in ups.items()}
    worst = {1: 0.0, 2: 0.0}
    for which, have in SIDE_COMBOS:
        out = cu(torch.full((F + 1, 45), PREFILL, dtype=torch.float32))
        a = [d_up[k] if k in have else None for k in 'bjrtRT']
        L.check(lib.hn_pose_side_vjp(L.ptr(d_h) if which & 1 else None, L.ptr(d_o) if which & 2 else None, *[L.ptr(x) for x in a], F, which,
                                     L.ptr(out), L.stream_ptr()), 'hn_pose_side_vjp')
        torch.cuda.synchronize()
        h = [ups[k] if k in have else None for k in 'bjrtRT']
        want, mag, sel = C.pose_side_vjp_f64(jac_h, jac_o, *h, which, F, PREFILL)
        got = C.f64(out)
        assert torch.isfinite(got).all()
        assert float((got[F] - PREFILL).abs().max()) == 0.0, 'written past [F,45]'
        assert torch.equal(got[:F][:, ~sel], want[:, ~sel]), 'which = %d, %r: an unselected column was written' % (which, have)
        err = (got[:F] - want).abs()
        K = torch.where(torch.arange(45) < 36, torch.tensor(float(C.k_vjp(399))), torch.tensor(float(C.K_SIDE_OBJ))).to(torch.float64)
        bound = K * C.U * mag
        live = sel[None, :] & (bound > 0)
        dead = sel[None, :] & (bound == 0)
        assert float(err[dead.expand_as(err)].max() if dead.any() else 0.0) == 0.0, 'which = %d, %r: no upstream gradient, not zero' % (which, have)
        if live.any():
            r = err / bound.clamp_min(1e-300)
            for bit, cols in ((1, slice(0, 36)), (2, slice(36, 45))):
                if which & bit and bool(live[:, cols].any()):
                    worst[bit] = max(worst[bit], float(r[:, cols][live[:, cols]].max()))
    bounded('hn_pose_side_vjp F = %d, hand columns over %d combinations (observed / bound)' % (F, len(SIDE_COMBOS)), worst[1], 1.0, kind='ratio')
    bounded('hn_pose_side_vjp F = %d, object columns (observed / bound)' % F, worst[2], 1.0, kind='ratio')
    # which = 3 against hn_pose_chain_bwd: two summation orders of the same addends, each within its own bound of their exact sum
    out3, outb = cu(torch.full((F, 45), PREFILL, dtype=torch.float32)), nans(F, 36)
    L.check(lib.hn_pose_side_vjp(L.ptr(d_h), L.ptr(d_o), *[L.ptr(d_up[k]) for k in 'bjrtRT'], F, 3, L.ptr(out3), L.stream_ptr()), 'hn_pose_side_vjp')
    L.check(lib.hn_pose_chain_bwd(L.ptr(d_h), L.ptr(d_up['b']), L.ptr(d_up['j']), F, L.ptr(outb), L.stream_ptr()), 'hn_pose_chain_bwd')
    torch.cuda.synchronize()
    _, mag = C.vjp_f64(jac_h, np.concatenate([ups['b'], ups['j']], axis=1))
    hold('hn_pose_side_vjp (which = 3) hand half vs hn_pose_chain_bwd, F = %d' % F, out3[:, :36], C.f64(outb), (C.k_vjp(399) + C.K_CHAIN_BWD) * C.U * mag)


def test_pose_side_vjp_refusals():
    L, lib = _lib()
    d_h, d_o, out = f32(np.zeros((1, 399, 36))), f32(np.zeros((1, 412, 18))), nans(1, 45)
    n6 = [None] * 6
    st = L.stream_ptr()
    assert refused(lib.hn_pose_side_vjp(L.ptr(d_h), L.ptr(d_o), *n6, 1, 0, L.ptr(out), st), lib)
    assert refused(lib.hn_pose_side_vjp(None, L.ptr(d_o), *n6, 1, 1, L.ptr(out), st), lib)
    assert refused(lib.hn_pose_side_vjp(None, L.ptr(d_o), *n6, 1, 3, L.ptr(out), st), lib)
    assert refused(lib.hn_pose_side_vjp(L.ptr(d_h), None, *n6, 1, 2, L.ptr(out), st), lib)
    assert refused(lib.hn_pose_side_vjp(L.ptr(d_h), None, *n6, 1, 3, L.ptr(out), st), lib)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- hn_leaf_rows_gather / _scatter ---------------------------------------------------------------------------------------------------
def test_leaf_rows_gather_and_scatter_are_indexing():
    L, lib = _lib()
    leaves, g = C.leaf_case()
    n = C.LEAF_ROWS_N
    d_leaves = [f32(x) for x in leaves]
    ptrs = (ctypes.c_void_p * 6)(*[x.data_ptr() for x in d_leaves])
    rows = cu(torch.tensor(C.LEAF_ROWS, dtype=torch.long))
    F = len(C.LEAF_ROWS)
    prm_h, prm_o = nans(F + 1, 36), nans(F + 1, 18)
    L.check(lib.hn_leaf_rows_gather(ptrs, L.ptr(rows), F, n, L.ptr(prm_h), L.ptr(prm_o), L.stream_ptr()), 'hn_leaf_rows_gather')
    torch.cuda.synchronize()
    wh, wo = C.leaf_rows_gather_ref(leaves, C.LEAF_ROWS)
    assert np.array_equal(prm_h.cpu().numpy()[:F], wh, equal_nan=True) and np.array_equal(prm_o.cpu().numpy()[:F], wo, equal_nan=True)
    assert np.isnan(wh[4:]).all() and np.isnan(wo[4:, :9]).all() and not wo[:, 9:].any()           # rows -1 and 7; the unused inputs
    assert torch.isnan(prm_h[F]).all() and torch.isnan(prm_o[F]).all()
    # scatter, every (row, column) its own value: each of the six blocks exactly; rows -1 and 7 write nothing (the guard rows behind
    # `out` and the untouched rows stay zero / NaN)
    def scatter(row_list):
        out = cu(torch.cat([torch.zeros(n * 45), torch.full((45,), NAN)]).to(torch.float32))
        r = cu(torch.tensor(row_list, dtype=torch.long))
        L.check(lib.hn_leaf_rows_scatter(L.ptr(f32(g[:len(row_list)])), L.ptr(r), len(row_list), n, L.ptr(out), L.stream_ptr()), 'hn_leaf_rows_scatter')
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.isnan(o[n * 45:]).all()
        blocks, at = [], 0
        for leaf in (0, 1, 2, 3, 4, 5):                       # the layout of `out`: the six blocks in the leaves' order
            w = C.LEAF_WIDTHS[leaf]
            blocks.append(o[at:at + n * w].reshape(n, w))
            at += n * w
        return blocks
    got = scatter(C.LEAF_ROWS_SCATTER)
    want = C.leaf_rows_scatter_ref(g, C.LEAF_ROWS_SCATTER, n)
    for leaf in range(6):
        assert np.array_equal(got[leaf], want[leaf]), 'scatter: block %d' % leaf
    # a repeated row: one of its writers' values, whole columns from either
    got = scatter(C.LEAF_ROWS_REPEAT)
    want, alts = C.leaf_rows_scatter_ref(g, C.LEAF_ROWS_REPEAT, n, candidates=True)
    for leaf in range(6):
        cands = np.stack([v for r, v in alts[leaf] if r == 3])
        assert all(got[leaf][3, c] in cands[:, c] for c in range(C.LEAF_WIDTHS[leaf])), 'scatter, repeated row: block %d' % leaf
        others = [r for r in range(n) if r != 3]
        assert np.array_equal(got[leaf][others], want[leaf][others])


# ---- hn_adam_step ----------------------------------------------------------------------------------------------------------------------
B1, B2, EPS = 0.9, 0.999, 1e-8


def _adam(lib, L, blocks, n=None, steps=None, null_at=None):
    """One hn_adam_step over the blocks; each device buffer is one element longer than its block (a guard that must keep its value; a
    zero-length block still has a pointer)."""
    n = len(blocks) if n is None else n
    dev = [{k: cu(torch.from_numpy(np.concatenate([b[k], np.float32([123.0])]))) for k in 'pgmv'} for b in blocks]
    arr = lambda k: (ctypes.c_void_p * n)(*[(None if (null_at == (i, k)) else dev[i][k].data_ptr()) for i in range(n)])
    sizes = (ctypes.c_int * n)(*[blocks[i]['p'].size for i in range(n)])
    lrs = (ctypes.c_float * n)(*[blocks[i]['lr'] for i in range(n)])
    st = (ctypes.c_int * n)(*(steps if steps is not None else [blocks[i]['step'] for i in range(n)]))
    rc = lib.hn_adam_step(n, arr('p'), arr('g'), arr('m'), arr('v'), sizes, lrs, B1, B2, EPS, st, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dev


def _adam_compare(tag, blocks, dev):
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for t, (b, d) in enumerate(zip(blocks, dev)):
        n = b['p'].size
        got = {k: d[k].cpu().numpy() for k in 'pgmv'}
        for k in 'pgmv':
            assert got[k][n] == 123.0, '%s block %d: %s written past its end' % (tag, t, k)
        assert np.array_equal(got['g'][:n], b['g'])
        p64, m64, v64, dp = C.adam_f64(b['p'], b['g'], b['m'], b['v'], b['lr'], B1, B2, EPS, b['step'])
        bp, bm, bv = C.adam_bounds(p64, m64, v64, dp)
        for k, want, bnd in (('p', p64, bp), ('m', m64, bm), ('v', v64, bv)):
            x = got[k][:n].astype(np.float64)
            assert np.isfinite(x).all(), (tag, t, k)
            err = np.abs(x - want)
            assert (err[bnd == 0] == 0).all(), '%s block %d: %s moved where the update is exactly zero' % (tag, t, k)
            if (bnd > 0).any():
                worst[k] = max(worst[k], float((err[bnd > 0] / bnd[bnd > 0]).max()))
        still = (b['g'] == 0) & (b['m'] == 0) & (b['v'] == 0)
        assert np.array_equal(got['p'][:n][still], b['p'][still]), '%s block %d: zero gradient on zero moments moved p' % (tag, t)
    for k in 'pmv':
        bounded('hn_adam_step %s: %s (observed / bound)' % (tag, k), worst[k], 1.0, kind='ratio')


def test_adam_step_sixteen_blocks():
    """(a) 16 blocks, three of them empty, sizes around the 256-thread block and the 1024-element grid step, per-block step counts 1 .. 16
    and learning rates: the walk from element to (block, offset) across every boundary."""
    L, lib = _lib()
    blocks = C.adam_case(C.ADAM_SIZES_16, 1)
    rc, dev = _adam(lib, L, blocks)
    L.check(rc, 'hn_adam_step')
    _adam_compare('16 blocks', blocks, dev)


@pytest.mark.parametrize('sizes', C.ADAM_BIG)
def test_adam_step_grid_thresholds(sizes):
    """(b) totals above 65 536 (64 blocks of threads) and above 262 144 (256: every thread strides over several elements and blocks)."""
    L, lib = _lib()
    blocks = C.adam_case(sizes, 2)
    rc, dev = _adam(lib, L, blocks)
    L.check(rc, 'hn_adam_step')
    _adam_compare('%d x %d' % (len(sizes), sizes[0]), blocks, dev)


def test_adam_step_refusals():
    L, lib = _lib()
    blocks = C.adam_case((4,) * 17, 3, first_step=True)
    before = [b['p'].copy() for b in blocks]
    rc, dev = _adam(lib, L, blocks)                                      # 17 blocks
    assert refused(rc, lib)
    rc2, dev2 = _adam(lib, L, blocks, n=2, steps=[1, 0])                 # a step count of 0
    assert refused(rc2, lib)
    rc3, dev3 = _adam(lib, L, blocks, n=2, null_at=(1, 'm'))             # a NULL block pointer
    assert refused(rc3, lib)
    for d in (dev, dev2, dev3):
        for b0, x in zip(before, d):
            assert np.array_equal(x['p'].cpu().numpy()[:4], b0)


# ---- PoseAdam advances the parameters' version counters -------------------------------------------------------------------------------
def _step_all(modules, seed):
    from honerf_amd import fitting as F
    params = [p for m in modules for p in m.parameters()]
    gen = torch.Generator().manual_seed(seed)
    opt = F.PoseAdam([{'params': params, 'lr': 1e-2}])
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).to(p.device)
    versions = [p._version for p in params]
    opt.step()
    torch.cuda.synchronize()
    return params, versions


def test_pose_adam_step_reaches_a_standalone_module():
    """module.sdf(x) after PoseAdam.step() is the stepped weights' answer: the bits of a fresh module loaded with the stepped
    state_dict, and not the answer from before the step (the packed copy is keyed on the parameters' version counters, which a write
    through raw pointers does not advance by itself)."""
    from honerf_amd import nets
    net = nets.SDFNetwork_OBJ().cuda()
    net.reset_parameters(11)
    x = cu(torch.randn(64, 3, generator=torch.Generator().manual_seed(0)) * 0.3)
    with torch.no_grad():
        before = net.sdf(x).clone()
        params, versions = _step_all([net], 1)
        after = net.sdf(x).clone()
        fresh = nets.SDFNetwork_OBJ()
        fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
        want = fresh.cuda().sdf(x).clone()
    torch.cuda.synchronize()
    assert not torch.equal(want, before), 'the step did not change the function: the test would prove nothing'
    assert torch.equal(after, want), 'sdf() after the step is stale: max |after - stepped| %g, max |after - before| %g' % (
        float((after - want).abs().max()), float((after - before).abs().max()))
    assert all(p._version > v for p, v in zip(params, versions)), 'PoseAdam.step() left a version counter where it was'


def test_pose_adam_step_reaches_the_renderer_field():
    """The same through NeuSRenderer.field(), without mark_parameters_changed()."""
    from honerf_amd import nets
    from honerf_amd.renderer import NeuSRenderer

    def build():
        return nets.SDFNetwork_OBJ().cuda(), nets.SingleVarianceNetwork(0.3).cuda(), nets.RenderingNetwork_OBJ().cuda()
    sdf_net, var, col = build()
    sdf_net.reset_parameters(11)
    col.reset_parameters(12)
    ren = NeuSRenderer(sdf_net, var, col, 'obj', 32, 0, 0, 4, 1.0)
    x = cu(torch.randn(64, 3, generator=torch.Generator().manual_seed(0)) * 0.3)
    with torch.no_grad():
        before = ren.field().sdf(x).clone()
        _step_all([sdf_net, var, col], 2)
        after = ren.field().sdf(x).clone()
        f_sdf, f_var, f_col = build()
        for dst, src in ((f_sdf, sdf_net), (f_var, var), (f_col, col)):
            dst.load_state_dict({k: v.detach().clone() for k, v in src.state_dict().items()})
        want = NeuSRenderer(f_sdf, f_var, f_col, 'obj', 32, 0, 0, 4, 1.0).field().sdf(x).clone()
    torch.cuda.synchronize()
    assert not torch.equal(want, before)
    assert torch.equal(after, want), 'field() after the step is stale: max |after - stepped| %g, max |after - before| %g' % (
        float((after - want).abs().max()), float((after - before).abs().max()))
