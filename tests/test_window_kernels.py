"""GPU tests of the fitting_video window kernels (ho-nerf_amd/csrc/hn_fit_window.hip), one entry point at a time through the
C ABI, against a float64 torch restatement of the same operation on the same (fp32) inputs:
  hn_mat3_inverse / _bwd     torch.linalg.inv and its autograd
  hn_stable_pts / _bwd       R_f p[f, ::stride] + t_f and its autograd w.r.t. (obj_r, obj_t)
  hn_stable_value            get_stable_loss_cross behind a given hand sdf (stable_f64: scipy's cKDTree for the nearest outside
                             vertex; with strict_reference it is oracle.losses.stable_loss_cross, checked case by case)
  hn_window_loss / _bwd      fitting_video.py:285-334 for a window of F frames (window_loss_f64; oracle.losses.video_step_loss is
                             the same statements for F = 4, and pins the restatement there)
and the refusals of the host side.  Bounds: 1e-5 relative (short fp32 reductions against float64), cond(R)-scaled for the
inverse, bit-exact where the result is a copy or a re-run of the same launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

from helpers import assert_close, bounded
from oracle import losses as ol

pytestmark = pytest.mark.gpu

RT = 1e-5                  # values and gradients of the stable-term and window kernels against float64 (observed on MI355X: <= 2.6e-7,
                           # the window's mask term 6.5e-7)
EPS32 = 2.0 ** -23
# hn_mat3_inverse: the adjugate has no pivoting, its error grows with cond(R).  Per matrix, max |Y - Y64| / max |Y64| <= INV_K cond eps;
# the adjoint, max |gR - gR64| / (max |Y64|^2 max |g|) <= INV_BWD_K cond eps.  (A float32 emulation of the kernel's statements peaks at
# 2.1 and 8.4 over 20 000 rotations; both constants keep a factor ~4 for the device's FMA contraction.  Observed on MI355X: 1.7, 4.8.)
INV_K, INV_BWD_K = 8.0, 32.0
WEIGHTS = (0.5, 30.0, 20.0, 30.0, 20.0, 50.0, 100.0)      # autograd.FitWindowLossFn.WEIGHTS (the reference's)
NJ = 21


@pytest.fixture(scope='module')
def L():
    from honerf_amd import lib
    return lib


@pytest.fixture(scope='module')
def lib(L):
    return L.load()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(x):
    return x.detach().to('cuda', torch.float32).contiguous()


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _rotations(n, g):
    return ol.rot6d_to_matrix(torch.randn(n, 6, generator=g, dtype=torch.float64))


def _well_conditioned(n, g):
    """U diag(s) V^T: singular values 1 and 10 and one in between (cond = 10), either sign of the determinant, scale 0.5..2."""
    U, V = _rotations(n, g), _rotations(n, g)
    s = torch.exp(torch.rand(n, 3, generator=g, dtype=torch.float64) * np.log(10.0))
    s[:, 0], s[:, 1] = 1.0, 10.0
    s[:, 2] *= torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    scale = 0.5 + 1.5 * torch.rand(n, 1, 1, generator=g, dtype=torch.float64)
    return (U * s[:, None, :]) @ V.transpose(1, 2) * scale


# ---- hn_mat3_inverse / _bwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['rotation', 'general'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_mat3_inverse_and_adjoint_against_float64(L, lib, n, kind):
    g = _gen(100 + n)
    R32 = (_rotations(n, g) if kind == 'rotation' else _well_conditioned(n, g)).float()
    R64 = R32.double()
    cond = torch.linalg.cond(R64).numpy()
    Rd = _dev(R32)
    Y = _nan(n, 9)
    L.check(lib.hn_mat3_inverse(L.ptr(Rd), n, L.ptr(Y), L.stream_ptr()), 'hn_mat3_inverse')
    Gd = _dev(torch.randn(n, 9, generator=g))
    gR = _nan(n, 9)
    L.check(lib.hn_mat3_inverse_bwd(L.ptr(Y), L.ptr(Gd), n, L.ptr(gR), L.stream_ptr()), 'hn_mat3_inverse_bwd')
    torch.cuda.synchronize()
    Yh, gRh, G = Y.cpu().double(), gR.cpu().double(), Gd.cpu().double()
    # values: torch.linalg.inv in float64, per matrix, relative to cond(R) eps
    R_req = R64.clone().requires_grad_(True)
    Y64 = torch.linalg.inv(R_req)
    (Y64 * G.view(n, 3, 3)).sum().backward()
    Y64 = Y64.detach().reshape(n, 9)
    y_mag = Y64.abs().max(1).values
    err = ((Yh - Y64).abs().max(1).values / y_mag).numpy()
    bounded('hn_mat3_inverse %s n=%d: max_i err_i / (cond_i eps)' % (kind, n), float((err / (cond * EPS32)).max()), INV_K, kind='cond-scaled')
    # adjoint: float64 autograd of torch.linalg.inv at a random upstream gradient
    gR64 = R_req.grad.reshape(n, 9)
    scale = y_mag ** 2 * G.abs().max(1).values
    e_bwd = ((gRh - gR64).abs().max(1).values / scale).numpy()
    bounded('hn_mat3_inverse_bwd %s n=%d: max_i err_i / (cond_i eps) vs autograd' % (kind, n), float((e_bwd / (cond * EPS32)).max()), INV_BWD_K,
            kind='cond-scaled')
    # the documented formula on the kernel's own Y: g_R = -Y^T g Y^T
    Ym, Gm = Yh.view(n, 3, 3), G.view(n, 3, 3)
    assert_close(gRh.view(n, 3, 3), -(Ym.transpose(1, 2) @ Gm @ Ym.transpose(1, 2)), RT, 'hn_mat3_inverse_bwd %s n=%d: -Y^T g Y^T' % (kind, n))


# ---- hn_stable_pts / _bwd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 10, 10000])
@pytest.mark.parametrize('n_verts', [1, 9, 10, 11, 2565, 10240])
def test_stable_pts_and_adjoint_against_float64(L, lib, n_verts, stride):
    F = 3
    g = _gen(7 * n_verts + stride)
    V = (n_verts + stride - 1) // stride
    pts = (0.1 * torch.randn(F, n_verts, 3, generator=g)).float()
    R32 = _rotations(F, g).float()
    t32 = (0.05 * torch.randn(F, 3, generator=g)).float()
    pd, Rd, td = _dev(pts), _dev(R32), _dev(t32)
    pw, p0 = _nan(F * V, 3), _nan(V, 3)
    pw_nop0 = _nan(F * V, 3)
    L.check(lib.hn_stable_pts(L.ptr(pd), F, n_verts, stride, L.ptr(Rd), L.ptr(td), L.ptr(pw), L.ptr(p0), L.stream_ptr()), 'hn_stable_pts')
    L.check(lib.hn_stable_pts(L.ptr(pd), F, n_verts, stride, L.ptr(Rd), L.ptr(td), L.ptr(pw_nop0), None, L.stream_ptr()), 'hn_stable_pts (p0 NULL)')
    gd = _dev(torch.randn(F, V, 3, generator=g))
    gR, gt = _nan(F, 9), _nan(F, 3)
    L.check(lib.hn_stable_pts_bwd(L.ptr(pd), F, n_verts, stride, L.ptr(gd), L.ptr(gR), L.ptr(gt), L.stream_ptr()), 'hn_stable_pts_bwd')
    torch.cuda.synchronize()
    sel = pts[:, ::stride]
    assert sel.shape[1] == V
    assert torch.equal(p0.cpu(), sel[0]), 'p0 is not frame 0\'s selected vertices bit for bit'
    assert torch.equal(pw_nop0, pw), 'pts_world depends on whether p0 is written'
    R64 = R32.double().requires_grad_(True)
    t64 = t32.double().requires_grad_(True)
    ref = torch.einsum('frc,fvc->fvr', R64, sel.double()) + t64[:, None]
    assert_close(pw.cpu().view(F, V, 3), ref.detach(), RT, 'hn_stable_pts n_verts=%d stride=%d' % (n_verts, stride))
    (ref * gd.cpu().double()).sum().backward()
    assert_close(gR.cpu().view(F, 3, 3), R64.grad, RT, 'hn_stable_pts_bwd g_obj_r n_verts=%d stride=%d' % (n_verts, stride))
    assert_close(gt.cpu(), t64.grad, RT, 'hn_stable_pts_bwd g_obj_t n_verts=%d stride=%d' % (n_verts, stride))


# ---- hn_stable_value ----------------------------------------------------------------------------------------------------------------
def _spread_points(V, g, d_min=0.02):
    """V points in the unit cube at least d_min apart (greedy rejection), fp32-representable."""
    out = torch.empty(0, 3, dtype=torch.float64)
    while out.shape[0] < V:
        c = torch.rand(4 * V + 16, 3, generator=g).double().float().double()
        for p in c:
            if out.shape[0] == 0 or float(((out - p) ** 2).sum(1).min()) >= d_min * d_min:
                out = torch.cat([out, p[None]])
                if out.shape[0] == V:
                    break
    return out


def _nearest_margin(p0, inside, strict):
    """Premise of the comparison: for every query (inside vertex of a penetrating frame) the nearest candidate is nearer than the
    second one by a relative margin far above fp32 rounding (~6e-7 of a squared distance), so that the kernel's fp32 distances choose what float64 chooses."""
    d2 = ((p0[:, None] - p0[None]) ** 2).sum(-1)
    worst = np.inf
    for f in range(inside.shape[0]):
        if not inside[f].any():
            continue
        cand = _candidates(inside[f], strict)
        if cand.sum() < 2:
            continue
        d = d2[inside[f]][:, cand].sort(1).values
        worst = min(worst, float(((d[:, 1] - d[:, 0]) / d[:, 1].clamp_min(1e-30)).min()))
    return worst


def _candidates(in_f, strict):
    V = in_f.shape[0]
    if not strict:
        return ~in_f
    cand = torch.ones(V, dtype=torch.bool)      # np.setdiff1d(range(V), boolean mask): removes 1 if any inside, 0 if any outside
    if V > 1 and in_f.any():
        cand[1] = False
    if (~in_f).any():
        cand[0] = False
    return cand


def stable_f64(sdf, p0, strict):
    """get_stable_loss_cross from the sdf [F,V] of the selected vertices and their frame-0 positions p0 [V,3], float64, the nearest
    outside vertex by scipy's cKDTree as in the reference.  strict: the reference's 'outside' set (quirk B-12: then this is
    oracle.losses.stable_loss_cross, which the test checks); else the complement of the inside set, the product's corrected reading,
    where a penetrating frame whose every vertex is inside has no outside vertex and contributes no outside term."""
    from scipy import spatial
    F, V = sdf.shape
    inside = sdf.detach() < 0
    pen = [f for f in range(F) if inside[f].any()]
    if len(pen) <= 1:
        return sdf.sum() * 0.0
    S, T = sdf[pen], len(pen)
    value = 0.0
    for f in pen:
        in_f = inside[f]
        n_in = int(in_f.sum())
        value = value + S[:, in_f].clamp(0, 1e7).sum() / ((T - 1) * n_in)
        cand = _candidates(in_f, strict)
        if cand.any():
            _, k = spatial.cKDTree(p0[cand].numpy()).query(p0[in_f].numpy(), k=1)
            near = torch.nonzero(cand)[:, 0][torch.from_numpy(np.unique(k))]
            value = value + 0.05 * S[:, near].clamp(-1e7, 0).abs().sum() / ((T - 1) * n_in)
    return value / T


def _oracle_stable(sdf64, p0):
    """oracle.losses.stable_loss_cross (the reference's statements, quirk B-12 included, scipy cKDTree) with the given sdf standing
    for the hand field and identity Ro / To: its points pts[:, ::10] are p0 in every frame."""
    F, V = sdf64.shape
    pts = torch.zeros(F, 10 * (V - 1) + 1, 3, dtype=torch.float64)
    pts[:, ::10] = p0
    Ro, To = torch.eye(3, dtype=torch.float64).expand(F, 3, 3), torch.zeros(F, 3, dtype=torch.float64)
    v = ol.stable_loss_cross(lambda p, b, tp: sdf64.reshape(-1, 1), pts, None, None, Ro, To)
    return v if isinstance(v, torch.Tensor) else sdf64.sum() * 0.0


def _stable_case(F, V, pattern, seed):
    g = _gen(seed)
    p0 = _spread_points(V, g, d_min=min(0.02, 0.5 / max(V, 1) ** (1 / 3)))
    mag = 1e-3 + 0.05 * torch.rand(F, V, generator=g).double()
    inside = torch.zeros(F, V, dtype=torch.bool)
    if pattern == 'one':
        inside[F // 2] = torch.rand(V, generator=g) < 0.4
        inside[F // 2, 0] = True
    elif pattern in ('all', 'full'):
        inside = torch.rand(F, V, generator=g) < 0.35
        inside[:, torch.randint(V, (F,), generator=g)] = True    # every frame penetrates
        inside[torch.arange(F), torch.randint(V, (F,), generator=g)] = True
        if pattern == 'full':
            inside[F - 1] = True                                   # a frame with every vertex inside
    sdf = torch.where(inside, -mag, mag).float()
    sdf[:, 3::7][~inside[:, 3::7]] = 0.0                           # exact zeros: outside (the reference's `< 0`), gradient of the inside clip
    return sdf, p0.float()


STABLE_FV = [(F, V) for F in (1, 2, 4, 8) for V in (1, 2, 17, 1024)]


@pytest.mark.parametrize('strict', [0, 1])
@pytest.mark.parametrize('pattern', ['none', 'one', 'all', 'full'])
@pytest.mark.parametrize('F,V', STABLE_FV)
def test_stable_value_against_the_oracle(L, lib, F, V, pattern, strict):
    sdf32, p032 = _stable_case(F, V, pattern, seed=1000 * F + 10 * V + len(pattern))
    inside = sdf32 < 0
    margin = _nearest_margin(p032.double(), inside, strict)
    assert margin > 1e-5, 'test data: nearest-vertex margin %.1e too small for an fp32 / fp64 comparison' % margin
    need = lib.hn_stable_value_scratch_bytes(F, V)
    scr = torch.zeros(need, dtype=torch.uint8, device='cuda')
    val_d = _nan(1 + F * V)
    sd, pd = _dev(sdf32), _dev(p032)
    L.check(lib.hn_stable_value(L.ptr(sd), L.ptr(pd), F, V, strict, L.ptr(val_d[0:1]), L.ptr(val_d[1:]), L.ptr(scr), need, L.stream_ptr()),
            'hn_stable_value')
    torch.cuda.synchronize()
    got_v, got_d = float(val_d[0]), val_d[1:].cpu().view(F, V).double()
    assert int(scr[:4].view(torch.int32)[0]) == 0, 'hn_stable_value left its counter non-zero'
    sdf64 = sdf32.double().requires_grad_(True)
    ref = stable_f64(sdf64, p032.double(), bool(strict))
    ref_v = float(ref.detach())
    if strict:              # strict_reference: the restatement is the reference's own statements
        orc = _oracle_stable(sdf64, p032.double())
        orc_v = float(orc.detach())
        assert abs(ref_v - orc_v) <= 1e-12 * max(1.0, abs(orc_v)), (ref_v, orc_v)
    (d_ref,) = torch.autograd.grad(ref, sdf64) if ref.requires_grad else (torch.zeros(F, V, dtype=torch.float64),)
    tag = 'hn_stable_value F=%d V=%d %s strict=%d' % (F, V, pattern, strict)
    n_pen = int(inside.any(1).sum())
    if n_pen <= 1:          # in_time 0 or 1: the term is 0 and so is its gradient, exactly
        assert got_v == 0.0 and ref_v == 0.0, (got_v, ref_v)
        assert torch.count_nonzero(got_d) == 0, tag + ': d_sdf not all zero'
        bounded(tag + ': value (0)', abs(got_v), 0.0, kind='abs')
        return
    if ref_v == 0.0:        # every penetrating frame wholly inside and no outside vertex (non-strict, V <= 2): no term survives
        bounded(tag + ': value (0)', abs(got_v), 0.0, kind='abs')
    else:
        bounded(tag + ': value', abs(got_v - ref_v) / abs(ref_v), RT)
    assert_close(got_d, d_ref, RT, tag + ': d_sdf vs autograd')


def test_stable_value_ties_go_to_the_lowest_index(L, lib):
    """Two outside vertices at exactly the same distance from an inside vertex (exact in fp32 and fp64): the nearest one is the lower
    index.  Vertex 0's tie is between 5 and 69 (the same lane of the wave's scan), vertex 2's between 3 and 4 (neighbouring lanes, the
    cross-lane reduction).  Expectation by hand, not by cKDTree (whose tie order is unspecified)."""
    V, F = 70, 2
    p0 = torch.stack([torch.tensor([100.0 + 3 * k, 50.0, 50.0]) for k in range(V)])   # far apart, far from the queries
    p0[0], p0[5], p0[69] = torch.tensor([0.0, 0, 0]), torch.tensor([0.25, 0, 0]), torch.tensor([-0.25, 0, 0])
    p0[2], p0[3], p0[4] = torch.tensor([10.0, 0, 0]), torch.tensor([10.25, 0, 0]), torch.tensor([9.75, 0, 0])
    sdf = torch.full((F, V), 0.5)
    sdf[0, 0], sdf[0, 2] = -0.1, -0.2        # frame 0: inside {0, 2}; nearest outside: 5 (not 69), 3 (not 4)
    sdf[1, 5], sdf[1, 3] = -0.3, -0.4        # frame 1: inside {5, 3}; nearest outside: 0, 2 (no ties)
    sdf[1, 0], sdf[1, 2] = 0.125, 0.375
    sdf[0, 5], sdf[0, 3] = 0.0625, 0.25
    # in_time 2 (denominators (2 - 1) x 2):  frame 0: in (0.125 + 0.375) / 2, out 0.05 (0.3 + 0.4) / 2;  frame 1: in (0.0625 + 0.25) / 2,
    # out 0.05 (0.1 + 0.2) / 2;  all over in_time = 2
    expect = ((0.125 + 0.375) / 2 + 0.05 * 0.7 / 2 + (0.0625 + 0.25) / 2 + 0.05 * 0.3 / 2) / 2
    need = lib.hn_stable_value_scratch_bytes(F, V)
    scr = torch.zeros(need, dtype=torch.uint8, device='cuda')
    val_d = _nan(1 + F * V)
    sd, pd = _dev(sdf), _dev(p0)
    L.check(lib.hn_stable_value(L.ptr(sd), L.ptr(pd), F, V, 0, L.ptr(val_d[0:1]), L.ptr(val_d[1:]), L.ptr(scr), need, L.stream_ptr()),
            'hn_stable_value')
    torch.cuda.synchronize()
    d = val_d[1:].cpu().view(F, V)
    bounded('hn_stable_value tie: value', abs(float(val_d[0]) - expect) / expect, RT)
    # selected by frame 0 and inside in frame 1: d = (-0.05 Wout) / in_time = -0.05 (1/2) / 2; the losers of the ties: 0
    assert float(d[1, 5]) == pytest.approx(-0.0125, rel=1e-6) and float(d[1, 3]) == pytest.approx(-0.0125, rel=1e-6), d[1, [3, 5]]
    assert float(d[1, 69]) == 0.0 and float(d[1, 4]) == 0.0, d[1, [4, 69]]


def test_stable_value_scratch_is_reusable_across_grid_sizes(L, lib):
    """The scratch is zeroed ONCE and handed over again at every launch (autograd.StableTerm): every launch must leave its counter
    at zero, whatever the grid size of the launch before.  Each launch of a sequence of different sizes on one scratch equals the
    same launch on fresh scratch, bit for bit."""
    seq = [(8, 1024), (1, 1), (4, 17), (2, 1024), (8, 2), (3, 300), (8, 1024), (5, 100), (2, 2), (8, 1000), (4, 1024), (1, 17)]
    need_max = max(lib.hn_stable_value_scratch_bytes(F, V) for F, V in seq)
    shared = torch.zeros(need_max, dtype=torch.uint8, device='cuda')
    for k, (F, V) in enumerate(seq):
        sdf32, p032 = _stable_case(F, V, 'all', seed=77 + k)
        sd, pd = _dev(sdf32), _dev(p032)
        need = lib.hn_stable_value_scratch_bytes(F, V)
        outs = []
        for scr in (shared, torch.zeros(need, dtype=torch.uint8, device='cuda')):
            val_d = _nan(1 + F * V)
            L.check(lib.hn_stable_value(L.ptr(sd), L.ptr(pd), F, V, 1, L.ptr(val_d[0:1]), L.ptr(val_d[1:]), L.ptr(scr), scr.numel(),
                                        L.stream_ptr()), 'hn_stable_value')
            outs.append(val_d)
        torch.cuda.synchronize()
        assert int(shared[:4].view(torch.int32)[0]) == 0, 'launch %d (%d x %d) left the counter non-zero' % (k, F, V)
        assert not torch.isnan(outs[0]).any(), 'launch %d (%d x %d) on re-used scratch wrote no result' % (k, F, V)
        assert torch.equal(outs[0], outs[1]), 'launch %d (%d x %d): re-used scratch differs from fresh scratch' % (k, F, V)


# ---- hn_window_loss / _bwd ----------------------------------------------------------------------------------------------------------
def window_loss_f64(color, wsum, true_rgb, true_mask, sdf_h, sdf_o, joint_3d, joint_pred, R, t, Rp, tp, verts, stable, anchor, w=WEIGHTS):
    """fitting_video.py:285-334 for a window of F = joint_3d.shape[0] frames (oracle.losses.video_step_loss is the same for F = 4):
    color / true_rgb [n,3], wsum / true_mask [n] (all rays of the window), sdf_h / sdf_o [m], joint_3d / joint_pred [F,21,3], R / Rp
    [F,3,3], t / tp [F,3], verts [V,3]; anchor bit 0 / bit 1: the smoothness term is anchored at the first / (else) the last frame.
    Returns (loss, terms10) as hn_window_loss: {loss, colour, mask, contact, penetration, joint, verts, w5 smooth, w6 stable, 0}."""
    color_loss = ((color - true_rgb) * true_mask[:, None]).abs().sum() / true_mask.shape[0]
    mask_loss = tF.binary_cross_entropy(wsum.clip(1e-3, 1.0 - 1e-3), true_mask)
    contact, penet = ol.interaction_terms(sdf_h[:, None], sdf_o[:, None])
    pv = (R[:, None] @ verts[None, :, :, None])[..., 0] + t[:, None]       # pred_obj_v_w
    cv = (Rp[:, None] @ verts[None, :, :, None])[..., 0] + tp[:, None]     # compare_obj_v_w
    joint = ol.pose_loss_video(joint_3d, joint_pred)
    verts_l = ol.pose_loss_video(pv, cv)
    smooth = ol.pose_loss_video(joint_3d[1:], joint_3d[:-1]) + ol.pose_loss_video(pv[1:], pv[:-1])
    if anchor & 1:
        smooth = smooth + ol.pose_loss_video(joint_3d[:1], joint_pred[:1]) + ol.pose_loss_video(pv[:1], cv[:1])
    elif anchor & 2:
        smooth = smooth + ol.pose_loss_video(joint_3d[-1:], joint_pred[-1:]) + ol.pose_loss_video(pv[-1:], cv[-1:])
    st = stable if stable is not None else torch.zeros((), dtype=color.dtype)
    loss = (w[0] * (color_loss + 0.5 * mask_loss) + (w[1] * contact + w[2] * penet) + (w[3] * joint + w[4] * verts_l) + w[5] * smooth
            + w[6] * st)
    z = torch.zeros((), dtype=color.dtype)
    return loss, [loss, color_loss, mask_loss, contact, penet, joint, verts_l, w[5] * smooth, w[6] * st, z]


def _sdf_pair(m, sets, g):
    """sdf_hand, sdf_obj [m] at least 1e-4 from 0 and |sh| + |so| at least 1e-4 from the 1e-2 contact threshold: fp32 and float64
    select the same samples.  'empty': no contact, no penetration; 'large': both sets hold a large share of the samples."""
    def mags(small):
        lo, hi = (1e-4, 4.9e-3) if small else (1.1e-2, 0.5)
        return lo + (hi - lo) * torch.rand(m, generator=g)
    sign = lambda: torch.where(torch.rand(m, generator=g) < 0.5, -1.0, 1.0)
    if sets == 'empty':
        return mags(False), sign() * mags(False)
    small_h, small_o = torch.rand(m, generator=g) < 0.5, torch.rand(m, generator=g) < 0.5
    sh = sign() * torch.where(small_h, mags(True), mags(False))
    so = sign() * torch.where(small_o, mags(True), mags(False))
    return sh, so


def _window_case(F, n_rays, n_samples, sets, zero_norm, seed, n_verts=300, with_stable=True):
    g = _gen(seed)
    c = {}
    c['color'] = torch.rand(n_rays, 3, generator=g)
    c['true_rgb'] = torch.rand(n_rays, 3, generator=g)
    c['true_mask'] = (torch.rand(n_rays, generator=g) < 0.6).float()
    w = torch.rand(n_rays, generator=g) * 0.98 + 0.01
    w[::5] = 5e-4                       # below the clip (no gradient); away from the clip bounds by far more than fp32 rounding
    w[1::7] = 1.0 - 5e-4
    c['wsum'] = w
    c['sdf_h'], c['sdf_o'] = _sdf_pair(n_samples, sets, g)
    c['joint_pred'] = 0.1 * torch.randn(F, NJ, 3, generator=g)
    c['Rp'] = _rotations(F, g).float()
    c['tp'] = 0.05 * torch.randn(F, 3, generator=g)
    if zero_norm:       # the first step of a window: the chain starts at the prediction, every |e| of the regularisers is 0
        c['joint_3d'], c['R'], c['t'] = c['joint_pred'].clone(), c['Rp'].clone(), c['tp'].clone()
    else:
        c['joint_3d'] = c['joint_pred'] + 0.01 * torch.randn(F, NJ, 3, generator=g)
        c['R'] = (c['Rp'].double() @ ol.rot6d_to_matrix(torch.tensor([[1.0, 0, 0, 1, 0, 0]], dtype=torch.float64) +
                                                         0.05 * torch.randn(F, 6, generator=g, dtype=torch.float64))).float()
        c['t'] = c['tp'] + 0.01 * torch.randn(F, 3, generator=g)
    c['verts'] = 0.1 * torch.randn(n_verts, 3, generator=g)
    c['stable'] = torch.tensor(0.0123 + 0.01 * float(torch.rand(1, generator=g))) if with_stable else None
    return {k: (v.float().contiguous() if v is not None else None) for k, v in c.items()}


def _run_window(L, lib, c, anchor, g_losses, scratch=None):
    """hn_window_loss, then hn_window_loss_bwd once per upstream gradient -> (terms10, [per g_loss: dict of gradients])."""
    F, n_rays, n_samples = c['joint_3d'].shape[0], c['color'].shape[0], c['sdf_h'].shape[0]
    d = {k: (_dev(v) if v is not None else None) for k, v in c.items()}
    need = lib.hn_window_loss_scratch_bytes(n_rays, n_samples)
    if scratch is None:
        scratch = torch.zeros(need, dtype=torch.uint8, device='cuda')
    sums, terms = _nan(6), _nan(10)
    gj, gR, gt = _nan(F * 63), _nan(F * 9), _nan(F * 3)
    w7 = (ctypes.c_float * 7)(*WEIGHTS)
    st = d['stable'].reshape(1) if d['stable'] is not None else None
    L.check(lib.hn_window_loss(L.ptr(d['color']), L.ptr(d['wsum']), L.ptr(d['true_rgb']), L.ptr(d['true_mask']), n_rays, L.ptr(d['sdf_h']),
                               L.ptr(d['sdf_o']), n_samples, L.ptr(d['joint_3d']), L.ptr(d['joint_pred']), F, L.ptr(d['R']), L.ptr(d['t']),
                               L.ptr(d['Rp']), L.ptr(d['tp']), L.ptr(d['verts']), d['verts'].shape[0], L.ptr(st), anchor, w7, L.ptr(scratch),
                               scratch.numel(), L.ptr(sums), L.ptr(terms), L.ptr(gj), L.ptr(gR), L.ptr(gt), L.stream_ptr()), 'hn_window_loss')
    grads = []
    for gl in g_losses:
        gld = torch.tensor([gl], device='cuda')
        o = {'color': _nan(n_rays, 3), 'wsum': _nan(n_rays), 'sdf_h': _nan(n_samples), 'sdf_o': _nan(n_samples), 'joint_3d': _nan(F, NJ, 3),
             'R': _nan(F, 3, 3), 't': _nan(F, 3), 'stable': _nan(1)}
        L.check(lib.hn_window_loss_bwd(L.ptr(d['color']), L.ptr(d['wsum']), L.ptr(d['true_rgb']), L.ptr(d['true_mask']), n_rays, L.ptr(d['sdf_h']),
                                       L.ptr(d['sdf_o']), n_samples, L.ptr(sums), L.ptr(gld), w7, L.ptr(gj), L.ptr(gR), L.ptr(gt), F, L.ptr(o['color']),
                                       L.ptr(o['wsum']), L.ptr(o['sdf_h']), L.ptr(o['sdf_o']), L.ptr(o['joint_3d']), L.ptr(o['R']), L.ptr(o['t']),
                                       L.ptr(o['stable']), L.stream_ptr()), 'hn_window_loss_bwd')
        grads.append(o)
    torch.cuda.synchronize()
    return terms.cpu(), [{k: v.cpu() for k, v in o.items()} for o in grads]


GRAD_KEYS = ('color', 'wsum', 'sdf_h', 'sdf_o', 'joint_3d', 'R', 't', 'stable')
TERM_NAMES = ('loss', 'colour', 'mask', 'contact', 'penetration', 'joint', 'verts', 'smooth x50', 'stable x100', 'zero')


def _check_window(L, lib, c, anchor, tag, g_losses=(1.0, 0.37)):
    terms, grads = _run_window(L, lib, c, anchor, g_losses)
    x = {k: (v.double().requires_grad_(k in GRAD_KEYS) if v is not None else None) for k, v in c.items()}
    loss, ref_terms = window_loss_f64(x['color'], x['wsum'], x['true_rgb'], x['true_mask'], x['sdf_h'], x['sdf_o'], x['joint_3d'], x['joint_pred'],
                                      x['R'], x['t'], x['Rp'], x['tp'], x['verts'], x['stable'], anchor)
    for k, (name, r) in enumerate(zip(TERM_NAMES, ref_terms)):
        r = float(r)
        e = abs(float(terms[k]) - r) / abs(r) if r != 0.0 else abs(float(terms[k]))
        bounded('%s: terms10[%d] %s' % (tag, k, name), e, RT if r != 0.0 else 0.0, kind='rel' if r != 0.0 else 'abs (reference 0)')
    keys = [k for k in GRAD_KEYS if x[k] is not None]
    g64 = dict(zip(keys, torch.autograd.grad(loss, [x[k] for k in keys])))
    for gl, got in zip(g_losses, grads):
        for k in keys:
            assert_close(got[k].reshape(g64[k].shape), gl * g64[k], RT, '%s g_loss=%g: d loss / d %s' % (tag, gl, k))


@pytest.mark.parametrize('zero_norm', [False, True])
@pytest.mark.parametrize('anchor', [0, 1, 2, 3])
@pytest.mark.parametrize('F', [2, 3, 4, 8])
def test_window_loss_pose_terms_against_float64(L, lib, F, anchor, zero_norm):
    """Every window size the kernel takes (its joint threads tf = tid / 21 and 12 F gradient threads scale with F), every anchor (0:
    the very first step, no anchor; 3: both bits, the start wins as in the reference's if / elif), and the zero-norm start."""
    c = _window_case(F, 40 * F, 256, 'large', zero_norm, seed=31 * F + 7 * anchor + int(zero_norm))
    _check_window(L, lib, c, anchor, 'hn_window_loss F=%d anchor=%d%s' % (F, anchor, ' zero-norm' if zero_norm else ''))


@pytest.mark.parametrize('with_stable', [True, False])
@pytest.mark.parametrize('sets', ['empty', 'large'])
@pytest.mark.parametrize('n_rays,n_samples', [(40, 40), (40, 256), (256, 257), (257, 256), (40, 4 * 40 * 192), (4 * 40 * 192, 257), (257, 40)])
def test_window_loss_sizes_and_sets_against_float64(L, lib, n_rays, n_samples, sets, with_stable):
    """One block and many in the last-block reduction (n_samples above and below n_rays); contact / penetration sets empty and
    large; the stable term given and NULL."""
    c = _window_case(4, n_rays, n_samples, sets, False, seed=n_rays + 3 * n_samples + len(sets), with_stable=with_stable)
    _check_window(L, lib, c, 1, 'hn_window_loss rays=%d samples=%d %s%s' % (n_rays, n_samples, sets, '' if with_stable else ' stable NULL'))


def test_window_loss_scratch_is_reusable_across_grid_sizes(L, lib):
    """The scratch's counter (the last-block reduction) must come back to zero after every launch: consecutive launches of different
    grid sizes on one scratch give what the same launch gives on fresh scratch, bit for bit."""
    sizes = [(4 * 40 * 192, 257), (40, 256), (257, 4 * 40 * 192), (40, 40), (4 * 40 * 192, 40)]
    need = max(lib.hn_window_loss_scratch_bytes(r, s) for r, s in sizes)
    shared = torch.zeros(need, dtype=torch.uint8, device='cuda')
    for k, (r, s) in enumerate(sizes):
        c = _window_case(3, r, s, 'large', False, seed=500 + k)
        t_shared, g_shared = _run_window(L, lib, c, 2, (0.37,), scratch=shared)
        t_fresh, g_fresh = _run_window(L, lib, c, 2, (0.37,))
        assert int(shared[:4].view(torch.int32)[0]) == 0, 'launch %d left the counter non-zero' % k
        assert not torch.isnan(t_shared).any(), 'launch %d (%d rays, %d samples) on re-used scratch wrote no terms' % (k, r, s)
        assert torch.equal(t_shared, t_fresh), 'launch %d: terms on re-used scratch differ from fresh scratch' % k
        for key in GRAD_KEYS:
            assert torch.equal(g_shared[0][key], g_fresh[0][key]), 'launch %d: gradient %s differs' % (k, key)


def test_window_restatement_is_video_step_loss_at_four_frames():
    """window_loss_f64 is fitting_video.py:285-334 generalised to F frames: at F = 4 it is oracle.losses.video_step_loss (the
    reference's statements, hard-wired to 4 frames through index[3]) for each anchor.  Needs no GPU."""
    c = _window_case(4, 4 * 40, 300, 'large', False, seed=4)
    x = {k: (v.double() if v is not None else None) for k, v in c.items()}
    P = 40
    ro = {'color_fine': x['color'].view(4, P, 3), 'weight_sum': x['wsum'].view(4, P, 1), 'sdf_hand': x['sdf_h'][:, None], 'sdf_obj': x['sdf_o'][:, None]}
    pv = (x['R'][:, None] @ x['verts'][None, :, :, None])[..., 0] + x['t'][:, None]
    cv = (x['Rp'][:, None] @ x['verts'][None, :, :, None])[..., 0] + x['tp'][:, None]
    # (index, data_num, later) of the reference -> anchor: first window of the sequence, last window, a middle one, the very first step
    for index, data_num, later, anchor in (([0, 1, 2, 3], 8, True, 1), ([4, 5, 6, 7], 8, True, 2), ([2, 3, 4, 5], 8, True, 0),
                                           ([0, 1, 2, 3], 4, False, 0), ([0, 1, 2, 3], 4, True, 3)):
        ref = ol.video_step_loss(ro, x['true_rgb'].view(4, P, 3), x['true_mask'].view(4, P, 1), x['joint_3d'], x['joint_pred'], pv, cv, index,
                                 data_num, later, stable=x['stable'])
        loss, terms = window_loss_f64(x['color'], x['wsum'], x['true_rgb'], x['true_mask'], x['sdf_h'], x['sdf_o'], x['joint_3d'], x['joint_pred'],
                                      x['R'], x['t'], x['Rp'], x['tp'], x['verts'], x['stable'], anchor)
        for name, mine in (('loss', terms[0]), ('color', terms[1]), ('mask', terms[2]), ('contact', terms[3]), ('penetration', terms[4]),
                           ('joint', terms[5]), ('obj_verts', terms[6]), ('smooth', terms[7]), ('stable', terms[8])):
            assert abs(float(mine) - float(ref[name])) <= 1e-12 * max(1.0, abs(float(ref[name]))), (anchor, name, float(mine), float(ref[name]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_window_kernels_refuse_what_they_do_not_take(L, lib):
    """Every bound the host side declares returns a status < 0 with a message in hn_last_error(), and launches nothing (the outputs
    keep their sentinel)."""
    s = L.stream_ptr()
    x = torch.zeros(4096, device='cuda')
    out = _nan(4096)

    def refused(rc, word):
        assert rc < 0, 'accepted (rc %d), expected a refusal mentioning %r' % (rc, word)
        msg = lib.hn_last_error()
        assert msg and word in msg, (word, msg)

    P = L.ptr
    # hn_mat3_inverse / _bwd: NULL arguments (n = 0 is an empty no-op, not an error)
    refused(lib.hn_mat3_inverse(None, 4, P(out), s), b'NULL')
    refused(lib.hn_mat3_inverse(P(x), 4, None, s), b'NULL')
    refused(lib.hn_mat3_inverse_bwd(P(x), None, 4, P(out), s), b'NULL')
    assert lib.hn_mat3_inverse(P(x), 0, P(out), s) == 0
    # hn_stable_pts / _bwd: n_verts < 1, n_frames < 1, stride < 1, NULL
    refused(lib.hn_stable_pts(P(x), 2, 0, 10, P(x), P(x), P(out), None, s), b'stable_pts')
    refused(lib.hn_stable_pts(P(x), 0, 10, 10, P(x), P(x), P(out), None, s), b'stable_pts')
    refused(lib.hn_stable_pts(P(x), 2, 10, 0, P(x), P(x), P(out), None, s), b'stable_pts')
    refused(lib.hn_stable_pts(None, 2, 10, 10, P(x), P(x), P(out), None, s), b'stable_pts')
    refused(lib.hn_stable_pts_bwd(P(x), 2, 0, 10, P(x), P(out), P(out), s), b'stable_pts_bwd')
    refused(lib.hn_stable_pts_bwd(P(x), 2, 10, 10, P(x), None, P(out), s), b'stable_pts_bwd')
    # hn_stable_value: n_frames 9 / 0, V 1025 / 0, NULL, scratch too small
    scr = torch.zeros(lib.hn_stable_value_scratch_bytes(8, 1024), dtype=torch.uint8, device='cuda')
    big = torch.zeros(9 * 1025 + 1, device='cuda')
    for F, V in ((9, 10), (0, 10), (2, 1025), (2, 0)):
        refused(lib.hn_stable_value(P(big), P(big), F, V, 0, P(out), P(out), P(scr), scr.numel(), s), b'at most')
    refused(lib.hn_stable_value(None, P(x), 2, 10, 0, P(out), P(out), P(scr), scr.numel(), s), b'NULL')
    refused(lib.hn_stable_value(P(x), P(x), 2, 10, 0, P(out), P(out), None, scr.numel(), s), b'NULL')
    refused(lib.hn_stable_value(P(x), P(x), 8, 1024, 0, P(out), P(out), P(scr), lib.hn_stable_value_scratch_bytes(8, 1024) - 1, s), b'scratch')
    # hn_window_loss: n_frames 9 / 1, n_verts 0, n_rays 0, one sdf without the other, NULL, scratch too small
    c = _window_case(8, 40, 40, 'large', False, seed=9)
    d = {k: _dev(v) for k, v in c.items()}
    j9, R9 = torch.zeros(9 * 63, device='cuda'), torch.zeros(9 * 12, device='cuda')
    wscr = torch.zeros(lib.hn_window_loss_scratch_bytes(40, 40), dtype=torch.uint8, device='cuda')
    w7 = (ctypes.c_float * 7)(*WEIGHTS)
    sums, terms = _nan(6), _nan(10)

    def wl(F=4, n_rays=40, sdf_o=True, n_verts=300, color=True, scratch_bytes=None, jp=None):
        jj = P(jp) if jp is not None else P(d['joint_3d'])
        return lib.hn_window_loss(P(d['color']) if color else None, P(d['wsum']), P(d['true_rgb']), P(d['true_mask']), n_rays, P(d['sdf_h']),
                                  P(d['sdf_o']) if sdf_o else None, 40, jj, jj, F, P(R9), P(R9), P(R9), P(R9), P(d['verts']), n_verts, None, 1,
                                  w7, P(wscr), wscr.numel() if scratch_bytes is None else scratch_bytes, P(sums), P(terms), P(j9), P(R9), P(R9), s)
    refused(wl(F=9, jp=j9), b'bad sizes')
    refused(wl(F=1), b'bad sizes')
    refused(wl(n_verts=0), b'bad sizes')
    refused(wl(n_rays=0), b'bad sizes')
    refused(wl(sdf_o=False), b'bad sizes')
    refused(wl(color=False), b'NULL')
    refused(wl(scratch_bytes=wscr.numel() - 1), b'scratch')
    # hn_window_loss_bwd: NULL arguments; sdf gradients without both fields
    gl = torch.ones(1, device='cuda')
    refused(lib.hn_window_loss_bwd(P(d['color']), P(d['wsum']), P(d['true_rgb']), P(d['true_mask']), 40, None, None, 0, P(sums), None, w7, P(j9),
                                   P(R9), P(R9), 4, P(out), P(out), None, None, P(out), P(out), P(out), None, s), b'NULL')
    refused(lib.hn_window_loss_bwd(P(d['color']), P(d['wsum']), P(d['true_rgb']), P(d['true_mask']), 40, P(d['sdf_h']), P(d['sdf_o']), 40, P(sums),
                                   P(gl), w7, P(j9), P(R9), P(R9), 4, P(out), P(out), None, P(out), P(out), P(out), P(out), None, s), b'sdf')
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(sums).all() and torch.isnan(terms).all(), 'a refused call wrote its outputs'
