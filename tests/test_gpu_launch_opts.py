"""The options of one library call do not outlive it (every field launch takes its FieldLaunchOpts as an argument).
On ONE host thread a plain hn_field_eval / hn_field_eval_bwd of a hand field must return the same bits before and after calls that
launch the same kernels over a compact list (device-side count, permutation), with the per-sample direction form of the object
adjoint, inside a render that keeps a tape, and in live-first order: a count, a permutation or a flag left behind by one of them
would change what the next dense launch computes.  160 points = one full 128-sample tile + a 32-sample tail."""
import numpy as np
import pytest
import torch

from honerf_amd import lib as L, synth
from helpers import cu, product_modules, t

pytestmark = pytest.mark.gpu

CUTOFF = torch.tensor([0.08, 0.03, 0.03, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02,
                       0.02, 0.02])
BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)
NEAR, FAR = 0.4, 1.5


def is_far(pts):
    """The ordering pass's classification: far only if 200 (v_b - cutoff_b) > 17 for every bone."""
    q = torch.einsum('bij,nj->nbi', t(BT_INV)[:, :3, :3], pts) + t(BT_INV)[:, :3, 3] - t(T_POSE)
    return (200.0 * (q.norm(dim=-1) - CUTOFF) > 17.0).all(-1)


def rays_through(points):
    """Rays of a camera at the origin looking along +z through the given world points (d = the unit vector to the point, the
    origin one unit in front of the camera plane's crossing, as tests/test_gpu_live_first_order.py)."""
    p = torch.as_tensor(np.asarray(points), dtype=torch.float32)
    p1 = torch.cat([p[:, :2] / p[:, 2:3], torch.ones(len(p), 1)], dim=-1)
    d = torch.nn.functional.normalize(p1, dim=-1)
    return (p1 - d).contiguous(), d.contiguous()


def adjoint(hand, pts, dirs, spr, gs, gg, gr):
    """hn_field_eval_bwd of the hand field: d / d pts, d / d rays_d, d / d bt_inv, d / d T_pose."""
    lib = L.load()
    n = pts.shape[0]
    out = [torch.empty(n, 3, device='cuda'), torch.empty(n // spr, 3, device='cuda'), torch.zeros(1, 21, 4, 4, device='cuda'),
           torch.zeros(1, 21, 3, device='cuda')]
    need = lib.hn_field_bwd_workspace_bytes(hand.handle, n)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    L.check(lib.hn_field_eval_bwd(hand.handle, L.ptr(cu(pts)), L.ptr(cu(dirs)), n, spr, L.ptr(cu(t(BT_INV)[None])), L.ptr(cu(t(T_POSE)[None])), 1, n,
                                  L.ptr(cu(gs)), L.ptr(cu(gg)), L.ptr(cu(gr)), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), L.ptr(ws), need,
                                  L.stream_ptr()), 'hn_field_eval_bwd')
    torch.cuda.synchronize()
    return out


def test_options_of_one_call_do_not_reach_the_next(monkeypatch):
    """(a) hn_field_eval on 160 points, half of them around joint 9 and half of them far from every bone, alternating; (e) hn_field_eval_bwd on
    the same points; (b) one differentiable two-field render and its backward at 32 rays x 128 samples, one frame -- 4096 samples, the
    smallest size at which the hand's samples are compacted --; (c) one NeuSRenderer.render with HONERF_LIVE_FIRST=2 at 12 rays x 32
    samples; then (a) and (e) again: torch.equal for the four outputs and the four gradients.  (The pose gradients of a one-frame launch of
    two tiles are summed per tile in a fixed order, not with atomics -- tests/test_gpu_parity.py::
    test_hand_pose_gradients_are_additive_over_launch_shapes asks two runs for the same bits --, so no gradient needs a tolerance.)"""
    from honerf_amd.renderer import NeuSRenderer, NeuSRenderer_fitting
    dev = torch.device('cuda')
    m = product_modules()
    dual = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 32, 0, 4, 1.0)
    dual.precision = 'f16x3'
    dual.compact_far_field = True
    hand, obj = dual.fields()
    assert hand.compaction and hand.precision == 'f16x3' and obj.precision == 'f16x3'

    g = torch.Generator().manual_seed(31)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    around = t(JOINTS[9]) + unit(80) * (0.01 + 0.02 * torch.rand(80, 1, generator=g))
    away = t(JOINTS[9]) + 0.6 * unit(80)
    pts = torch.stack([around, away], dim=1).reshape(160, 3).contiguous()
    assert is_far(pts).reshape(80, 2).tolist() == [[False, True]] * 80
    spr = 4
    dirs = unit(160 // spr)
    gs, gg, gr = torch.randn(160, 1, generator=g), torch.randn(160, 3, generator=g), torch.randn(160, 3, generator=g)
    bt, tp = cu(t(BT_INV)), cu(t(T_POSE))

    def evaluate():
        out = hand.evaluate(pts.to(dev), dirs.to(dev), spr, bt, tp, want_feat=True)
        torch.cuda.synchronize()
        return [x.clone() for x in out]

    grads_before = adjoint(hand, pts, dirs, spr, gs, gg, gr)                                        # (e), first time
    A = evaluate()                                                                                  # (a)
    assert all(bool(torch.isfinite(x).all()) for x in A + grads_before)

    # (b) compact list + permutation in the forward and the backward pass, per-sample directions in the object adjoint, a tape
    through = JOINTS[torch.randint(0, 21, (32,), generator=g).numpy()] + (0.03 * torch.randn(32, 3, generator=g)).numpy().astype(np.float32)
    o, d = rays_through(through)
    R_obj, _ = synth.synth_obj_pose(10)
    leaves = [cu(x).clone().requires_grad_(True) for x in (t(BT_INV), t(R_obj).T.contiguous(), t(JOINTS).mean(0) + torch.tensor([0.02, 0.0, 0.03]))]
    out = dual.render(cu(o), cu(d), NEAR, FAR, leaves[0], tp, None, leaves[1], leaves[2], t_rand=cu(torch.rand(32, 1, generator=g)))
    assert out['sdf_hand'].numel() == 4096
    sh = out['sdf_hand'].detach().reshape(-1)
    far_share = float((sh == sh.mode().values).float().mean())
    assert 0.05 < far_share < 0.95, far_share                      # the compact list is shorter than the dense one, and not empty
    loss = sum((out[k] * torch.randn(out[k].shape, generator=g).to(dev)).sum() for k in ('color_fine', 'weight_sum', 'sdf_hand', 'sdf_obj', 'gradient_hand'))
    for x in torch.autograd.grad(loss, leaves):
        assert bool(torch.isfinite(x).all())

    # (c) the live-first order at a size it is not the default for
    single = NeuSRenderer(m['sdf_hand'], m['var_hand'], m['color_hand'], 'hand', 32, 0, 0, 4, 1.0)
    single.precision = 'f16x3'
    monkeypatch.setenv('HONERF_LIVE_FIRST', '2')
    with torch.no_grad():
        got = single.render(cu(o[:12]), cu(d[:12]), NEAR, FAR, bt, tp, None, None, None, 0, t_rand=cu(torch.rand(12, 1, generator=g)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got['color_fine']).all())
    monkeypatch.delenv('HONERF_LIVE_FIRST')

    for name, a, b in zip(('sdf', 'gradient', 'rgb', 'feature vector'), A, evaluate()):              # (d)
        assert torch.equal(a, b), 'hn_field_eval: %s changed after a compacted render and a live-first render' % name
    for name, a, b in zip(('pts', 'rays_d', 'bt_inv', 'T_pose'), grads_before, adjoint(hand, pts, dirs, spr, gs, gg, gr)):   # (e), second time
        assert torch.equal(a, b), 'hn_field_eval_bwd: d / d %s changed after a compacted render and a live-first render' % name
