"""The device VGG19 perceptual loss (hn_vggloss.hip + hn_conv3x3.h through honerf_amd.training.VggLoss) against the torch restatement of
tests/test_vgg_loss_cpu.py on full-width seeded weights and inputs without a marginal gate: loss, the five tap means and
d loss / d color_fine under helpers.assert_parity at 16 x 16, 21 x 21, 18 x 23 and 33 x 16 (all reach the few-row split-K layers; the
last two catch a transposed layout), the gradient's structure, a dead relu1_2, determinism, refusals through the raw ABI, and a
training step with the term added."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import assert_parity, product_modules, record
from test_vgg_loss_cpu import SIZES, evaluate, reference, state_dict, weights

pytestmark = pytest.mark.gpu

_MODEL = {}


def model(variant='plain'):
    from honerf_amd.training import VggLoss
    if variant not in _MODEL:
        _MODEL[variant] = VggLoss(state_dict(weights(variant), 'features.'))
    return _MODEL[variant]


def _bits(x):
    return x.detach().cpu().numpy().tobytes()


def run_patch(m, r, g_loss=None):
    """patch_loss on the device -> (loss, tap means, gradient)."""
    c = r['color'].cuda().requires_grad_(True)
    t = r['true'].cuda().requires_grad_(True)
    loss = m.patch_loss(c, t, r['n0'], r['n1'])
    means = m.last_terms
    if g_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(g_loss, device='cuda'))
    assert t.grad is None
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0 and tuple(means.shape) == (5,) and not means.requires_grad
    assert tuple(c.grad.shape) == tuple(c.shape) and bool(torch.isfinite(c.grad).all())
    return loss.detach(), means, c.grad


def run_nchw(m, r):
    from honerf_amd.training import patch_image
    c = r['color'].cuda().requires_grad_(True)
    loss = m(patch_image(c, r['n0'], r['n1']), patch_image(r['true'].cuda(), r['n0'], r['n1']))
    means = m.last_terms
    loss.backward()
    return loss.detach(), means, c.grad


def check(got, r, what):
    loss, means, grad = got
    assert_parity(loss, r['loss32'], r['loss64'], what + ' loss')
    for k in range(5):
        assert_parity(means[k], r['means32'][k], r['means64'][k], what + ' mean of tap %d' % (k + 1))
    assert_parity(grad, r['grad32'], r['grad64'], what + ' d loss / d color_fine')


@pytest.mark.parametrize('H,W', SIZES)
def test_matches_the_restatement(H, W):
    r, m = reference(H, W), model()
    got = run_patch(m, r)
    check(got, r, '%d x %d patch_loss:' % (H, W))
    again = run_nchw(m, r)
    check(again, r, '%d x %d forward (NCHW):' % (H, W))
    assert [_bits(x) for x in got] == [_bits(x) for x in again]
    assert float(got[0]) > 0.0 and float(got[2].abs().max()) > 0.0
    record('%d x %d loss' % (H, W), float(got[0]), 1.0, kind='value')


def test_gradient_structure():
    r, m = reference(21, 21), model()
    # source == target: exactly 0, both
    same = dict(r, true=r['color'])
    loss, means, grad = run_patch(m, same)
    assert float(loss) == 0.0 and float(means.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0
    # the gradient is linear in the upstream gradient
    _, _, g1 = run_patch(m, r)
    _, _, g25 = run_patch(m, r, g_loss=2.5)
    assert_parity(g25, 2.5 * r['grad32'], 2.5 * r['grad64'], '21 x 21 gradient with g_loss = 2.5 against 2.5 x the restatement')
    assert_parity(g25, 2.5 * g1, 2.5 * g1.double(), '21 x 21 gradient with g_loss = 2.5 against 2.5 x the gradient with 1')


def test_a_dead_relu1_2_leaves_only_the_first_tap():
    r, m = reference(21, 21, 'dead'), model('dead')
    got = run_patch(m, r)
    check(got, r, '21 x 21, dead relu1_2:')
    assert float(got[1][1:].abs().max()) == 0.0 and float(got[1][0]) > 0.0 and float(got[2].abs().max()) > 0.0


def test_repeated_calls_give_the_same_bits():
    m = model()
    first = [_bits(x) for x in run_patch(m, reference(21, 21))]
    assert [_bits(x) for x in run_patch(m, reference(21, 21))] == first
    run_patch(m, reference(33, 16))                              # another size in between
    run_patch(m, reference(16, 16))
    assert [_bits(x) for x in run_patch(m, reference(21, 21))] == first


def test_refusals_return_an_error_and_a_valid_call_still_works():
    from honerf_amd import lib
    r, m = reference(21, 21), model()
    L = lib.load()
    want = run_patch(m, r)
    h = m._model(torch.device('cuda', torch.cuda.current_device()))
    wsb = L.hn_vgg_loss_workspace_bytes
    assert wsb(15, 21) == 0 and wsb(21, 15) == 0 and wsb(0, 0) == 0 and wsb(-3, 21) == 0 and wsb(1 << 16, 1 << 16) == 0 and wsb(1 << 40, 16) == 0
    need = wsb(21, 21)
    assert need >= 2 * 441 * 64 * 4 * 2
    c, t = r['color'].cuda(), r['true'].cuda()
    terms = torch.zeros(6, device='cuda')
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    g = torch.zeros(441, 3, device='cuda')
    one = torch.ones(1, device='cuda')
    P, S = lib.ptr, lib.stream_ptr()
    fwd = lambda *a: L.hn_vgg_loss_fwd(*a, S)
    bwd = lambda *a: L.hn_vgg_loss_bwd(*a, S)
    calls = [fwd(None, P(c), P(t), 21, 21, 3, 63, 1, P(terms), P(ws), need), fwd(h, None, P(t), 21, 21, 3, 63, 1, P(terms), P(ws), need),
             fwd(h, P(c), None, 21, 21, 3, 63, 1, P(terms), P(ws), need), fwd(h, P(c), P(t), 21, 21, 3, 63, 1, None, P(ws), need),
             fwd(h, P(c), P(t), 21, 21, 3, 63, 1, P(terms), None, need),
             fwd(h, P(c), P(t), 21, 21, 3, 63, 1, P(terms), P(ws), need - 1),                     # a workspace one byte short
             fwd(h, P(c), P(t), 15, 21, 3, 45, 1, P(terms), P(ws), need), fwd(h, P(c), P(t), 21, 15, 3, 63, 1, P(terms), P(ws), need),
             fwd(h, P(c), P(t), 21, 21, 0, 63, 1, P(terms), P(ws), need), fwd(h, P(c), P(t), 1 << 16, 1 << 16, 3, 63, 1, P(terms), P(ws), need),
             bwd(None, 21, 21, 3, 63, 1, P(one), P(ws), need, P(g)), bwd(h, 21, 21, 3, 63, 1, None, P(ws), need, P(g)),
             bwd(h, 21, 21, 3, 63, 1, P(one), None, need, P(g)), bwd(h, 21, 21, 3, 63, 1, P(one), P(ws), need, None),
             bwd(h, 21, 21, 3, 63, 1, P(one), P(ws), need - 1, P(g)), bwd(h, 15, 21, 3, 45, 1, P(one), P(ws), need, P(g)),
             bwd(h, 21, 21, 3, -63, 1, P(one), P(ws), need, P(g))]
    assert calls == [-1] * len(calls), calls
    assert L.hn_last_error()
    null13, handle = (ctypes.c_void_p * 13)(), ctypes.c_void_p()
    assert L.hn_vgg_loss_create(null13, null13, ctypes.byref(handle), S) == -1 and L.hn_last_error() and not handle.value
    assert L.hn_vgg_loss_create(None, null13, ctypes.byref(handle), S) == -1 and L.hn_vgg_loss_destroy(None) == 0
    torch.cuda.synchronize()
    assert float(terms.abs().sum()) == 0.0 and int(ws.sum()) == 0 and float(g.abs().sum()) == 0.0          # nothing written
    # a following valid pair of calls gives the right answer
    assert fwd(h, P(c), P(t), 21, 21, 3, 63, 1, P(terms), P(ws), need) == 0 and bwd(h, 21, 21, 3, 63, 1, P(one), P(ws), need, P(g)) == 0
    assert _bits(terms[0]) == _bits(want[0]) and _bits(terms[1:]) == _bits(want[1]) and _bits(g) == _bits(want[2])
    check((terms[0], terms[1:], g), r, 'after the refusals:')


def test_train_step_with_the_term_added():
    """train_step on the object nets with 256 rays as a 16 x 16 patch and extra_loss = vgg_extra_loss(...): the gradient the term sends
    into color_fine against the restatement evaluated on the render's color_fine in float32 and float64 on the host."""
    from honerf_amd import synth, training
    from honerf_amd.renderer import NeuSRenderer
    from oracle import render as orr
    dev = torch.device('cuda:0')
    mods = product_modules(dev)
    ren = NeuSRenderer(mods['sdf_obj'], mods['var_obj'], mods['color_obj'], 'obj', 32, 0, 0, 4, 1.0)
    opt = training.make_optimizer(ren, 5e-4)
    cam = synth.front_camera(dist=1.0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    o, d = orr.rays_from_xy(tt(synth.ndc_grid(16, 16) * 0.5), tt(cam['R'][0]), tt(cam['T'][0]), tt(cam['focal'][0]), tt(cam['principal'][0]))
    true = reference(16, 16)['true']
    t_rand = torch.rand(256, 1, generator=torch.Generator().manual_seed(5))
    weight, rate = 1.0, 0.5
    inner = training.vgg_extra_loss(model(), true.to(dev), weight, rate)
    seen = {}

    def extra(out):
        c = out['color_fine'].clone()                            # the term's own branch: its gradient alone arrives here
        seen['color'] = c.detach().cpu()
        c.register_hook(lambda g: seen.__setitem__('grad', g.detach().cpu()))
        return inner(dict(out, color_fine=c))

    params = training.trainable_parameters(ren)
    before = [p.detach().clone() for p in params]
    terms = training.train_step(ren, opt, o.to(dev), d.to(dev), 0.4, 1.5, None, None, torch.eye(3, device=dev), torch.zeros(3, device=dev), true.to(dev),
                                torch.ones(256, 1, device=dev), 1.0, 1.0, t_rand=t_rand.to(dev), extra_loss=extra)
    assert 'vgg_loss' in terms and float(terms['vgg_loss']) > 0.0 and bool(torch.isfinite(terms['loss']))
    ref = {}
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        ref['loss' + tag], _, g = evaluate(weights(), seen['color'], true, 16, 16, dtype)
        ref['grad' + tag] = rate * weight * g
    assert_parity(terms['vgg_loss'], ref['loss32'], ref['loss64'], 'train_step: vgg_loss on the render')
    assert_parity(seen['grad'], ref['grad32'], ref['grad64'], 'train_step: d (rate weight vgg_loss) / d color_fine')
    for p, b in zip(params, before):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert any(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    changed = sum(int(not torch.equal(p.detach(), b)) for p, b in zip(params, before))
    record('train_step with the VGG term: parameters changed', changed, len(params), kind='value')
