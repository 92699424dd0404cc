"""The VGG19 perceptual loss of training (honerf_amd.training.VggLoss) on the host: the torch restatement
`vgg_loss_reference` against the reference's own VGGLoss through tests/golden/vgg_loss.npz (tests/golden/make_golden_vgg.py: 1/16
width, seeded weights), its convolution against the definition written out, tap shapes, the patch sampler, the state-dict layouts, the
training loop's switch and ramp, and the inputs of tests/test_vgg_loss.py: full-width seeded weights and, per size, the first input
seed without a marginal gate."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import assert_parity, record
from test_lpips_cpu import np_conv3x3_relu

from honerf_amd import training
from honerf_amd.training import (VGG19_CONV_COUT, VGG19_CONV_INDEX, VGG19_POOL_BEFORE, VGG19_TAP_CONVS, VggLoss, patch_image, patch_pixels, vgg19_tensors,
                                 vgg_extra_loss, vgg_loss_reference, vgg_taps_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'vgg_loss.npz')
NARROW = tuple(c // 16 for c in VGG19_CONV_COUT)
CONV_CIN = (3,) + VGG19_CONV_COUT[:-1]
TAP_C = (64, 128, 256, 512, 512)
SIZES = [(16, 16), (21, 21), (18, 23), (33, 16)]             # (H, W) of the image VGG sees: color_fine is [W H, 3] with n0 = W, n1 = H
# the first input seed per size without a marginal gate (test_the_chosen_seeds_have_no_marginal_gate; `first_clean_seed` finds them).
# Scanned on one thread (marginal_units): seeds 0..59 at 16 x 16 hold 1 clean seed, 0..999 at 21 x 21 hold 2 (569, 976), 0..299 at
# 18 x 23 hold 1, 0..1599 at 33 x 16 hold 1.
SEEDS = {(16, 16): 44, (21, 21): 569, (18, 23): 264, (33, 16): 1518}
MARGIN = 16.0


# ---- weights and inputs ----------------------------------------------------------------------------------------------------------------
def make_weights(seed=0):
    """-> (13 conv weights [Cout, Cin, 3, 3], 13 biases), float32: randn sqrt(2 / (9 Cin)), then 0.1 randn, from one generator."""
    g = torch.Generator().manual_seed(seed)
    conv_w = [torch.randn(co, ci, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * ci))) for ci, co in zip(CONV_CIN, VGG19_CONV_COUT)]
    conv_b = [0.1 * torch.randn(co, generator=g) for co in VGG19_CONV_COUT]
    return conv_w, conv_b


_WEIGHTS, _REF = {}, {}


def weights(variant='plain'):
    """The seed-0 weights, made once and never changed; 'dead': the bias of conv index 2 is -1e3 (relu1_2 is zero everywhere, so every
    later tap sees biases alone and only tap 1 carries gradient)."""
    if 'plain' not in _WEIGHTS:
        _WEIGHTS['plain'] = make_weights(0)
    if variant not in _WEIGHTS:
        assert variant == 'dead', variant
        w, b = (list(x) for x in _WEIGHTS['plain'])
        b[1] = torch.full_like(b[1], -1e3)
        _WEIGHTS[variant] = (w, b)
    return _WEIGHTS[variant]


def state_dict(wts, prefix):
    sd = {}
    for i, w, b in zip(VGG19_CONV_INDEX, *wts):
        sd['%s%d.weight' % (prefix, i)], sd['%s%d.bias' % (prefix, i)] = w, b
    return sd


def inputs(H, W, seed):
    """color_fine, true_rgb [W H, 3] float32: uniform in [0, 1]; the target is the source + 0.1 randn, clipped."""
    g = torch.Generator().manual_seed(seed)
    color = torch.rand(H * W, 3, generator=g)
    true = (color + 0.1 * torch.randn(H * W, 3, generator=g)).clamp(0.0, 1.0)
    return color, true


def evaluate(wts, color, true, n0, n1, dtype):
    """The restatement on a patch -> (loss, means [5], d loss / d color_fine), detached, in `dtype`."""
    c = color.detach().to(dtype).clone().requires_grad_(True)
    loss, means = vgg_loss_reference(wts[0], wts[1], patch_image(c, n0, n1), patch_image(true.to(dtype), n0, n1))
    loss.backward()
    return loss.detach(), torch.stack([m.detach() for m in means]), c.grad.detach()


def reference(H, W, variant='plain'):
    """The inputs of a size and the restatement's values in float32 and float64, computed once and shared."""
    key = (H, W, variant)
    if key not in _REF:
        color, true = inputs(H, W, SEEDS[(H, W)])
        r = dict(color=color, true=true, n0=W, n1=H)
        for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
            r['loss' + tag], r['means' + tag], r['grad' + tag] = evaluate(weights(variant), color, true, W, H, dtype)
        _REF[key] = r
    return _REF[key]


def marginal_units(H, W, seed, wts=None):
    """How many gates of the float64 restatement lie within MARGIN e_l of switching, e_l = max |pre32 - pre64| of layer l on the source:
    pre-activations near 0, pool windows whose two largest values nearly tie (the largest positive), tap elements with s nearly t
    (unless both are 0)."""
    wts = wts or weights()
    color, true = inputs(H, W, seed)
    tr = {}
    # on ONE thread: e_l is a measured float32 error and torch's convolution blocks its sums by the thread count, so a unit that sits
    # at the margin counts with one thread count and not with another (21 x 21, seed 569: clean with 1, 4, 8, 16 threads, one
    # pre-activation inside the margin with 2).  Pinned, the count -- and so "the first clean seed" -- is the same wherever this runs.
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
                tr[tag] = {}
                tr['taps' + tag] = vgg_taps_reference(wts[0], wts[1], patch_image(color.to(dtype), W, H), tr[tag])
            taps_t = vgg_taps_reference(wts[0], wts[1], patch_image(true.double(), W, H))
    finally:
        torch.set_num_threads(threads)
    e = [float((a.double() - b).abs().max()) for a, b in zip(tr['32']['pre'], tr['64']['pre'])]
    n_pre = sum(int((p.abs() < MARGIN * e[l]).sum()) for l, p in enumerate(tr['64']['pre']))
    n_pool = 0
    for l, q in zip(VGG19_POOL_BEFORE, tr['64']['pool_in']):
        n, c, hh, ww = q.shape
        win = q[:, :, :hh // 2 * 2, :ww // 2 * 2].reshape(n, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, hh // 2, ww // 2, 4)
        top = win.topk(2, -1).values
        n_pool += int((((top[..., 0] - top[..., 1]) < MARGIN * e[l - 1]) & (top[..., 0] > 0)).sum())
    n_tap = sum(int((((s - t).abs() < MARGIN * e[l]) & ((s != 0) | (t != 0))).sum()) for l, s, t in zip(VGG19_TAP_CONVS, tr['taps64'], taps_t))
    return n_pre, n_pool, n_tap


def first_clean_seed(H, W, limit=2000):
    """The scan that gave SEEDS: seeds from 0 upward, the first without a marginal unit (about 1 s per 20 seeds)."""
    for seed in range(limit):
        if marginal_units(H, W, seed) == (0, 0, 0):
            return seed
    raise AssertionError('no seed below %d without a marginal gate at %d x %d' % (limit, H, W))


# ---- A: the restatement against the reference's VGGLoss ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(GOLDEN))
    state = {k: torch.from_numpy(v) for k, v in g.items() if k.startswith('features.')}
    return g, vgg19_tensors(state, NARROW)


@pytest.mark.parametrize('case', ['21x21', '18x23'])
def test_restatement_reproduces_the_reference(golden, case):
    g, wts = golden
    n0, n1 = (int(v) for v in g[case + '.n0n1'])
    color, true = torch.from_numpy(g[case + '.color_fine']), torch.from_numpy(g[case + '.true_rgb'])
    assert tuple(color.shape) == (n0 * n1, 3)
    loss64, means64, grad64 = evaluate(wts, color, true, n0, n1, torch.float64)
    for what, got, want in (('loss', loss64, g[case + '.loss64']), ('tap means', means64, g[case + '.means64']), ('gradient', grad64, g[case + '.grad64'])):
        e = float(np.abs(got.numpy() - want).max() / np.abs(want).max())
        record('%s float64 restatement against the reference, %s' % (case, what), e, 1e-12)
        assert e <= 1e-12, (what, e)
    loss32, means32, grad32 = evaluate(wts, color, true, n0, n1, torch.float32)
    assert grad32.dtype == torch.float32
    assert_parity(loss32, g[case + '.loss32'], g[case + '.loss64'], case + ' float32 restatement against the reference, loss')
    assert_parity(means32, g[case + '.means32'], g[case + '.means64'], case + ' float32 restatement against the reference, tap means')
    assert_parity(grad32, g[case + '.grad32'], g[case + '.grad64'], case + ' float32 restatement against the reference, gradient')
    # a transposed layout is another image: the same data read with n0 and n1 swapped gives another loss where they differ
    if n0 != n1:
        other = evaluate(wts, color, true, n1, n0, torch.float64)[0]
        assert abs(float(other) - float(g[case + '.loss64'])) > 1e-6
    # the target carries no gradient, and VggLoss on CPU tensors is the restatement
    t = true.double().requires_grad_(True)
    loss, _ = vgg_loss_reference(wts[0], wts[1], patch_image(color.double().requires_grad_(True), n0, n1), patch_image(t, n0, n1))
    loss.backward()
    assert t.grad is None


# ---- B, C: the convolution and the tap shapes ----------------------------------------------------------------------------------------------
def test_convolution_against_the_definition():
    wts = weights()
    color, _ = inputs(16, 16, 3)
    x = patch_image(color.double(), 16, 16)
    got = vgg_taps_reference(wts[0], wts[1], x)[0].numpy()
    want = np_conv3x3_relu(x.numpy(), wts[0][0].double().numpy(), wts[1][0].double().numpy())
    assert got.shape == want.shape == (1, 64, 16, 16)
    e = float(np.abs(got - want).max() / np.abs(want).max())
    record('restatement, relu1_1, against the written-out convolution', e, 1e-13)
    assert e <= 1e-13, e
    assert float((want > 0).mean()) > 0.2


@pytest.mark.parametrize('H,W', SIZES)
def test_tap_shapes_floor_at_every_pool(H, W):
    wts = weights()
    color, _ = inputs(H, W, 0)
    with torch.no_grad():
        taps = vgg_taps_reference(wts[0], wts[1], patch_image(color, W, H))
    assert [tuple(t.shape) for t in taps] == [(1, c, H >> k, W >> k) for k, c in enumerate(TAP_C)]
    if (H, W) == (33, 16):
        assert [tuple(t.shape[2:]) for t in taps] == [(33, 16), (16, 8), (8, 4), (4, 2), (2, 1)]


# ---- D: the patch sampler ------------------------------------------------------------------------------------------------------------------
def _mask(H, W, r_lo, r_hi, c_lo, c_hi, seed=0):
    m = np.zeros((H, W), dtype=np.uint8)
    r = np.random.RandomState(seed)
    m[r_lo:r_hi + 1, c_lo:c_hi + 1] = r.rand(r_hi - r_lo + 1, c_hi - c_lo + 1) > 0.3
    m[r_lo, c_lo] = m[r_hi, c_hi] = 1
    return m


@pytest.mark.parametrize('what,box', [('taller and wider than c', (20, 70, 30, 100)), ('shorter than c', (40, 52, 60, 66)),
                                      ('touching the top-left border', (0, 9, 0, 30)), ('touching the bottom-right border', (85, 95, 110, 127))])
def test_patch_pixels(what, box):
    H, W, n_rays = 96, 128, 450                                  # isqrt(450) = 21, as the confs' 441
    c = 21
    mask = _mask(H, W, *box)
    image = np.random.RandomState(1).rand(H, W, 3).astype(np.float32)
    r_lo, r_hi, c_lo, c_hi = box
    seen_r, seen_c = set(), set()
    for draw in range(40):
        rays_xy, rows, cols, flat = patch_pixels(mask, n_rays, np.random.default_rng(draw))
        assert rays_xy.shape == (c * c, 2) and rays_xy.dtype == np.float32 and rows.shape == cols.shape == flat.shape == (c * c,)
        r0, c0 = int(rows.min()), int(cols.min())
        # c x c, contiguous, inside the image; flat order: rows vary fastest
        p = np.arange(c * c)
        assert (rows == r0 + p % c).all() and (cols == c0 + p // c).all() and (flat == rows * W + cols).all()
        assert 0 <= r0 and r0 + c <= H and 0 <= c0 and c0 + c <= W
        # the exclusive end within [min(lo + c, hi), max(lo + c, hi)]; only where that interval reaches outside [c, size] may the window
        # instead sit at the border it was shifted to
        for end, lo, hi, size in ((r0 + c, r_lo, r_hi, H), (c0 + c, c_lo, c_hi, W)):
            st, ed = min(lo + c, hi), max(lo + c, hi)
            assert st <= end <= ed or (st < c and end == c) or (ed > size and end == size), (what, end, lo, hi)
        seen_r.add(r0)
        seen_c.add(c0)
        assert np.allclose(rays_xy[:, 0], -(cols - W / 2.0) / (H / 2.0)) and np.allclose(rays_xy[:, 1], -(rows - H / 2.0) / (H / 2.0))
        # the reference's reshape / permute of the gathered colours is the crop, upright
        crop = patch_image(torch.from_numpy(image.reshape(-1, 3)[flat]), c, c)[0]
        assert torch.equal(crop, torch.from_numpy(image[r0:r0 + c, c0:c0 + c]).permute(2, 0, 1))
    # the draw is used: every end of the interval that lies inside the image is reachable, so 40 draws see more than one start
    for seen, lo, hi, size in ((seen_r, r_lo, r_hi, H), (seen_c, c_lo, c_hi, W)):
        reachable = len(set(min(max(e - c, 0), size - c) for e in range(min(lo + c, hi), max(lo + c, hi) + 1)))
        assert len(seen) > 1 or reachable == 1, (what, seen)
    with pytest.raises(ValueError):
        patch_pixels(np.zeros((H, W)), n_rays, np.random.default_rng(0))
    with pytest.raises(ValueError):
        patch_pixels(mask[:20], n_rays, np.random.default_rng(0))


# ---- E: the state-dict layouts -------------------------------------------------------------------------------------------------------------
def test_the_key_layouts_load_to_the_same_tensors():
    wts = weights()
    for prefix in ('features.', ''):
        sd = state_dict(wts, prefix)
        sd.update({prefix + '30.weight': torch.zeros(512, 512, 3, 3), prefix + '32.bias': torch.zeros(7), 'classifier.0.weight': torch.zeros(2, 2),
                   prefix + '1.weight': torch.zeros(3)})
        got = vgg19_tensors(sd)
        assert [len(x) for x in got] == [13, 13]
        for x, y in zip(got[0] + got[1], wts[0] + wts[1]):
            assert torch.equal(torch.as_tensor(x), y)
    got = vgg19_tensors({k: v.numpy() for k, v in state_dict(wts, '').items()})
    assert torch.equal(got[0][4], wts[0][4]) and torch.equal(got[1][12], wts[1][12])
    assert VggLoss(state_dict(wts, 'features.')).conv_weight[3] is wts[0][3]             # made without touching a device


def test_missing_and_misshaped_keys_are_named():
    sd = state_dict(weights(), 'features.')
    short = {k: v for k, v in sd.items() if k not in ('features.7.weight', 'features.28.bias')}
    with pytest.raises(ValueError) as e:
        VggLoss(short)
    assert 'features.7.weight' in str(e.value) and 'features.28.bias' in str(e.value) and 'features.5.weight' not in str(e.value)
    wrong = dict(sd)
    wrong['features.16.weight'] = torch.zeros(512, 256, 3, 3)       # VGG16's shape at that place
    wrong['features.0.bias'] = torch.zeros(63)
    with pytest.raises(ValueError) as e:
        vgg19_tensors(wrong)
    assert 'features.16.weight' in str(e.value) and 'features.0.bias' in str(e.value)


def test_the_c_abi_declares_the_vgg_loss():
    import re
    from honerf_amd import lib
    with open(os.path.join(ROOT, 'include', 'honerf.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name, n_args in (('hn_vgg_loss_create', 4), ('hn_vgg_loss_destroy', 1), ('hn_vgg_loss_workspace_bytes', 2), ('hn_vgg_loss_fwd', 12), ('hn_vgg_loss_bwd', 11)):
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, src)
        assert m, name + ' is not declared in include/honerf.h'
        assert len(m.group(1).split(',')) == n_args, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args, name
    assert lib.SIGNATURES['hn_vgg_loss_workspace_bytes'][0] is lib.c_sz


# ---- VggLoss on the host: the restatement, refusals ----------------------------------------------------------------------------------------
def test_host_tensors_take_the_restatement_and_small_or_odd_inputs_are_refused():
    vgg = VggLoss(state_dict(weights(), ''))
    r = reference(16, 16)
    c = r['color'].double().requires_grad_(True)
    t = r['true'].double().requires_grad_(True)
    loss = vgg.patch_loss(c, t)
    loss.backward()
    assert loss.dtype == torch.float64 and float(loss.detach()) == float(r['loss64']) and torch.equal(c.grad, r['grad64']) and t.grad is None
    assert torch.equal(vgg.last_terms, r['means64']) and not vgg.last_terms.requires_grad
    same = vgg(patch_image(r['color'].double(), 16, 16), patch_image(r['true'].double(), 16, 16))
    assert float(same) == float(loss.detach())
    extra = vgg_extra_loss(vgg, r['true'], weight=2.0, rate=0.25)
    out = extra({'color_fine': r['color']})
    assert sorted(out) == ['loss', 'vgg_loss'] and abs(float(out['loss']) - 0.5 * float(out['vgg_loss'])) < 1e-7
    assert abs(float(out['vgg_loss']) - float(r['loss32'])) < 1e-6 and (extra.weight, extra.rate) == (2.0, 0.25)
    with pytest.raises(ValueError, match='16 x 16'):
        vgg.patch_loss(torch.zeros(15 * 21, 3), torch.zeros(15 * 21, 3), 15, 21)
    with pytest.raises(ValueError, match='16 x 16'):
        vgg(torch.zeros(1, 3, 21, 15), torch.zeros(1, 3, 21, 15))
    with pytest.raises(ValueError, match='square'):
        vgg.patch_loss(torch.zeros(18 * 23, 3), torch.zeros(18 * 23, 3))
    with pytest.raises(ValueError):
        vgg.patch_loss(torch.zeros(18 * 23, 3), torch.zeros(18 * 23, 3), 18, 22)
    with pytest.raises(ValueError):
        vgg(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))


# ---- F: the training loop ------------------------------------------------------------------------------------------------------------------
def _run_train(tmp_path, name, **kw):
    from honerf_amd.nets import RenderingNetwork_OBJ, SDFNetwork_OBJ, SingleVarianceNetwork

    class R:
        pass
    r = R()
    r.sdf_network, r.color_network, r.deviation_network = SDFNetwork_OBJ(), RenderingNetwork_OBJ(), SingleVarianceNetwork(0.3)
    log = []

    def fake_step(renderer, optimizer, rays_o, rays_d, near, far, bt_inv, T_pose_21, Ro, To, true_rgb, true_mask, igr_weight, mask_weight, extra_loss=None,
                  dist=None):
        log.append((len(log), rays_o, true_rgb, None if extra_loss is None else (extra_loss.weight, extra_loss.rate, extra_loss.vgg),
                    optimizer.param_groups[0]['lr']))
        terms = {'loss': torch.tensor(1.0)}
        if extra_loss is not None:
            terms['vgg_loss'] = torch.tensor(0.125)
        return terms

    patch = dict(rays_o='patch rays', rays_d=None, true_rgb='patch rgb', true_mask=None, Ro=None, To=None)
    batch = dict(rays_o='random rays', rays_d=None, true_rgb='random rgb', true_mask=None, Ro=None, To=None, patch=patch)
    n = training.train(r, [batch], 13, str(tmp_path / name), learning_rate=1e-3, warm_up_end=4, save_freq=100, report_freq=1, step_fn=fake_step, **kw)
    assert n == 13
    return log, [json.loads(x) for x in open(tmp_path / name / 'metrics.jsonl')]


def test_train_switches_to_the_patch_and_ramps_the_term(tmp_path):
    vgg = VggLoss(state_dict(weights(), 'features.'))
    log, lines = _run_train(tmp_path, 'vgg', vgg=vgg, vgg_weight=0.5, vgg_start=4, vgg_ramp=4)
    # iter_step <= vgg_start: the random sample, no term; from vgg_start + 1 on: the batch's 'patch' entry and the ramp
    for i in range(5):
        assert log[i][1:4] == ('random rays', 'random rgb', None)
    want = {5: 0.25, 6: 0.5, 8: 1.0, 12: 1.0}                    # vgg_start + 1, + vgg_ramp / 2, + vgg_ramp, + 2 vgg_ramp
    for i in range(5, 13):
        assert log[i][1:3] == ('patch rays', 'patch rgb') and log[i][3][0] == 0.5 and log[i][3][2] is vgg
        assert log[i][3][1] == min((i - 4) / 4.0, 1.0)
    assert all(log[i][3][1] == v for i, v in want.items())
    assert ['vgg_loss' in x for x in lines] == [False] * 5 + [True] * 8 and lines[5]['vgg_loss'] == 0.125
    # the default start: 0.3 end_iter = 3.9 -> from iteration 4 on; the default ramp of 10000
    log, _ = _run_train(tmp_path, 'default', vgg=vgg)
    assert [x[3] is None for x in log] == [True] * 4 + [False] * 9
    assert log[4][3][:2] == (1.0, (4 - 0.3 * 13) / 10000.0)
    # a batch without a 'patch' entry is used as it is; weight 0 adds no term but still switches (exp_runner.py:140-143, :228)
    log, _ = _run_train(tmp_path, 'weightless', vgg=vgg, vgg_weight=0.0, vgg_start=4)
    assert [x[1] for x in log] == ['random rays'] * 5 + ['patch rays'] * 8 and all(x[3] is None for x in log)


def test_train_without_vgg_is_unchanged(tmp_path):
    plain, lines_plain = _run_train(tmp_path, 'plain')
    explicit, lines_explicit = _run_train(tmp_path, 'explicit', vgg=None, vgg_weight=3.0, vgg_start=2, vgg_ramp=5)
    assert plain == explicit and lines_plain == lines_explicit
    assert all(x[1:4] == ('random rays', 'random rgb', None) for x in plain)


# ---- G: the inputs of the device test ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', SIZES)
def test_the_chosen_seeds_have_no_marginal_gate(H, W):
    assert marginal_units(H, W, SEEDS[(H, W)]) == (0, 0, 0)
    r = reference(H, W)
    gmax = float(r['grad64'].abs().max())
    e = float((r['grad32'].double() - r['grad64']).abs().max()) / gmax
    record('%d x %d float32 restatement against float64, gradient (relative to its largest value)' % (H, W), e, 5e-6)
    record('%d x %d loss' % (H, W), float(r['loss64']), 1.0, kind='value')
    # away from every gate float32 and float64 agree to rounding: far inside the 1e-4 the device path is held to
    assert e <= 5e-6 and gmax > 1e-4 and 0.01 < float(r['loss64']) < 10.0
    assert float(r['means64'].min()) > 0.0


def test_the_dead_variant_leaves_only_the_first_tap():
    r, plain = reference(21, 21, 'dead'), reference(21, 21)
    assert r['means64'][1:].abs().max() == 0.0 and float(r['means64'][0]) == float(plain['means64'][0])
    assert bool(torch.isfinite(r['grad32']).all()) and float(r['grad64'].abs().max()) > 0.0
    assert weights('plain')[1][1].min() > -1.0                   # the shared weights are untouched
