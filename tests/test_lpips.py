"""The device LPIPS (hn_lpips.hip + hn_conv3x3.h through honerf_amd.image_metrics.LpipsVgg) against the torch restatement of tests/test_lpips_cpu.py
on seeded random weights: every element of every tap, every tap mean and every total under helpers.assert_parity (1e-4 of the
largest float32 reference value; where the float32 reference is itself further from float64, no further from float64 than 1.5 x
the reference); a dead first tap and a first tap beyond f16's range; exact zeros and symmetry; the same bits on a repeated call,
for every position in a batch, every split of it and every input form; refusals; and tools/image_eval.py --lpips-weights on a tree of
files."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_parity, record
from test_image_metrics_cpu import image_pairs
from test_lpips_cpu import SIZES, TAP_C, ref_features, ref_layers_of, ref_lpips, state_dicts, weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


_MODEL, _REF = {}, {}


def model(variant='plain'):
    from honerf_amd.image_metrics import LpipsVgg
    if variant not in _MODEL:
        _MODEL[variant] = LpipsVgg(*state_dicts(weights(variant), 'features.'))
    return _MODEL[variant]


def reference(H, W, variant='plain'):
    """The scene and the restatement's values of it in float32 and float64, computed once per size and weight variant."""
    key = (H, W, variant)
    if key not in _REF:
        a, b = image_pairs(H, W)
        wts = weights(variant)
        r = dict(a=a, b=b)
        for name, dtype in (('32', torch.float32), ('64', torch.float64)):
            ta, tb = ref_features(a, wts, dtype), ref_features(b, wts, dtype)
            layers = ref_layers_of(ta, tb, wts)
            r['taps_a' + name], r['taps_b' + name], r['layers' + name], r['lpips' + name] = ta, tb, layers, ref_lpips(layers)
        _REF[key] = r
    return _REF[key]


def check_against(ref, m, what):
    a, b = ref['a'], ref['b']
    F, H, W = a.shape[:3]
    for side, img in (('a', a), ('b', b)):
        taps = m.features(img)
        assert len(taps) == 5
        for k, t in enumerate(taps):
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (F, TAP_C[k], H >> k, W >> k)
            assert bool(torch.isfinite(t).all())
            assert_parity(t, ref['taps_%s32' % side][k], ref['taps_%s64' % side][k], '%s tap %d of %s, every element' % (what, k + 1, side))
    layers = m.lpips_layers(a, b)
    assert layers.is_cuda and layers.dtype == torch.float64 and tuple(layers.shape) == (F, 5) and bool(torch.isfinite(layers).all())
    for k in range(5):
        for f in range(F):
            assert_parity(layers[f, k], ref['layers32'][f, k], ref['layers64'][f, k], '%s mean of tap %d, pair %d' % (what, k + 1, f))
    total = m.lpips(a, b)
    assert total.is_cuda and total.dtype == torch.float64 and tuple(total.shape) == (F,)
    for f in range(F):
        assert_parity(total[f], ref['lpips32'][f], ref['lpips64'][f], '%s lpips, pair %d' % (what, f))
    s = layers[:, 0]
    for k in range(1, 5):
        s = s + layers[:, k]
    assert _np(total).tobytes() == _np(s).tobytes()                              # the sum of the five means, in order
    return taps, layers, total


@pytest.mark.parametrize('H,W', SIZES)
def test_matches_the_restatement(H, W):
    ref = reference(H, W)
    _, layers, total = check_against(ref, model(), '%d x %d' % (H, W))
    assert float(total.min()) > 0.0
    m = model()
    # identical images: exactly 0; swapped images: the same bits
    assert _np(m.lpips(ref['a'], ref['a'])).tolist() == [0.0] * 3 and _np(m.lpips_layers(ref['b'], ref['b'])).tolist() == [[0.0] * 5] * 3
    assert _np(m.lpips_layers(ref['b'], ref['a'])).tobytes() == _np(layers).tobytes()


def test_a_dead_tap_is_exactly_zero_and_nothing_is_nan():
    ref = reference(17, 31, 'dead')
    assert float(ref['taps_a32'][0].abs().max()) == 0.0 and float(ref['taps_a32'][1].abs().max()) > 0.0
    taps, layers, total = check_against(ref, model('dead'), '17 x 31, dead first tap:')
    assert float(taps[0].abs().max()) == 0.0
    assert _np(layers[:, 0]).tolist() == [0.0] * 3 and not bool(torch.isnan(layers).any()) and not bool(torch.isnan(total).any())


def test_a_tap_beyond_f16_range_stays_finite_and_within_the_bounds():
    ref = reference(17, 31, 'range')
    assert float(ref['taps_a32'][0].max()) > 1e5
    taps, _, total = check_against(ref, model('range'), '17 x 31, first layer x 2^15:')
    assert float(taps[0].max()) > 1e5 and bool(torch.isfinite(total).all())


@pytest.mark.parametrize('H,W', [(37, 41), (16, 130)])
def test_input_forms_splits_and_repeated_calls_give_the_same_bits(H, W, monkeypatch):
    from honerf_amd import image_metrics as im
    ref = reference(H, W)
    a, b = ref['a'], ref['b']
    m = model()
    run = lambda x, y: (_np(m.lpips(x, y)).tobytes(), _np(m.lpips_layers(x, y)).tobytes())
    first = run(a, b)
    assert run(a, b) == first                                                   # a repeated call
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert run(ta, tb) == first and run(ta.cuda(), tb.cuda()) == first and run(a, tb.cuda()) == first
    feats = [_np(t).tobytes() for t in m.features(a)]
    assert [_np(t).tobytes() for t in m.features(ta.cuda())] == feats
    # image 1 of the batch alone, and as [H, W, 3]
    alone, flat = run(ta.cuda()[1:2], tb.cuda()[1:2]), run(a[1], b[1])
    for x, y, z in zip(first, alone, flat):
        per = len(x) // 3
        assert y == x[per:2 * per] and z == y
    assert m.lpips(a[1], b[1]).dim() == 0 and tuple(m.lpips_layers(a[1], b[1]).shape) == (5,)
    one = m.features(a[1])
    assert [tuple(t.shape) for t in one] == [(TAP_C[k], H >> k, W >> k) for k in range(5)]
    assert all(_np(t).tobytes() == _np(u[1]).tobytes() for t, u in zip(one, m.features(a)))
    # a forced split: one pair per device call
    monkeypatch.setattr(im, 'LPIPS_WORKSPACE_LIMIT', 0)
    assert m._per_call(3, H, W, 'test')[0] == 1
    assert run(a, b) == first and [_np(t).tobytes() for t in m.features(a)] == feats
    monkeypatch.undo()
    assert m._per_call(3, H, W, 'test')[0] == 3
    # non-contiguous input (a channel flip, as a BGR reader would hand over) is the image it shows
    flipped = (np.ascontiguousarray(a[..., ::-1]), np.ascontiguousarray(b[..., ::-1]))
    assert run(a[..., ::-1], b[..., ::-1]) == run(*flipped)
    planar = lambda t: t.cuda().flip(-1).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)        # [F, H, W, 3] strides of a planar image
    assert not planar(ta).is_contiguous() and run(planar(ta), planar(tb)) == run(*flipped) and run(*flipped) != first
    # the summary
    both = im.image_metrics(a, b, lpips=m)
    plain = im.image_metrics(a, b)
    assert sorted(plain) == ['psnr', 'psnr_mean', 'ssim', 'ssim_mean'] and sorted(both) == ['lpips', 'lpips_mean', 'psnr', 'psnr_mean', 'ssim', 'ssim_mean']
    assert both['lpips'].dtype == np.float64 and both['lpips'].tobytes() == first[0] and both['lpips_mean'] == float(both['lpips'].mean())
    assert both['psnr'].tobytes() == plain['psnr'].tobytes() and both['ssim'].tobytes() == plain['ssim'].tobytes()
    single = im.image_metrics(a[1], b[1], lpips=m)
    assert np.ndim(single['lpips']) == 0 and single['lpips_mean'] == float(single['lpips'])


def test_refusals_raise_and_a_valid_call_still_works():
    from honerf_amd import image_metrics as im, lib
    ref = reference(17, 31)
    a, b = ref['a'], ref['b']
    m = model()
    small_a, small_b = image_pairs(15, 40)
    for fn in (m.lpips, m.lpips_layers, lambda x, y: im.image_metrics(x, y, lpips=m)):
        with pytest.raises(ValueError, match='16 x 16'):
            fn(small_a, small_b)                                                # 15 x 40
        with pytest.raises(ValueError, match='16 x 16'):
            fn(a[:, :, :15], b[:, :, :15])
        with pytest.raises(ValueError):
            fn(a.astype(np.float32), b)                                         # wrong dtype
        with pytest.raises(ValueError):
            fn(a, torch.from_numpy(b).double())
        with pytest.raises(ValueError):
            fn(a, b[:2])                                                        # mismatched shapes
        with pytest.raises(ValueError):
            fn(a, b[:, :, :30])
        with pytest.raises(ValueError):
            fn(a[0], b)
    with pytest.raises(ValueError, match='16 x 16'):
        m.features(small_a)
    with pytest.raises(ValueError):
        m.features(a.astype(np.float32))
    with pytest.raises(ValueError, match='LpipsVgg'):
        im.image_metrics(a, b, lpips='vgg')
    # the library itself: status codes with a message, before anything is launched
    L = lib.load()
    wsb = L.hn_lpips_workspace_bytes
    assert wsb(0, 17, 31) == 0 and wsb(3, 15, 31) == 0 and wsb(3, 17, 15) == 0 and wsb(-1, 17, 31) == 0
    assert wsb(1 << 10, 1 << 10, 1 << 10) == 0 and wsb(1, 1 << 16, 1 << 16) == 0 and wsb(1 << 40, 16, 16) == 0
    need = wsb(3, 17, 31)
    assert need >= 6 * 17 * 31 * (64 + 32 + 64) * 4
    x, y = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.zeros(3, 5, dtype=torch.float64, device='cuda')
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    taps = [torch.zeros(3, c, 17 >> k, 31 >> k, dtype=torch.float32, device='cuda') for k, c in enumerate(TAP_C)]
    P, S, h = lib.ptr, lib.stream_ptr(), m._handle
    T = [P(t) for t in taps]
    calls = [L.hn_lpips(None, P(x), P(y), 3, 17, 31, P(out), P(ws), need, S), L.hn_lpips(h, None, P(y), 3, 17, 31, P(out), P(ws), need, S),
             L.hn_lpips(h, P(x), None, 3, 17, 31, P(out), P(ws), need, S), L.hn_lpips(h, P(x), P(y), 3, 17, 31, None, P(ws), need, S),
             L.hn_lpips(h, P(x), P(y), 3, 17, 31, P(out), None, need, S),
             L.hn_lpips(h, P(x), P(y), 3, 17, 31, P(out), P(ws), need - 1, S),                    # a workspace that is too small
             L.hn_lpips(h, P(x), P(y), 3, 15, 31, P(out), P(ws), need, S), L.hn_lpips(h, P(x), P(y), 3, 17, 15, P(out), P(ws), need, S),
             L.hn_lpips(h, P(x), P(y), 0, 17, 31, P(out), P(ws), need, S), L.hn_lpips(h, P(x), P(y), 1 << 10, 1 << 10, 1 << 10, P(out), P(ws), need, S),
             L.hn_lpips_features(None, P(x), 3, 17, 31, *T, P(ws), need, S), L.hn_lpips_features(h, None, 3, 17, 31, *T, P(ws), need, S),
             L.hn_lpips_features(h, P(x), 3, 17, 31, T[0], T[1], None, T[3], T[4], P(ws), need, S),
             L.hn_lpips_features(h, P(x), 3, 17, 31, *T, None, need, S), L.hn_lpips_features(h, P(x), 3, 17, 31, *T, P(ws), 64, S),
             L.hn_lpips_features(h, P(x), 3, 15, 31, *T, P(ws), need, S), L.hn_lpips_features(h, P(x), 0, 17, 31, *T, P(ws), need, S)]
    assert calls == [-1] * len(calls), calls
    assert L.hn_last_error()
    null13, null5, handle = (ctypes.c_void_p * 13)(), (ctypes.c_void_p * 5)(), ctypes.c_void_p()
    assert L.hn_lpips_create(null13, null13, null5, ctypes.byref(handle), S) == -1 and L.hn_last_error() and not handle.value
    assert L.hn_lpips_create(None, null13, null5, ctypes.byref(handle), S) == -1 and L.hn_lpips_destroy(None) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and int(ws.sum()) == 0 and all(float(t.abs().sum()) == 0.0 for t in taps)      # nothing written
    # a following valid call still gives the right answer
    assert L.hn_lpips(h, P(x), P(y), 3, 17, 31, P(out), P(ws), need, S) == 0
    assert _np(out).tobytes() == _np(m.lpips_layers(a, b)).tobytes()
    for f in range(3):
        assert_parity(out[f].sum(), ref['lpips32'][f], ref['lpips64'][f], 'after the refusals: lpips, pair %d' % f)


def test_files_to_image_eval_with_lpips_weights(tmp_path):
    """Producer to consumer: harness.write_image leaves two held-out views and a training view in the reference's tree, torch.save a
    weight file in lpips' layout (and one file holding both), tools/image_eval.py --lpips-weights on them against image_metrics."""
    from honerf_amd import harness, image_metrics as im
    ours, gt = image_pairs(37, 41)
    ours, gt = ours[:2], gt[:2]
    gt_dir = tmp_path / 'final_render_img' / 'p1_box' / '000010' / 'MASK'
    our_dir = tmp_path / 'analys_res' / '12' / 'p1_box' / '000010' / 'render_12'
    gt_dir.mkdir(parents=True)
    our_dir.mkdir(parents=True)
    names = ['image_2132004%d.ppm' % v for v in range(2)]
    for v, name in enumerate(names):
        harness.write_image(str(gt_dir / name), gt[v])
        harness.write_image(str(our_dir / name), ours[v])
    harness.write_image(str(gt_dir / 'image_21320027.ppm'), gt[0])             # a training view: skipped, and it has no render
    sd, lin = state_dicts(weights(), 'net.')
    torch.save(sd, str(tmp_path / 'vgg.pth'))
    torch.save(lin, str(tmp_path / 'lin.pth'))
    torch.save(dict(sd, **lin), str(tmp_path / 'both.pth'))
    loaded = im.LpipsVgg.load(str(tmp_path / 'vgg.pth'), str(tmp_path / 'lin.pth'))
    want = im.image_metrics(ours, gt, lpips=loaded)
    assert want['lpips'].tobytes() == _np(model().lpips(ours, gt)).tobytes()
    record('producer to consumer: lpips_mean', want['lpips_mean'], 1.0, kind='value')
    torch.cuda.synchronize()
    tool = [sys.executable, os.path.join(ROOT, 'tools', 'image_eval.py'), str(tmp_path / 'final_render_img'), str(tmp_path / 'analys_res')]
    env = dict(os.environ, PYTHONPATH=ROOT)
    out_json = tmp_path / 'per_file.json'
    run = subprocess.run(tool + ['--json', str(out_json), '--lpips-weights', str(tmp_path / 'vgg.pth'), str(tmp_path / 'lin.pth')], capture_output=True, text=True,
                         timeout=600, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    three = ['2', '     psnr,     ssim,     lpips', 'ours:  %.4f %.6f %.6f' % (want['psnr_mean'], want['ssim_mean'], want['lpips_mean'])]
    assert run.stdout.splitlines() == three, (run.stdout, want)
    with open(str(out_json)) as f:
        per_file = json.load(f)
    assert sorted(per_file) == ['p1_box+000010+' + n for n in names]
    assert [per_file['p1_box+000010+' + n]['lpips'] for n in names] == want['lpips'].tolist()
    run = subprocess.run(tool + ['--lpips-weights', str(tmp_path / 'both.pth')], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0 and run.stdout.splitlines() == three, (run.stdout, run.stderr[-2000:])
    # without the option: today's lines
    run = subprocess.run(tool + ['--json', str(out_json)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines() == ['2', '     psnr,     ssim', 'ours:  %.4f %.6f' % (want['psnr_mean'], want['ssim_mean'])], run.stdout
    with open(str(out_json)) as f:
        assert all(sorted(v) == ['psnr', 'ssim'] for v in json.load(f).values())
