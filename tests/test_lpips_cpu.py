"""LPIPS (VGG) of analys_results/analys_psnr_ssim_lpips.py:28-33,44 restated with torch operators (`ref_features`, `ref_layers`), the
yardstick of tests/test_lpips.py, the seeded weight maker both files use, and the state-dict layouts honerf_amd.image_metrics.LpipsVgg
accepts.

lpips and torchvision are not installed where these tests run and are not part of the reference tree, so the restatement is written
from what lpips.LPIPS(net='vgg') documents for its defaults (version 0.1, linear layers on, spatial off, eval mode):
  x = u8 / 128 - 1 (the reference's own scaling, :28-31), the scaling layer (x - shift) / scale with shift = (-0.030, -0.088, -0.188),
  scale = (0.458, 0.448, 0.450); VGG16's `features`: 3x3 convolutions with zero padding 1 and bias, each followed by ReLU, at module
  indices 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, MaxPool2d(2, 2) (floor mode) after 2, 7, 14, 21; the taps are the ReLU outputs
  after 2, 7, 14, 21, 28, BEFORE the pool; per tap n(f) = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w[c] (n(fa) - n(fb))^2, the mean of d
  over the tap's pixels; LPIPS = the sum of the five means.
Parity with the two packages' binaries and with pretrained weights is unpinned: the weights here are seeded random numbers of the
scale a He initialisation gives (activations neither die nor grow through the 13 layers).  The convolution itself is checked against
the definition written out in numpy."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import record
from test_image_metrics_cpu import image_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_AFTER = (2, 7, 14, 21)
TAP_AFTER = (2, 7, 14, 21, 28)
TAP_C = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
SIZES = [(16, 16), (17, 31), (37, 41), (16, 130)]            # (H, W) of tests/test_lpips.py


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def make_weights(seed=0):
    """-> (13 conv weights [Cout, Cin, 3, 3], 13 biases, 5 linear weights [1, C, 1, 1]), float32: randn sqrt(2 / (9 Cin)), 0.1 randn,
    rand / C."""
    g = torch.Generator().manual_seed(seed)
    conv_w = [torch.randn(co, ci, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * ci))) for ci, co in zip(CONV_CIN, CONV_COUT)]
    conv_b = [0.1 * torch.randn(co, generator=g) for co in CONV_COUT]
    lin_w = [torch.rand(1, c, 1, 1, generator=g) / c for c in TAP_C]
    return conv_w, conv_b, lin_w


_WEIGHTS = {}


def weights(variant='plain'):
    """The seed-0 weights, made once and never changed; 'dead': the bias of conv index 2 is -1e3 (the first tap is zero everywhere);
    'range': weight and bias of conv index 0 times 2^15 (the first tap exceeds 1e5, beyond f16's range)."""
    if 'plain' not in _WEIGHTS:
        _WEIGHTS['plain'] = make_weights(0)
    if variant not in _WEIGHTS:
        w, b, lin = (list(x) for x in _WEIGHTS['plain'])
        if variant == 'dead':
            b[1] = torch.full_like(b[1], -1e3)
        elif variant == 'range':
            w[0], b[0] = w[0] * 32768.0, b[0] * 32768.0
        else:
            raise KeyError(variant)
        _WEIGHTS[variant] = (w, b, lin)
    return _WEIGHTS[variant]


def state_dicts(wts, layout):
    """The weights as the state dict of torchvision's vgg16 ('features.'), of its .features (''), or of a whole lpips.LPIPS ('net.')."""
    conv_w, conv_b, lin_w = wts
    sd = {}
    for i, w, b in zip(CONV_INDEX, conv_w, conv_b):
        if layout == 'net.':
            prefix = 'net.slice%d.%d.' % (1 + sum(i >= first for first in (4, 9, 16, 23)), i)
        else:
            prefix = layout + '%d.' % i
        sd[prefix + 'weight'], sd[prefix + 'bias'] = w, b
    lin = {'lin%d.model.1.weight' % k: w for k, w in enumerate(lin_w)}
    return sd, lin


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def ref_features(img, wts, dtype):
    """img uint8 numpy [F, H, W, 3] -> the five taps [F, C, h, w] in `dtype`."""
    conv_w, conv_b, _ = wts
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(0, 3, 1, 2).to(dtype) / 128.0 - 1.0
    x = (x - torch.tensor(SHIFT, dtype=dtype)[None, :, None, None]) / torch.tensor(SCALE, dtype=dtype)[None, :, None, None]
    taps = []
    for i, w, b in zip(CONV_INDEX, conv_w, conv_b):
        x = F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), stride=1, padding=1))
        if i in TAP_AFTER:
            taps.append(x)
        if i in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return taps


def ref_layers_of(taps_a, taps_b, wts):
    """-> the five tap means [F, 5] in the taps' dtype."""
    out = []
    for fa, fb, w in zip(taps_a, taps_b, wts[2]):
        na = fa / (torch.sqrt((fa * fa).sum(1, keepdim=True)) + 1e-10)
        nb = fb / (torch.sqrt((fb * fb).sum(1, keepdim=True)) + 1e-10)
        d = (w.to(fa.dtype) * (na - nb) ** 2).sum(1)
        out.append(d.mean(dim=(1, 2)))
    return torch.stack(out, 1)


def ref_layers(a, b, wts, dtype):
    return ref_layers_of(ref_features(a, wts, dtype), ref_features(b, wts, dtype), wts)


def ref_lpips(layers):
    return (((layers[:, 0] + layers[:, 1]) + layers[:, 2]) + layers[:, 3]) + layers[:, 4]


def np_conv3x3_relu(x, w, b):
    """The definition, written out: out[n, o, y, x] = relu(b[o] + sum_{c, ky, kx} w[o, c, ky, kx] xpad[n, c, y + ky, x + kx]) in float64:
    loops over n, y, x, ky, kx; the sums over o and c as one matrix product per term."""
    n_img, cin, h, wd = x.shape
    xp = np.zeros((n_img, cin, h + 2, wd + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n_img, w.shape[0], h, wd))
    for n in range(n_img):
        for y in range(h):
            for xx in range(wd):
                acc = b.copy()
                for ky in range(3):
                    for kx in range(3):
                        acc = acc + w[:, :, ky, kx] @ xp[n, :, y + ky, xx + kx]
                out[n, :, y, xx] = np.maximum(acc, 0.0)
    return out


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def test_convolution_against_the_definition():
    a, _ = image_pairs(16, 16)
    wts = weights()
    x = a[:1].transpose(0, 3, 1, 2).astype(np.float64) / 128.0 - 1.0
    x = (x - np.array(SHIFT)[None, :, None, None]) / np.array(SCALE)[None, :, None, None]
    y = x
    for l in range(2):
        y = np_conv3x3_relu(y, wts[0][l].double().numpy(), wts[1][l].double().numpy())
    got = ref_features(a[:1], wts, torch.float64)[0].numpy()
    assert got.shape == y.shape == (1, 64, 16, 16)
    e = float(np.abs(got - y).max() / np.abs(y).max())
    record('restatement, first two layers, against the written-out convolution', e, 1e-13)
    assert e <= 1e-13, e
    assert float((y > 0).mean()) > 0.2                           # the taps are alive


def test_tap_shapes_floor_at_every_pool():
    a, _ = image_pairs(17, 31)
    taps = ref_features(a, weights(), torch.float32)
    assert [tuple(t.shape) for t in taps] == [(3, 64, 17, 31), (3, 128, 8, 15), (3, 256, 4, 7), (3, 512, 2, 3), (3, 512, 1, 1)]


@pytest.mark.parametrize('H,W', SIZES)
def test_float32_restatement_against_float64(H, W):
    a, b = image_pairs(H, W)
    wts = weights()
    t64a, t64b = ref_features(a, wts, torch.float64), ref_features(b, wts, torch.float64)
    t32a, t32b = ref_features(a, wts, torch.float32), ref_features(b, wts, torch.float32)
    l64, l32 = ref_layers_of(t64a, t64b, wts), ref_layers_of(t32a, t32b, wts)
    assert l64.dtype == torch.float64 and l32.dtype == torch.float32 and tuple(l64.shape) == (3, 5)
    v = ref_lpips(l64).numpy()
    record('%d x %d lpips, smallest' % (H, W), v.min(), 1.0, kind='value')
    record('%d x %d lpips, largest' % (H, W), v.max(), 1.0, kind='value')
    assert (v > 1e-6).all() and (v < 1e-1).all(), v
    # the float32 reference sits far inside the 1e-4 the device path is held to (tests/helpers.py, assert_parity)
    e_tap = max(float(((x.double() - y).abs().max() / y.abs().max())) for x, y in zip(t32a + t32b, t64a + t64b))
    e_mean = float(((l32.double() - l64).abs() / l64.abs()).max())
    e_total = float(((ref_lpips(l32).double() - ref_lpips(l64)).abs() / ref_lpips(l64)).max())
    for what, e in (('any tap tensor (relative to its largest value)', e_tap), ('any tap mean (relative)', e_mean), ('total (relative)', e_total)):
        record('%d x %d float32 restatement against float64, %s' % (H, W, what), e, 5e-5)
        assert e <= 5e-5, (what, e)
    for t in t64a + t64b:
        assert float((t * t).sum(1).min()) > 0.0                 # no pixel with an all-zero channel vector
    # identical images: exactly 0, in both precisions
    assert ref_lpips(ref_layers_of(t32a, t32a, wts)).tolist() == [0.0] * 3 and ref_lpips(ref_layers_of(t64b, t64b, wts)).tolist() == [0.0] * 3


def test_variants_kill_the_first_tap_and_leave_f16_range():
    a, b = image_pairs(17, 31)
    dead = ref_features(a, weights('dead'), torch.float32)
    assert float(dead[0].abs().max()) == 0.0 and all(float(t.abs().max()) > 0.0 for t in dead[1:])
    layers = ref_layers(a, b, weights('dead'), torch.float32)
    # behind a dead tap the network sees its biases alone: the later taps are alive, the same for both images, and every distance is 0
    assert layers[:, 0].tolist() == [0.0] * 3 and bool(torch.isfinite(layers).all()) and float(layers.abs().max()) == 0.0
    big = ref_features(a, weights('range'), torch.float32)
    assert float(big[0].max()) > 1e5 and all(bool(torch.isfinite(t).all()) for t in big)
    assert weights('plain')[1][1].min() > -1.0 and weights('plain')[0][0].abs().max() < 2.0        # the shared weights are untouched


def test_the_three_key_layouts_load_to_the_same_tensors():
    from honerf_amd.image_metrics import lpips_vgg_tensors
    wts = weights()
    loaded = []
    for layout in ('features.', '', 'net.'):
        sd, lin = state_dicts(wts, layout)
        loaded.append(lpips_vgg_tensors(sd, lin))
        both = dict(sd, **lin)                                                           # one dict holding both, with keys to ignore
        both.update({'classifier.0.weight': torch.zeros(2, 2), 'lins.0.model.1.weight': torch.zeros(1, 3, 1, 1),
                     'scaling_layer.shift': torch.zeros(1, 3, 1, 1), 'features.1.weight': torch.zeros(7), 'net.slice1.1.weight': torch.zeros(7)})
        loaded.append(lpips_vgg_tensors(both))
    assert 'net.slice2.5.weight' in state_dicts(wts, 'net.')[0] and 'net.slice5.28.bias' in state_dicts(wts, 'net.')[0]
    assert 'net.slice3.14.weight' in state_dicts(wts, 'net.')[0] and 'net.slice4.21.weight' in state_dicts(wts, 'net.')[0]
    for got in loaded:
        assert [len(x) for x in got] == [13, 13, 5]
        for x, y in zip(got[0] + got[1] + got[2], wts[0] + wts[1] + wts[2]):
            assert torch.equal(torch.as_tensor(x), y)
    # numpy arrays are taken too
    sd, lin = state_dicts(wts, '')
    got = lpips_vgg_tensors({k: v.numpy() for k, v in sd.items()}, {k: v.numpy() for k, v in lin.items()})
    assert torch.equal(got[0][4], wts[0][4]) and torch.equal(got[2][3], wts[2][3])


def test_missing_and_misshaped_keys_are_named():
    from honerf_amd.image_metrics import LpipsVgg, lpips_vgg_tensors
    wts = weights()
    sd, lin = state_dicts(wts, 'features.')
    short = {k: v for k, v in sd.items() if k not in ('features.7.weight', 'features.28.bias')}
    with pytest.raises(ValueError) as e:
        lpips_vgg_tensors(short, lin)
    assert 'features.7.weight' in str(e.value) and 'features.28.bias' in str(e.value) and 'features.5.weight' not in str(e.value)
    wrong = dict(sd)
    wrong['features.10.weight'] = torch.zeros(256, 128, 3, 2)
    wrong['features.0.bias'] = torch.zeros(63)
    lin_wrong = dict(lin)
    lin_wrong['lin2.model.1.weight'] = torch.zeros(256)
    del lin_wrong['lin4.model.1.weight']
    with pytest.raises(ValueError) as e:
        lpips_vgg_tensors(wrong, lin_wrong)
    for name in ('features.10.weight', 'features.0.bias', 'lin2.model.1.weight', 'lin4.model.1.weight'):
        assert name in str(e.value), (name, str(e.value))
    with pytest.raises(ValueError, match='lin0.model.1.weight'):
        lpips_vgg_tensors(sd)                                                            # no linear layers anywhere
    with pytest.raises(ValueError, match='features.7.weight'):
        LpipsVgg(short, lin)                                                             # refused before any device is touched


def test_the_c_abi_declares_lpips():
    from honerf_amd import lib
    with open(os.path.join(ROOT, 'include', 'honerf.h')) as f:
        text = f.read()
    assert 'analys_psnr_ssim_lpips.py:28-33,44' in text
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, n_args in (('hn_lpips_create', 5), ('hn_lpips_destroy', 1), ('hn_lpips_workspace_bytes', 3), ('hn_lpips', 10), ('hn_lpips_features', 13)):
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, src)
        assert m, name + ' is not declared in include/honerf.h'
        assert len(m.group(1).split(',')) == n_args, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args, name
    assert lib.SIGNATURES['hn_lpips_workspace_bytes'][0] is lib.c_sz
    assert lib.HN_VERSION == 121
