"""The image metrics of analys_results/analys_psnr_ssim_lpips.py:23-26 restated in float64 numpy (`np_sse`, `np_psnr`, `np_ssim_map`,
`np_ssim`), the yardstick of tests/test_image_metrics.py, and the scene maker both files use.

skimage and cv2 are not installed where these tests run and are not part of the reference tree, so the restatement is written from
the algorithm skimage documents for structural_similarity(channel_axis=2, data_range=255) on 8-bit-valued input: per channel a
7 x 7 uniform window, sample covariance (cov_norm = 49 / 48), C1 = (0.01 255)^2, C2 = (0.03 255)^2,
S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), the mean of S over the map cropped by 3 pixels on every side
-- exactly the (H - 6) x (W - 6) windows inside the image, so no border rule enters -- and the mean of the three channel means.
Parity with skimage's own binary is unpinned (as pytorch3d's is for ray generation).  The window sums are exact integers from
cumulative sums; a second, independent route (scipy.ndimage.uniform_filter in float64) is compared when scipy imports, and the
distance of the same formula evaluated in float32 -- what skimage runs on the reference's float32 arrays -- is recorded.

Here as well: closed forms, the PPM reader and writer of honerf_amd.harness, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from helpers import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = (0.01 * 255.0) * (0.01 * 255.0), (0.03 * 255.0) * (0.03 * 255.0)
SIZES = [(7, 7), (8, 130), (37, 41), (64, 96), (70, 75)]       # (H, W) of tests/test_image_metrics.py


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def np_sse(a, b):
    """[H, W, 3] uint8 x 2 -> the exact integer sum of (a - b)^2."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def np_psnr(a, b):
    """peak_signal_noise_ratio(a, b, data_range=255): 10 log10(255^2 / mse); +inf for identical images."""
    mse = np.float64(np_sse(a, b)) / np.float64(a.size)
    with np.errstate(divide='ignore'):
        return np.float64(10.0) * np.log10(np.float64(65025.0) / mse)


def _window_sums(z):
    """z int64 [H, W, 3] -> the sums over every 7 x 7 window inside the image, int64 [H - 6, W - 6, 3] (cumulative sums, exact)."""
    c = np.zeros((z.shape[0] + 1, z.shape[1] + 1, 3), dtype=np.int64)
    c[1:, 1:] = z.cumsum(0).cumsum(1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def np_ssim_map(a, b):
    """[H, W, 3] uint8 x 2 -> S float64 [H - 6, W - 6, 3]."""
    x, y = a.astype(np.int64), b.astype(np.int64)
    sx, sy, sxx, syy, sxy = (_window_sums(z) for z in (x, y, x * x, y * y, x * y))
    ux, uy = sx.astype(np.float64) / 49.0, sy.astype(np.float64) / 49.0
    vx = (49 * sxx - sx * sx).astype(np.float64) / 2352.0          # 49 * 48: the sample variance from exact integers
    vy = (49 * syy - sy * sy).astype(np.float64) / 2352.0
    vxy = (49 * sxy - sx * sy).astype(np.float64) / 2352.0
    a1, a2 = 2.0 * ux * uy + C1, 2.0 * vxy + C2
    b1, b2 = ux * ux + uy * uy + C1, vx + vy + C2
    return (a1 * a2) / (b1 * b2)


def np_ssim_channels(a, b):
    return np_ssim_map(a, b).mean(axis=(0, 1))


def np_ssim(a, b):
    return np.float64(np_ssim_channels(a, b).mean())


def np_ssim_float32(a, b):
    """The same formula as skimage evaluates it on float32 arrays: window MEANS of x, y, xx, yy, xy (separable 7-sums) and
    cov_norm (uxx - ux ux) in float32, the crop, the means in float64 (skimage's crop(S, 3).mean(dtype=float64))."""
    def mean7(z):
        h = sum(z[:, k:z.shape[1] - 6 + k] for k in range(7)) / np.float32(7)
        return sum(h[k:h.shape[0] - 6 + k] for k in range(7)) / np.float32(7)
    x, y = a.astype(np.float32), b.astype(np.float32)
    ux, uy, uxx, uyy, uxy = mean7(x), mean7(y), mean7(x * x), mean7(y * y), mean7(x * y)
    n = np.float32(49.0 / 48.0)
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    c1, c2 = np.float32(C1), np.float32(C2)
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    assert S.dtype == np.float32
    return np.float64(S.mean(axis=(0, 1), dtype=np.float64).mean())


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def image_pairs(H, W, seed=0):
    """Three different pairs (a, b) of uint8 [3, H, W, 3]: a smooth sinusoidal texture with per-channel offsets against itself plus
    Gaussian noise of sigma 4, the same with another phase and sigma 12, and a flat image against itself with one pixel zeroed."""
    r = np.random.RandomState(1000 * H + W + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b = np.empty((3, H, W, 3), dtype=np.uint8), np.empty((3, H, W, 3), dtype=np.uint8)
    for k, (sigma, phase) in enumerate(((4.0, 0.3), (12.0, 1.7))):
        tex = np.stack([110.0 + 20.0 * c + 60.0 * np.sin(0.21 * xx + phase + 0.5 * c) * np.cos(0.13 * yy - 0.4 * c) + 25.0 * np.sin(0.05 * (xx + yy))
                        for c in range(3)], axis=-1)
        a[k] = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
        b[k] = np.clip(np.rint(tex + sigma * r.standard_normal(tex.shape)), 0, 255).astype(np.uint8)
    a[2] = 200
    b[2] = 200
    b[2, H // 2, W // 3] = 0
    return a, b


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', SIZES)
def test_restatement_against_uniform_filter_and_float32(H, W):
    a, b = image_pairs(H, W)
    f32 = 0.0
    for k in range(3):
        s = np_ssim(a[k], b[k])
        assert 0.0 < s < 1.0
        f32 = max(f32, abs(np_ssim_float32(a[k], b[k]) - s))
    # recorded, not asserted tightly: what the float32 evaluation of the reference's call differs by from the float64 restatement
    record('%d x %d: SSIM, the float32 formula against the float64 restatement' % (H, W), f32, 1e-4, kind='abs')
    print('float32 path distance %d x %d: %.3e' % (H, W, f32))
    assert f32 < 1e-4
    ndi = pytest.importorskip('scipy.ndimage')
    worst = 0.0
    for k in range(3):
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        filt = lambda z: ndi.uniform_filter(z, size=(7, 7, 1))
        ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
        n = 49.0 / 48.0
        vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        worst = max(worst, abs(float(S[3:-3, 3:-3].mean(axis=(0, 1)).mean()) - np_ssim(a[k], b[k])))
    record('%d x %d: SSIM, scipy uniform_filter in float64 against the restatement' % (H, W), worst, 1e-12, kind='abs')
    assert worst < 1e-12           # the float64 moments cancel where the integers do not: 4e-15 observed


def test_the_cases_span_low_and_high_ssim():
    vals = [np_ssim(a[k], b[k]) for H, W in SIZES for a, b in [image_pairs(H, W)] for k in range(3)]
    assert min(vals) < 0.5 and max(vals) > 0.8, (min(vals), max(vals))


def test_closed_forms():
    a, b = image_pairs(37, 41)
    for k in range(3):
        assert np_ssim(a[k], a[k]) == 1.0 and (np_ssim_map(a[k], a[k]) == 1.0).all()
        assert np_psnr(a[k], a[k]) == np.inf and np_sse(a[k], a[k]) == 0
    # one 7 x 7 window by hand: x flat 200, y the same with one pixel zeroed
    x = np.full((7, 7, 3), 200, dtype=np.uint8)
    y = x.copy()
    y[3, 2] = 0
    uy = 200.0 * 48 / 49
    vy = (48 * 200.0 ** 2 - 49 * uy ** 2) / 48                      # sample variance: (sum y^2 - n uy^2) / (n - 1)
    by_hand = (2 * 200.0 * uy + C1) * C2 / ((200.0 ** 2 + uy ** 2 + C1) * (vy + C2))
    S = np_ssim_map(x, y)
    assert S.shape == (1, 1, 3)
    assert np.abs(S - by_hand).max() < 1e-15 and abs(np_ssim(x, y) - by_hand) < 1e-15
    assert abs(by_hand - 0.0669) < 1e-3
    assert np_sse(x, y) == 3 * 200 ** 2
    assert abs(np_psnr(x, y) - 10 * np.log10(65025.0 * 147 / 120000.0)) < 1e-12
    # a constant image against itself with one pixel changed: the 49 windows that hold the pixel give the value above, the others 1
    H, W = 20, 23
    x = np.full((H, W, 3), 200, dtype=np.uint8)
    y = x.copy()
    y[9, 11] = 0
    S = np_ssim_map(x, y)
    hit = np.zeros((H - 6, W - 6), dtype=bool)
    hit[3:10, 5:12] = True                                          # windows whose rows 9 - 6 .. 9 and columns 11 - 6 .. 11 start there
    assert np.abs(S[hit] - by_hand).max() < 1e-15 and (S[~hit] == 1.0).all()
    n = (H - 6) * (W - 6)
    assert abs(np_ssim(x, y) - (49 * by_hand + (n - 49)) / n) < 1e-14


@pytest.mark.parametrize('H,W', [(1, 1), (7, 5), (33, 41)])
def test_ppm_round_trip(tmp_path, H, W):
    from honerf_amd import harness
    img = np.random.RandomState(H * W).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    path = str(tmp_path / 'x.ppm')
    harness.write_image(path, img)
    with open(path, 'rb') as f:
        data = f.read()
    assert data == b'P6\n%d %d\n255\n' % (W, H) + img.tobytes()     # channels as they are in the array
    back = harness.read_image(path)
    assert back.dtype == np.uint8 and back.shape == (H, W, 3) and back.tobytes() == img.tobytes()
    import torch
    harness.write_image(path, torch.from_numpy(img))
    assert harness.read_image(path).tobytes() == img.tobytes()
    with open(path, 'wb') as f:                                     # a header with a comment, as other writers leave
        f.write(b'P6\n# made elsewhere\n%d %d\n255\n' % (W, H) + img.tobytes())
    assert harness.read_image(path).tobytes() == img.tobytes()


def test_ppm_refusals(tmp_path):
    from honerf_amd import harness
    img = np.arange(5 * 4 * 3, dtype=np.uint8).reshape(5, 4, 3)
    path = str(tmp_path / 'x.ppm')
    body = img.tobytes()
    for data, what in ((b'P5\n4 5\n255\n' + body, 'magic'), (b'P6\n4 5\n65535\n' + body + body, 'maxval'), (b'P6\n4 5\n255\n' + body[:-1], 'truncated'),
                       (b'P6\n4 5\n', 'truncated'), (b'P6\n4 5\n255', 'truncated'), (b'', 'magic')):
        with open(path, 'wb') as f:
            f.write(data)
        with pytest.raises(ValueError, match=what):
            harness.read_image(path)
    for bad in (img.astype(np.float32), img[..., :2], img[0], np.zeros((0, 4, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match='write_image'):
            harness.write_image(path, bad)
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match='PIL'):
            harness.write_image(str(tmp_path / 'x.png'), img)
        with pytest.raises(RuntimeError, match='PIL'):
            harness.read_image(str(tmp_path / 'x.png'))


def test_the_abi_declares_the_image_metrics():
    from honerf_amd import lib
    with open(os.path.join(ROOT, 'include', 'honerf.h')) as f:
        header = f.read()
    for name, n_args in (('hn_im_workspace_bytes', 3), ('hn_im_sse', 9), ('hn_im_ssim', 10)):
        m = re.search(r'\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/honerf.h'
        assert len(m.group(2).split(',')) == n_args, (name, m.group(2))
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args, name
    assert lib.SIGNATURES['hn_im_workspace_bytes'][0] is lib.c_sz
    assert lib.HN_VERSION == 121 and re.search(r'#define HN_VERSION 121\b', header)
