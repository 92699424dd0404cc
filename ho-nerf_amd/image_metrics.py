"""Image metrics on the device (hn_imgmetric.hip, hn_lpips.hip): the PSNR, SSIM and LPIPS of analys_results/analys_psnr_ssim_lpips.py
without skimage, cv2, lpips or torchvision, batched over the images.

The reference scores every held-out render against its ground-truth image on the CPU (get_metric, :12-35):
  psnr   skimage's peak_signal_noise_ratio(data_range=255): 10 log10(255^2 / mse), mse the mean over all H W 3 values of (a - b)^2;
         identical images give +inf;
  ssim   skimage's structural_similarity(channel_axis=2, data_range=255): per channel a 7 x 7 uniform window, sample covariance
         (49 / 48), C1 = (0.01 255)^2, C2 = (0.03 255)^2, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), the mean
         of S over the map cropped by 3 pixels on every side (exactly the windows that lie inside the image), then the mean of the
         three channels;
  lpips  lpips.LPIPS(net='vgg') on x = u8 / 128 - 1 (:28-33, :44): `LpipsVgg` below, built from weights the caller supplies (the
         pretrained VGG16 and the linear layers are files of torchvision and lpips; nothing here downloads them).  DESIGN.md 3.18.
DESIGN.md 3.16 is the contract.  The reference only ever scores 8-bit files; here the images ARE 8-bit, the squared error is an exact
integer and the SSIM window sums are exact integers, evaluated in fp64.

Arguments are numpy arrays or torch tensors, on either device, uint8, [F, H, W, 3] or [H, W, 3] (both arguments of one rank and one
shape, H and W at least 7); they are moved to the current CUDA device.  `sse`, `psnr`, `ssim` and `ssim_map` return device tensors;
`image_metrics`, the summary, reads everything back once and returns numpy arrays and floats.
"""
import ctypes
import sys

import numpy as np
import torch

from . import lib as _lib
from .interaction import _check, _device


def _image(x, what):
    """x -> a detached contiguous uint8 tensor [F, H, W, 3] on the current device, and whether it came as [H, W, 3]."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError('%s: expected a numpy array or a torch tensor, got %s' % (what, type(x).__name__))
    if x.dtype != torch.uint8:
        raise ValueError('%s: dtype %s, expected torch.uint8 (8-bit images, as the files the reference scores)' % (what, x.dtype))
    if x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError('%s: shape %s, expected [F, H, W, 3] or [H, W, 3]' % (what, tuple(x.shape)))
    if x.numel() == 0:
        raise ValueError('%s: shape %s is empty' % (what, tuple(x.shape)))
    if x.shape[-3] < 7 or x.shape[-2] < 7:
        raise ValueError('%s: shape %s, the 7 x 7 window needs images of at least 7 x 7' % (what, tuple(x.shape)))
    flat = x.dim() == 3
    x = x.detach().to(_device())
    return (x[None] if flat else x).contiguous(), flat


def _pair(a, b, what_a, what_b):
    a, flat_a = _image(a, what_a)
    b, flat_b = _image(b, what_b)
    if flat_a != flat_b:
        raise ValueError('%s is %d-D and %s is %d-D: pass both as [H, W, 3] or both as [F, H, W, 3]' % (what_a, 3 if flat_a else 4, what_b,
                                                                                                          3 if flat_b else 4))
    if a.shape != b.shape:
        raise ValueError('%s is %s and %s is %s' % (what_a, tuple(a.shape[flat_a:]), what_b, tuple(b.shape[flat_b:])))
    return a, b, flat_a


# ---- private passes on checked uint8 device tensors [F, H, W, 3] ---------------------------------------------------------------------
def _workspace(a, what):
    F, H, W = a.shape[:3]
    need = int(_lib.load().hn_im_workspace_bytes(F, H, W))
    if need == 0:
        raise ValueError('%s: %d images of %d x %d are beyond what one call takes (F x H x W x 3 below 2^31)' % (what, F, H, W))
    return torch.empty(need, dtype=torch.uint8, device=a.device)


def _sse(a, b):
    F, H, W = a.shape[:3]
    with torch.cuda.device(a.device):
        ws = _workspace(a, 'sse')
        out = torch.empty(F, dtype=torch.int64, device=a.device)
        _check(_lib.load().hn_im_sse(_lib.ptr(a), _lib.ptr(b), F, H, W, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'sse')
    return out


def _ssim(a, b, want_map=False):
    """-> (per-channel means float64 [F, 3], the S map float32 [F, H - 6, W - 6, 3] or None)."""
    F, H, W = a.shape[:3]
    with torch.cuda.device(a.device):
        ws = _workspace(a, 'ssim')
        ch = torch.empty(F, 3, dtype=torch.float64, device=a.device)
        s_map = torch.empty(F, H - 6, W - 6, 3, dtype=torch.float32, device=a.device) if want_map else None
        _check(_lib.load().hn_im_ssim(_lib.ptr(a), _lib.ptr(b), F, H, W, _lib.ptr(ch), _lib.ptr(s_map), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr()), 'ssim')
    return ch, s_map


def _psnr_of(sse_, n_values):
    """10 log10(255^2 / (sse / N)) in fp64; sse = 0 gives +inf, as skimage's division by a zero mse does."""
    mse = sse_.double() / float(n_values)
    return 10.0 * torch.log10(65025.0 / mse)


def _ssim_of(ch):
    """The mean of the three channel means, in the order numpy's mean of three takes them."""
    return ((ch[:, 0] + ch[:, 1]) + ch[:, 2]) / 3.0


# ---- public queries ------------------------------------------------------------------------------------------------------------------
def sse(a, b):
    """The exact sum over each image's H W 3 values of (a - b)^2 -> int64 [F] on the device (0-d for [H, W, 3] inputs)."""
    a, b, flat = _pair(a, b, 'a', 'b')
    s = _sse(a, b)
    return s[0] if flat else s


def psnr(a, b):
    """peak_signal_noise_ratio(a, b, data_range=255) (analys_psnr_ssim_lpips.py:23-24) per image -> float64 [F] on the device;
    +inf for identical images."""
    a, b, flat = _pair(a, b, 'a', 'b')
    p = _psnr_of(_sse(a, b), a[0].numel())
    return p[0] if flat else p


def ssim(a, b):
    """structural_similarity(a, b, channel_axis=2, data_range=255) (analys_psnr_ssim_lpips.py:25-26) per image -> float64 [F] on
    the device."""
    a, b, flat = _pair(a, b, 'a', 'b')
    s = _ssim_of(_ssim(a, b)[0])
    return s[0] if flat else s


def ssim_map(a, b):
    """The S map behind `ssim`: float32 [F, H - 6, W - 6, 3] on the device ([H - 6, W - 6, 3] for [H, W, 3] inputs), one value per
    7 x 7 window inside the image and channel (skimage's full=True map without its 3-pixel border)."""
    a, b, flat = _pair(a, b, 'a', 'b')
    m = _ssim(a, b, want_map=True)[1]
    return m[0] if flat else m


def image_metrics(pred, gt, lpips=None):
    """get_metric (analys_psnr_ssim_lpips.py:12-35) for all images at once: pred, gt uint8 [F, H, W, 3] (or [H, W, 3]).
    Returns a dict of float64 numpy arrays 'psnr', 'ssim' [F] (0-d for 3-D inputs) and floats 'psnr_mean', 'ssim_mean' (the means the
    reference prints, :77-78); with `lpips`, an `LpipsVgg`, also 'lpips' and 'lpips_mean' (:79; H and W at least 16 then).  One
    read-back."""
    p, g, flat = _pair(pred, gt, 'pred', 'gt')
    if lpips is not None:
        if not isinstance(lpips, LpipsVgg):
            raise ValueError('lpips: expected an LpipsVgg, got %s' % type(lpips).__name__)
        _at_least_16(p, 'pred')
    rows = [_psnr_of(_sse(p, g), p[0].numel()), _ssim_of(_ssim(p, g)[0])]
    if lpips is not None:
        rows.append(_lpips_of(lpips._layers(p, g)))
    host = torch.stack(rows).cpu().numpy()
    ps, ss = host[0], host[1]
    out = dict(psnr_mean=float(ps.mean()), ssim_mean=float(ss.mean()))
    out['psnr'], out['ssim'] = (ps[0], ss[0]) if flat else (ps, ss)
    if lpips is not None:
        out['lpips_mean'] = float(host[2].mean())
        out['lpips'] = host[2][0] if flat else host[2]
    return out


# ---- LPIPS ---------------------------------------------------------------------------------------------------------------------------
VGG_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)        # the Conv2d modules of torchvision's vgg16().features
VGG_CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
VGG_CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)                            # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LPIPS_WORKSPACE_LIMIT = 1 << 30            # bytes of workspace one device call may take; larger batches are split (same bits)


def _lpips_slice(i):
    """The slice of lpips' `vgg16` wrapper (net.slice1 .. net.slice5) that holds features module i."""
    return 1 + sum(i >= first for first in (4, 9, 16, 23))


def _backbone_names(i, leaf):
    return ('features.%d.%s' % (i, leaf), '%d.%s' % (i, leaf), 'net.slice%d.%d.%s' % (_lpips_slice(i), i, leaf))


def _at_least_16(x, what):
    if x.shape[1] < 16 or x.shape[2] < 16:
        raise ValueError('%s: shape %s, LPIPS needs images of at least 16 x 16 (its fifth tap is floor(H / 16) x floor(W / 16))' % (what, tuple(x.shape)))


def _lpips_of(layers):
    """The sum of the five tap means, in order."""
    return (((layers[:, 0] + layers[:, 1]) + layers[:, 2]) + layers[:, 3]) + layers[:, 4]


def lpips_vgg_tensors(backbone_state, lin_state=None):
    """The tensors `LpipsVgg` takes from its state dicts (its docstring lists the layouts): (13 conv weights, 13 biases, 5 linear
    weights [1, C, 1, 1]) as they lie in the dicts.  Touches no device.  ValueError names every missing or mis-shaped key."""
    lin_state = backbone_state if lin_state is None else lin_state
    bad, conv_w, conv_b, lin_w = [], [], [], []
    for i, cin, cout in zip(VGG_CONV_INDEX, VGG_CONV_CIN, VGG_CONV_COUT):
        _lib.pick_tensor(backbone_state, _backbone_names(i, 'weight'), (cout, cin, 3, 3), conv_w, bad)
        _lib.pick_tensor(backbone_state, _backbone_names(i, 'bias'), (cout,), conv_b, bad)
    for k, c in enumerate(LPIPS_TAP_CHANNELS):
        _lib.pick_tensor(lin_state, ('lin%d.model.1.weight' % k,), (1, c, 1, 1), lin_w, bad)
    if bad:
        raise ValueError('LpipsVgg: ' + '; '.join(bad))
    return conv_w, conv_b, lin_w


class LpipsVgg:
    """lpips.LPIPS(net='vgg') in its defaults (version 0.1, linear layers on, spatial off, eval mode) on the device, hn_lpips.hip.

    `backbone_state` maps names to tensors (or numpy arrays) and holds the 13 convolutions of VGG16's `features` under one of
      features.<i>.weight | bias        torchvision's vgg16().state_dict()
      <i>.weight | bias                 vgg16().features.state_dict()
      net.slice<k>.<i>.weight | bias    a whole lpips.LPIPS(net='vgg').state_dict()
    (i = 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28; weights [Cout, Cin, 3, 3]); `lin_state` holds the five linear layers as
    lin<k>.model.1.weight, [1, C, 1, 1] (lpips' own layout; None: they are in `backbone_state` too).  classifier.*, lins.*,
    scaling_layer.* and every other key are ignored.  A missing key or a wrong shape raises ValueError naming every offending key.
    These layouts are stated from the two packages' public formats; neither package is installed where this was written and tested,
    so the tests build such dicts themselves.

    The model lives on the CUDA device that is current when it is made.  Images are uint8 [F, H, W, 3] or [H, W, 3], numpy or torch,
    H and W at least 16; they enter the network as u8 / 128 - 1 (analys_psnr_ssim_lpips.py:28-31: 128, not 127.5)."""

    def __init__(self, backbone_state, lin_state=None):
        conv_w, conv_b, lin_w = lpips_vgg_tensors(backbone_state, lin_state)
        self._handle = None
        self.device = _device()
        with torch.cuda.device(self.device):
            self.conv_weight = [_lib.f32(w, self.device) for w in conv_w]
            self.conv_bias = [_lib.f32(b, self.device) for b in conv_b]
            self.lin_weight = [_lib.f32(w, self.device).reshape(-1) for w in lin_w]
            arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            handle = ctypes.c_void_p()
            _check(_lib.load().hn_lpips_create(arr(self.conv_weight), arr(self.conv_bias), arr(self.lin_weight), ctypes.byref(handle), _lib.stream_ptr()),
                   'LpipsVgg')
        self._handle = handle

    @classmethod
    def load(cls, backbone_path, lin_path=None):
        """From files written with torch.save: a state dict of one of the layouts above, and lpips' linear-layer file (None: one
        file holds both)."""
        backbone = torch.load(backbone_path, map_location='cpu')
        lin = torch.load(lin_path, map_location='cpu') if lin_path is not None else None
        for what, state in (('backbone', backbone), ('lin', lin)):
            if state is not None and not isinstance(state, dict):
                raise ValueError('LpipsVgg.load: the %s file holds a %s, expected a state dict' % (what, type(state).__name__))
        return cls(backbone, lin)

    def __del__(self):
        handle, self._handle = getattr(self, '_handle', None), None
        if handle is not None and not sys.is_finalizing():       # at interpreter exit the driver takes the allocation back
            try:
                _lib.load().hn_lpips_destroy(handle)
            except Exception:
                pass

    def _per_call(self, F, H, W, what):
        """How many images (pairs) of H x W one device call takes within LPIPS_WORKSPACE_LIMIT: at least 1."""
        wsb = _lib.load().hn_lpips_workspace_bytes
        one = int(wsb(1, H, W))
        if one == 0:
            raise ValueError('%s: images of %d x %d are beyond what one call takes (2 x H x W x 64 below 2^31)' % (what, H, W))
        n = max(1, min(F, LPIPS_WORKSPACE_LIMIT // one))
        while n > 1 and not 0 < int(wsb(n, H, W)) <= LPIPS_WORKSPACE_LIMIT:
            n -= 1
        return n, int(wsb(n, H, W))

    def _layers(self, a, b):
        """Checked uint8 device tensors [F, H, W, 3] -> the five tap means, float64 [F, 5]."""
        F, H, W = a.shape[:3]
        if a.device != self.device:
            raise ValueError('lpips: the images are on %s, the model is on %s' % (a.device, self.device))
        L = _lib.load()
        with torch.cuda.device(a.device):
            n, need = self._per_call(F, H, W, 'lpips')
            ws = torch.empty(need, dtype=torch.uint8, device=a.device)
            out = torch.empty(F, 5, dtype=torch.float64, device=a.device)
            for s in range(0, F, n):
                e = min(F, s + n)
                _check(L.hn_lpips(self._handle, _lib.ptr(a[s:e]), _lib.ptr(b[s:e]), e - s, H, W, _lib.ptr(out[s:e]), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr()), 'lpips')
        return out

    def lpips_layers(self, a, b):
        """The five tap means of every pair -> float64 [F, 5] on the device ([5] for [H, W, 3] inputs); their sum is `lpips`."""
        a, b, flat = _pair(a, b, 'a', 'b')
        _at_least_16(a, 'a')
        t = self._layers(a, b)
        return t[0] if flat else t

    def lpips(self, a, b):
        """lpips.LPIPS(net='vgg')(a / 128 - 1, b / 128 - 1) (analys_psnr_ssim_lpips.py:28-33) per pair -> float64 [F] on the device
        (0-d for [H, W, 3] inputs)."""
        a, b, flat = _pair(a, b, 'a', 'b')
        _at_least_16(a, 'a')
        v = _lpips_of(self._layers(a, b))
        return v[0] if flat else v

    def features(self, img):
        """The five taps of every image, after the scaling layer: a list of five float32 tensors [F, C, h, w] on the device
        ([C, h, w] for an [H, W, 3] input), C = 64, 128, 256, 512, 512 and h x w = floor(H / 2^k) x floor(W / 2^k)."""
        x, flat = _image(img, 'img')
        _at_least_16(x, 'img')
        F, H, W = x.shape[:3]
        if x.device != self.device:
            raise ValueError('features: the images are on %s, the model is on %s' % (x.device, self.device))
        L = _lib.load()
        with torch.cuda.device(x.device):
            n, need = self._per_call(F, H, W, 'features')
            ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            taps = [torch.empty(F, c, H >> k, W >> k, dtype=torch.float32, device=x.device) for k, c in enumerate(LPIPS_TAP_CHANNELS)]
            for s in range(0, F, n):
                e = min(F, s + n)
                _check(L.hn_lpips_features(self._handle, _lib.ptr(x[s:e]), e - s, H, W, *[_lib.ptr(t[s:e]) for t in taps], _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr()), 'features')
        return [t[0] for t in taps] if flat else taps
