"""Image metrics on the device (hn_imgmetric.hip): the PSNR and SSIM of analys_results/analys_psnr_ssim_lpips.py without skimage or
cv2, batched over the images.

The reference scores every held-out render against its ground-truth image on the CPU (get_metric, :12-35):
  psnr   skimage's peak_signal_noise_ratio(data_range=255): 10 log10(255^2 / mse), mse the mean over all H W 3 values of (a - b)^2;
         identical images give +inf;
  ssim   skimage's structural_similarity(channel_axis=2, data_range=255): per channel a 7 x 7 uniform window, sample covariance
         (49 / 48), C1 = (0.01 255)^2, C2 = (0.03 255)^2, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), the mean
         of S over the map cropped by 3 pixels on every side (exactly the windows that lie inside the image), then the mean of the
         three channels;
  lpips  is not computed: it needs pretrained VGG weights.
DESIGN.md 3.16 is the contract.  The reference only ever scores 8-bit files; here the images ARE 8-bit, the squared error is an exact
integer and the SSIM window sums are exact integers, evaluated in fp64.

Arguments are numpy arrays or torch tensors, on either device, uint8, [F, H, W, 3] or [H, W, 3] (both arguments of one rank and one
shape, H and W at least 7); they are moved to the current CUDA device.  `sse`, `psnr`, `ssim` and `ssim_map` return device tensors;
`image_metrics`, the summary, reads everything back once and returns numpy arrays and floats.
"""
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


def image_metrics(pred, gt):
    """get_metric (analys_psnr_ssim_lpips.py:12-35, without LPIPS) for all images at once: pred, gt uint8 [F, H, W, 3] (or [H, W, 3]).
    Returns a dict of float64 numpy arrays 'psnr', 'ssim' [F] (0-d for 3-D inputs) and floats 'psnr_mean', 'ssim_mean' (the means the
    reference prints, :77-78).  One read-back."""
    p, g, flat = _pair(pred, gt, 'pred', 'gt')
    host = torch.stack([_psnr_of(_sse(p, g), p[0].numel()), _ssim_of(_ssim(p, g)[0])]).cpu().numpy()
    ps, ss = host[0], host[1]
    out = dict(psnr_mean=float(ps.mean()), ssim_mean=float(ss.mean()))
    out['psnr'], out['ssim'] = (ps[0], ss[0]) if flat else (ps, ss)
    return out
