"""Times of the device image metrics: `hn_im_sse` and `hn_im_ssim` (without and with the S map) on F images of H x W, 64 of 512 x 334
by default (the reference's image size).  Both kernels read each of the two images once (the SSIM tiles re-read their 6-pixel halo:
38 / 32 x 70 / 64 = 1.30 times the bytes); the rate printed is the 2 F H W 3 bytes of the inputs over the time, beside the part's
HBM peak of 8 TB/s.  The SSIM kernel is not bound by memory: per window and channel it makes 14 LDS byte reads, about 50 integer
and 30 fp64 operations, one fp64 division among them.

Device events around a window of `--iters` calls after `--warmup` untimed ones; the median of `--rounds` such windows.  Needs a GPU.

    python tools/image_metrics_bench.py [--images 64] [--height 512] [--width 334] [--iters 50] [--warmup 3] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s


def timed(fn, iters, warmup, rounds):
    """Median over `rounds` windows of the device time of one call (ms)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=334)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('image_metrics_bench: no GPU')
    from honerf_amd import lib
    F, H, W = args.images, args.height, args.width
    r = np.random.RandomState(0)
    a = torch.from_numpy(r.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)).cuda()
    b = torch.from_numpy(r.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)).cuda()
    L = lib.load()
    need = int(L.hn_im_workspace_bytes(F, H, W))
    if need == 0:
        raise SystemExit('image_metrics_bench: %d images of %d x %d are beyond one call' % (F, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    sse = torch.empty(F, dtype=torch.int64, device='cuda')
    ch = torch.empty(F, 3, dtype=torch.float64, device='cuda')
    s_map = torch.empty(F, H - 6, W - 6, 3, dtype=torch.float32, device='cuda')
    P, S = lib.ptr, lib.stream_ptr()
    calls = {
        'sse': lambda: lib.check(L.hn_im_sse(P(a), P(b), F, H, W, P(sse), P(ws), need, S), 'hn_im_sse'),
        'ssim': lambda: lib.check(L.hn_im_ssim(P(a), P(b), F, H, W, P(ch), None, P(ws), need, S), 'hn_im_ssim'),
        'ssim_with_map': lambda: lib.check(L.hn_im_ssim(P(a), P(b), F, H, W, P(ch), P(s_map), P(ws), need, S), 'hn_im_ssim'),
    }
    read = 2.0 * F * H * W * 3
    rows = {}
    for name, fn in calls.items():
        ms, every = timed(fn, args.iters, args.warmup, args.rounds)
        rate = read / (ms * 1e-3)
        rows[name] = dict(ms=ms, ms_min=min(every), ms_max=max(every), input_bytes_per_s=rate, share_of_hbm_peak=rate / HBM_PEAK)
        print('%-14s F %d  %d x %d | %8.4f ms (min %.4f max %.4f) | %.3e input bytes/s = %5.2f %% of the %.1f TB/s HBM peak'
              % (name, F, H, W, ms, min(every), max(every), rate, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12), flush=True)
    print(json.dumps(dict(tool='image_metrics_bench', device=torch.cuda.get_device_name(0), images=F, height=H, width=W, input_bytes=read,
                          iters=args.iters, rounds=args.rounds, rows=rows)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
