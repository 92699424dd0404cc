"""Times of the device LPIPS (hn_lpips.hip + hn_conv3x3.h through honerf_amd.image_metrics.LpipsVgg) on `--pairs` pairs of `--height` x `--width`
images, 2 of 334 x 512 by default (the size of a harness.render_views leg), against the same arithmetic written with torch operators
on the device (F.conv2d, F.max_pool2d: what lpips.LPIPS runs), alternating in one process.  The weights are seeded random numbers
(randn sqrt(2 / (9 Cin)), biases 0.1 randn, linear weights rand / C): the times do not depend on their values.  The HIP path exists
because libhonerf.so is a C ABI without torch in it; the torch form is the yardstick, not a substitute.

Device events around each call after `--warmup` untimed ones of each arm; min / median / max over `--runs` alternating runs, and the
largest relative difference of the two arms' LPIPS values.  Writes the JSON line to `--out` as well.  Needs a GPU.

    python tools/lpips_bench.py [--pairs 2] [--height 334] [--width 512] [--runs 7] [--warmup 2] [--out profiles/lpips/lpips_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAP_C = (64, 128, 256, 512, 512)


def make_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ci, co in zip(CONV_INDEX, CONV_CIN, CONV_COUT):
        sd['features.%d.weight' % i] = torch.randn(co, ci, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * ci)))
        sd['features.%d.bias' % i] = 0.1 * torch.randn(co, generator=g)
    for k, c in enumerate(TAP_C):
        sd['lin%d.model.1.weight' % k] = torch.rand(1, c, 1, 1, generator=g) / c
    return sd


def torch_lpips(sd, a, b):
    """The same metric with torch operators, float32 on the device: a, b uint8 [F, H, W, 3] -> float32 [F]."""
    shift = torch.tensor((-0.030, -0.088, -0.188), device=a.device)[None, :, None, None]
    scale = torch.tensor((0.458, 0.448, 0.450), device=a.device)[None, :, None, None]
    x = torch.cat([a, b]).permute(0, 3, 1, 2).float() / 128.0 - 1.0
    x = (x - shift) / scale
    total, k = 0.0, 0
    for i in CONV_INDEX:
        x = F.relu(F.conv2d(x, sd['features.%d.weight' % i], sd['features.%d.bias' % i], padding=1))
        if i in (2, 7, 14, 21, 28):
            n = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
            d = (sd['lin%d.model.1.weight' % k] * (n[:a.shape[0]] - n[a.shape[0]:]) ** 2).sum(1)
            total = total + d.mean(dim=(1, 2))
            k += 1
        if i in (2, 7, 14, 21):
            x = F.max_pool2d(x, 2, 2)
    return total


def one(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--pairs', type=int, default=2)
    ap.add_argument('--height', type=int, default=334)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips', 'lpips_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lpips_bench: no GPU')
    if args.runs < 5:
        raise SystemExit('lpips_bench: at least 5 runs')
    from honerf_amd.image_metrics import LpipsVgg
    n, H, W = args.pairs, args.height, args.width
    r = np.random.RandomState(0)
    a = torch.from_numpy(r.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)).cuda()
    b = torch.from_numpy(np.clip(a.cpu().numpy().astype(np.int64) + r.randint(-20, 21, size=(n, H, W, 3)), 0, 255).astype(np.uint8)).cuda()
    sd = make_state()
    model = LpipsVgg(sd)
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    arms = {'hip': lambda: model.lpips(a, b), 'torch_operators': lambda: torch_lpips(sd_dev, a, b)}
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times, last = {k: [] for k in arms}, {}
        for _ in range(args.runs):
            for name, fn in arms.items():
                ms, last[name] = one(fn)
                times[name].append(ms)
    diff = float(((last['hip'] - last['torch_operators'].double()).abs() / last['torch_operators'].double().abs()).max())
    gmac = 2 * n * sum(ci * co * 9 * (H >> k) * (W >> k) for ci, co, k in zip(CONV_CIN, CONV_COUT, (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4))) / 1e9
    rows = {}
    for name, t in times.items():
        rows[name] = dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), ms_all=t, tmac_per_s=gmac / float(np.median(t)))
        print('%-16s %d pairs of %d x %d | min %8.3f  median %8.3f  max %8.3f ms | %.1f GMAC -> %.1f TMAC/s' % (name, n, H, W, min(t), float(np.median(t)),
                                                                                                            max(t), gmac, gmac / float(np.median(t))), flush=True)
    line = json.dumps(dict(tool='lpips_bench', device=torch.cuda.get_device_name(0), pairs=n, height=H, width=W, runs=args.runs, warmup=args.warmup,
                           conv_gmac=gmac, lpips_hip=last['hip'].tolist(), lpips_torch_operators=last['torch_operators'].tolist(),
                           largest_relative_difference=diff, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
