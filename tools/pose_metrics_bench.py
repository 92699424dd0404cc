"""Times of the device pose metrics: `pose_metrics` (one method, all passes, its read-back included) and `hn_pm_nearest` alone, for
object models of V vertices over F frames.  The nearest-point search visits F x V x V pairs; its rate is printed in pairs/s next to
the time.  Each pair costs 3 subtractions, a multiply, 2 fused multiply-adds and half a 3-way minimum: 6.5 fp32 vector
instructions.  The part's fp32 vector rate of 157.3 TFLOP/s is reached with packed instructions only; for the one-lane instructions
of this kernel half of it applies (78.6 TFLOP/s = 39.3e12 lane-instructions/s, an FMA counted as two operations), which bounds the
search at 6.0e12 pairs/s.

Device events around a window of calls (about 0.3 s of them, at most `--iters`) after `--warmup` untimed ones; the median of
`--rounds` such windows.  Needs a GPU.

    python tools/pose_metrics_bench.py [--verts 4096 32768] [--frames 8 64] [--iters 2000] [--warmup 3] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_PAIRS = 157.3e12 / 2 / 2 / 6.5      # one-lane instructions: half the packed rate; 2 FLOPs per FMA; 6.5 instructions per pair


def scene(V, F, seed=0):
    r = np.random.RandomState(seed)
    u = r.normal(size=(V, 3))
    model = (u / np.linalg.norm(u, axis=1, keepdims=True) * np.array([0.08, 0.05, 0.03])).astype(np.float32)

    def poses(jitter):
        q, _ = np.linalg.qr(r.normal(size=(F, 3, 3)))
        q *= np.sign(np.linalg.det(q))[:, None, None]
        return dict(joint3d=(r.normal(size=(F, 21, 3)) * 0.05 + [0.0, 0.0, 0.9]).astype(np.float32), Ro=q.astype(np.float32),
                    To=(np.array([0.02, -0.01, 0.9]) + jitter * r.normal(size=(F, 3))).astype(np.float32))
    return model, poses(0.05), poses(0.05)


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
    ap.add_argument('--verts', type=int, nargs='+', default=[4096, 32768])
    ap.add_argument('--frames', type=int, nargs='+', default=[8, 64])
    ap.add_argument('--iters', type=int, default=2000, help='the most calls per timed window')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pose_metrics_bench: no GPU')
    from honerf_amd import pose_metrics as pm
    rows = []
    for V in args.verts:
        for F in args.frames:
            model, pred, gt = scene(V, F)
            dev = {k: {n: torch.from_numpy(a).cuda() for n, a in d.items()} for k, d in (('pred', pred), ('gt', gt))}
            mv = torch.from_numpy(model).cuda()
            c = dev['gt']['To']
            q = pm._transform(mv, dev['gt']['Ro'], dev['gt']['To'], c)
            t = pm._transform(mv, dev['pred']['Ro'], dev['pred']['To'], c)
            ws = torch.empty(max(int(pm._lib.load().hn_pm_workspace_bytes(F, V, V)), 256), dtype=torch.uint8, device='cuda')
            pairs = float(F) * V * V
            # a window of about 0.3 s if the search runs at 30 % of the bound, within [3, --iters] calls
            iters = int(min(args.iters, max(3, 0.3 * 0.3 * PEAK_PAIRS / pairs)))
            nn_ms, nn_all = timed(lambda: pm._nearest(q, t, ws), iters, args.warmup, args.rounds)
            all_ms, all_all = timed(lambda: pm.pose_metrics(mv, dev['pred'], dev['gt']), iters, args.warmup, args.rounds)
            row = dict(verts=V, frames=F, pairs=pairs, iters=iters, nearest_ms=nn_ms, nearest_ms_min=min(nn_all), nearest_ms_max=max(nn_all),
                       nearest_pairs_per_s=pairs / (nn_ms * 1e-3), share_of_one_lane_fp32_bound=pairs / (nn_ms * 1e-3) / PEAK_PAIRS,
                       pose_metrics_ms=all_ms, pose_metrics_ms_min=min(all_all), pose_metrics_ms_max=max(all_all),
                       pose_metrics_pairs_per_s=pairs / (all_ms * 1e-3))
            rows.append(row)
            print('V %6d  F %3d  pairs %.3e | hn_pm_nearest %9.3f ms  %.3e pairs/s (%4.1f %% of the one-lane fp32 bound) | pose_metrics %9.3f ms'
                  '  %.3e pairs/s' % (V, F, pairs, nn_ms, row['nearest_pairs_per_s'], 100 * row['share_of_one_lane_fp32_bound'], all_ms,
                                      row['pose_metrics_pairs_per_s']), flush=True)
    print(json.dumps(dict(tool='pose_metrics_bench', device=torch.cuda.get_device_name(0), rows=rows)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
