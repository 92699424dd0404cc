"""Times of the fused geometry-buffer kernel (hn_gbuffer2, ho-nerf_amd/csrc/hn_gbuffer.hip) against the same buffers from the entry points
that existed before it, at one 512 x 334 view x 192 samples by default, alternating in one process:

  fused     one hn_gbuffer2 launch: reads sdf, gradient (both fields) and the depths once, 36 B per ray-sample, writes 40 B per ray
  unfused   hn_sample_points (mid-points and dists), hn_alpha x 2, hn_composite2 with both weight arrays written out, then the torch
            reductions over [rays, S]: sum w, sum w m, sum w grad per field, and the object's normal times Ro

The inputs are seeded: sorted depths in [0.4, 1.5], per ray and field an sdf that crosses zero somewhere along the ray with slope -cos,
gradients -cos d + noise; inv_s 14.9 / 20.1 (the synthetic fields' values).  The times do not depend on the values.

Device events around `--reps` back-to-back calls of an arm after `--warmup` untimed rounds of both; min / median / max of the per-call
time over `--runs` alternating runs; the fused kernel's achieved bytes per second from the bytes the algorithm needs (computed from the
shapes) over its median time, next to the HBM peak of MI355X_MICROARCH.md; and the largest relative difference between the two arms'
buffers.  Writes the JSON line to `--out` as well.  Needs a GPU.

    python tools/gbuffer_bench.py [--height 334] [--width 512] [--samples 192] [--runs 7] [--reps 10] [--warmup 2] [--out profiles/gbuffer/gbuffer_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12      # bytes / s, MI355X_MICROARCH.md
NEAR, FAR, N_SAMPLES = 0.4, 1.5, 64


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--height', type=int, default=334)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--samples', type=int, default=192)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gbuffer', 'gbuffer_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gbuffer_bench: no GPU')
    if args.runs < 5:
        raise SystemExit('gbuffer_bench: at least 5 runs')
    from honerf_amd import lib as L
    lib = L.load()
    dev = torch.device('cuda')
    N, S = args.height * args.width, args.samples
    g = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    unit = lambda v: torch.nn.functional.normalize(v, dim=-1)
    sample_dist = (FAR - NEAR) / N_SAMPLES
    z = torch.sort(NEAR + (FAR - NEAR) * rnd(N, S), -1)[0].contiguous()
    rays_o = rnd(N, 3) - 0.5
    d_h = unit(rnd(N, 3) - 0.5)
    Ro = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(1)))[0].to(dev).reshape(1, 3, 3).contiguous()
    d_o = (d_h @ Ro[0].T).contiguous()
    inv_s = (14.9, 20.1)
    f = {}
    for k, d in (('h', d_h), ('o', d_o)):
        cos = 0.3 + 0.7 * rnd(N, 1)
        z_s = NEAR + (FAR - NEAR) * (0.25 + 0.5 * rnd(N, 1))
        f['sdf_' + k] = ((z_s - z) * cos).contiguous()
        f['grad_' + k] = (-cos[:, :, None] * d[:, None, :] + 0.4 * (rnd(N, S, 3) - 0.5)).contiguous()
        f['rgb_' + k] = rnd(N, S, 3)
        f['alpha_' + k] = torch.empty(N, S, device=dev)
        f['w_' + k] = torch.empty(N, S, device=dev)
    pts, dists = torch.empty(N * S, 3, device=dev), torch.empty(N, S, device=dev)
    color, wsum = torch.empty(N, 3, device=dev), torch.empty(N, device=dev)
    opacity, depth, normal = torch.empty(N, 2, device=dev), torch.empty(N, 2, device=dev), torch.empty(N, 2, 3, device=dev)
    st = L.stream_ptr()
    P = L.ptr

    def fused():
        L.check(lib.hn_gbuffer2(P(f['sdf_h']), P(f['grad_h']), P(d_h), inv_s[0], P(f['sdf_o']), P(f['grad_o']), P(d_o), inv_s[1], P(z), 1, N, S,
                                sample_dist, P(Ro), P(opacity), P(depth), P(normal), st), 'hn_gbuffer2')
        return opacity, depth, normal

    def unfused():
        L.check(lib.hn_sample_points(P(rays_o), P(d_h), P(z), N, S, 1, sample_dist, P(pts), P(dists), st), 'hn_sample_points')
        for k, d, s in (('h', d_h, inv_s[0]), ('o', d_o, inv_s[1])):
            L.check(lib.hn_alpha(P(f['sdf_' + k]), P(f['grad_' + k]), P(d), P(dists), N * S, S, s, P(f['alpha_' + k]), None, st), 'hn_alpha')
        L.check(lib.hn_composite2(P(f['alpha_h']), P(f['rgb_h']), None, P(f['alpha_o']), P(f['rgb_o']), None, N, S, P(color), P(wsum), P(f['w_h']),
                                  P(f['w_o']), None, st), 'hn_composite2')
        mid = z + 0.5 * dists
        op = torch.stack([f['w_h'].sum(-1), f['w_o'].sum(-1)], -1)
        dp = torch.stack([(f['w_h'] * mid).sum(-1), (f['w_o'] * mid).sum(-1)], -1)
        n_h = (f['w_h'][:, :, None] * f['grad_h']).sum(1)
        n_o = (f['w_o'][:, :, None] * f['grad_o']).sum(1) @ Ro[0]
        return op, dp, torch.stack([n_h, n_o], 1)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.reps):
            out = fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / args.reps, out

    arms = {'fused': fused, 'unfused': unfused}
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times, last = {k: [] for k in arms}, {}
        for _ in range(args.runs):
            for name, fn in arms.items():
                ms, out = timed(fn)
                times[name].append(ms)
                last[name] = [t.double().cpu() for t in out]
    diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(last['fused'], last['unfused']))
    fused_bytes = N * S * (2 * (4 + 12) + 4) + N * (2 * 12 + 36 + 40)        # per-sample reads; per ray: two directions, Ro, the 10 outputs
    rows = {}
    for name, t in times.items():
        rows[name] = dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), ms_all=t)
        print('%-8s %d rays x %d samples | per call: min %8.3f  median %8.3f  max %8.3f ms' % (name, N, S, min(t), float(np.median(t)), max(t)), flush=True)
    bps = fused_bytes / (rows['fused']['ms_median'] * 1e-3)
    print('fused: %.1f MB per call -> %.0f GB/s, %.2f of the %.0f GB/s HBM peak; unfused / fused = %.1f; largest relative difference %.1e'
          % (fused_bytes / 1e6, bps / 1e9, bps / HBM_PEAK, HBM_PEAK / 1e9, rows['unfused']['ms_median'] / rows['fused']['ms_median'], diff))
    line = json.dumps(dict(tool='gbuffer_bench', device=torch.cuda.get_device_name(0), height=args.height, width=args.width, rays=N, samples=S,
                           runs=args.runs, reps=args.reps, warmup=args.warmup, fused_bytes_per_call=fused_bytes, fused_bytes_per_s=bps,
                           fused_share_of_hbm_peak=bps / HBM_PEAK, hbm_peak_bytes_per_s=HBM_PEAK,
                           unfused_over_fused=rows['unfused']['ms_median'] / rows['fused']['ms_median'], largest_relative_difference=diff, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
