"""Times of the geometry buffers' adjoint kernel (hn_gbuffer2_bwd, ho-nerf_amd/csrc/hn_gbuffer.hip) against the same gradients from the
entry points that existed before it, at one 512 x 334 view x 192 samples and at the fitting size 196 x 192, alternating in one process:

  fused     one hn_gbuffer2_bwd launch: reads sdf, gradient (both fields) and the depths once, 36 B per ray-sample, and writes g_sdf and
            g_grad of both fields, 32 B per ray-sample; alpha, weights and transmittance never reach memory
  unfused   hn_sample_points (mid-points and dists), hn_alpha x 2, the per-sample factors q^f = g_opacity^f + g_depth^f m + g_normal^f . grad^f
            as torch operators written into the first colour channel of each field, hn_composite2_bwd with g_color = (1, 0, 0) (its g_alpha
            is then dL / d alpha^f and its g_rgb channel 0 the weight w^f), hn_alpha_bwd x 2, and g_grad^f += w^f g_normal^f in torch

The inputs are gbuffer_bench's (seeded; sdf crossing zero along the ray, inv_s 14.9 / 20.1), the upstream gradients standard normal.
Device events around `--reps` back-to-back calls of an arm after `--warmup` untimed rounds of both; min / median / max of the per-call
time over `--runs` alternating runs; the fused kernel's achieved bytes per second from the bytes the algorithm needs over its median
time, next to the HBM peak of MI355X_MICROARCH.md; and the largest relative difference between the two arms' gradients (the unfused
arm forms d alpha / d sdf as hn_alpha_bwd does, as a difference of two close terms: DESIGN.md 3.25).  Writes one JSON line with both
sizes to `--out`.  Needs a GPU.

    python tools/gbuffer_bwd_bench.py [--samples 192] [--runs 7] [--reps 10] [--warmup 2] [--out profiles/gbuffer/gbuffer_bwd_bench.json]
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
SIZES = (('view 512 x 334', 512 * 334), ('fitting step', 196))


def bench(L, lib, N, S, args):
    dev = torch.device('cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    unit = lambda v: torch.nn.functional.normalize(v, dim=-1)
    sample_dist = (FAR - NEAR) / N_SAMPLES
    z = torch.sort(NEAR + (FAR - NEAR) * rnd(N, S), -1)[0].contiguous()
    rays_o = rnd(N, 3) - 0.5
    d_h = unit(rnd(N, 3) - 0.5)
    Ro = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(1)))[0].to(dev)
    d_o = (d_h @ Ro.T).contiguous()
    inv_s = (14.9, 20.1)
    n = N * S
    f = {}
    for k, d in (('h', d_h), ('o', d_o)):
        cos = 0.3 + 0.7 * rnd(N, 1)
        z_s = NEAR + (FAR - NEAR) * (0.25 + 0.5 * rnd(N, 1))
        f['sdf_' + k] = ((z_s - z) * cos).contiguous()
        f['grad_' + k] = (-cos[:, :, None] * d[:, None, :] + 0.4 * (rnd(N, S, 3) - 0.5)).contiguous()
        for name, shape in (('alpha_', (N, S)), ('g_alpha_', (N, S)), ('rgb_', (N, S, 3)), ('g_rgb_', (N, S, 3)), ('gs_', (n,)), ('gg_', (n, 3)),
                            ('gd_', (N, 3)), ('us_', (n,)), ('ug_', (n, 3)), ('ud_', (N, 3))):
            f[name + k] = torch.zeros(*shape, device=dev)
    g_op, g_dp, g_nr = (torch.randn(*s, device=dev, generator=g) for s in ((N, 2), (N, 2), (N, 2, 3)))
    pts, dists = torch.empty(n, 3, device=dev), torch.empty(N, S, device=dev)
    g_color = torch.tensor([1.0, 0.0, 0.0], device=dev).repeat(N, 1).contiguous()
    st = L.stream_ptr()
    P = L.ptr

    def fused():
        L.check(lib.hn_gbuffer2_bwd(P(f['sdf_h']), P(f['grad_h']), P(d_h), inv_s[0], P(f['sdf_o']), P(f['grad_o']), P(d_o), inv_s[1], P(z), 1, N, S,
                                    sample_dist, P(g_op), P(g_dp), P(g_nr), P(f['gs_h']), P(f['gg_h']), P(f['gs_o']), P(f['gg_o']), P(f['gd_h']),
                                    P(f['gd_o']), st), 'hn_gbuffer2_bwd')
        return [f[a + k] for k in 'ho' for a in ('gs_', 'gg_', 'gd_')]

    def unfused():
        L.check(lib.hn_sample_points(P(rays_o), P(d_h), P(z), N, S, 1, sample_dist, P(pts), P(dists), st), 'hn_sample_points')
        mid = z + 0.5 * dists
        for i, (k, d, s) in enumerate((('h', d_h, inv_s[0]), ('o', d_o, inv_s[1]))):
            L.check(lib.hn_alpha(P(f['sdf_' + k]), P(f['grad_' + k]), P(d), P(dists), n, S, s, P(f['alpha_' + k]), None, st), 'hn_alpha')
            f['rgb_' + k][:, :, 0] = g_op[:, i, None] + g_dp[:, i, None] * mid + (f['grad_' + k] * g_nr[:, i, None, :]).sum(-1)
        L.check(lib.hn_composite2_bwd(P(f['alpha_h']), P(f['rgb_h']), P(f['alpha_o']), P(f['rgb_o']), P(g_color), None, N, S, P(f['g_alpha_h']),
                                      P(f['g_rgb_h']), P(f['g_alpha_o']), P(f['g_rgb_o']), st), 'hn_composite2_bwd')
        for i, (k, d, s) in enumerate((('h', d_h, inv_s[0]), ('o', d_o, inv_s[1]))):
            L.check(lib.hn_alpha_bwd(P(f['sdf_' + k]), P(f['grad_' + k]), P(d), P(dists), P(f['g_alpha_' + k]), None, n, S, s, P(f['us_' + k]),
                                     P(f['ug_' + k]), P(f['ud_' + k]), st), 'hn_alpha_bwd')
            f['ug_' + k].view(N, S, 3).add_(f['g_rgb_' + k][:, :, :1] * g_nr[:, i, None, :])
        return [f[a + k] for k in 'ho' for a in ('us_', 'ug_', 'ud_')]

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
                last[name] = out      # (the arms write different buffers)
        diff = max(float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max()) for a, b in zip(last['fused'], last['unfused']))
    fused_bytes = n * (2 * (4 + 12) + 4) + n * 2 * (4 + 12) + N * (2 * 12 + 40 + 2 * 12)   # reads, writes; per ray: directions, upstream, g_rays_d
    rows = {name: dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), ms_all=t) for name, t in times.items()}
    for name, r in rows.items():
        print('%-8s %d rays x %d samples | per call: min %8.3f  median %8.3f  max %8.3f ms' % (name, N, S, r['ms_min'], r['ms_median'], r['ms_max']), flush=True)
    bps = fused_bytes / (rows['fused']['ms_median'] * 1e-3)
    print('fused: %.1f MB per call -> %.0f GB/s, %.2f of the %.0f GB/s HBM peak; unfused / fused = %.1f; largest relative difference %.1e'
          % (fused_bytes / 1e6, bps / 1e9, bps / HBM_PEAK, HBM_PEAK / 1e9, rows['unfused']['ms_median'] / rows['fused']['ms_median'], diff), flush=True)
    return dict(rays=N, samples=S, fused_bytes_per_call=fused_bytes, fused_bytes_per_s=bps, fused_share_of_hbm_peak=bps / HBM_PEAK,
                unfused_over_fused=rows['unfused']['ms_median'] / rows['fused']['ms_median'], largest_relative_difference=diff, rows=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--samples', type=int, default=192)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gbuffer', 'gbuffer_bwd_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gbuffer_bwd_bench: no GPU')
    if args.runs < 5:
        raise SystemExit('gbuffer_bwd_bench: at least 5 runs')
    from honerf_amd import lib as L
    lib = L.load()
    sizes = {name: bench(L, lib, N, args.samples, args) for name, N in SIZES}
    line = json.dumps(dict(tool='gbuffer_bwd_bench', device=torch.cuda.get_device_name(0), runs=args.runs, reps=args.reps, warmup=args.warmup,
                           hbm_peak_bytes_per_s=HBM_PEAK, sizes=sizes))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
