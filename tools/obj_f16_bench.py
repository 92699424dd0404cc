"""The object field's single-pass mode (precision='f16', k_field2_obj_f16<0|1>) against the f16x3 kernels, both in ONE process, alternating,
every shape warmed up, device events around the timed launches:
  (a) hn_field_eval / hn_field_sdf of a conf-size object field over 2^22 points on the C1 frame's rays between its near and far planes,
  (b) the C1 frame (bench.build_scene_c1 / bench.render_c1),
  (c) harness.render_views of the synthetic two-field scene (bench.build_fit) at 512 x 334, 2 views, fixed t_rand, both fields f16x3 and
      both fields f16, with the per-view PSNR / SSIM of the f16 images against the f16x3 images (honerf_amd.image_metrics).
Prints one JSON line (profiles/obj_f16/obj_f16_bench.json is a committed run).
   python tools/obj_f16_bench.py [--reps 7] [--points 4194304] [--legs abc]"""
import argparse
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

import bench
from honerf_amd import harness, synth
from honerf_amd import lib as L
from honerf_amd.image_metrics import image_metrics
from honerf_amd.nets import PackedField

MODES = ('f16x3', 'f16')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(fns, reps):
    """fns: {mode: callable}.  One warm-up call each, then `reps` rounds of f16x3, f16, f16x3, ... -> {mode: [ms]}."""
    for m in MODES:
        fns[m]()
    torch.cuda.synchronize()
    ms = {m: [] for m in MODES}
    for _ in range(reps):
        for m in MODES:
            ms[m].append(timed(fns[m])[0])
    return ms


def stats(ms):
    a = sorted(ms)
    return {'min': a[0], 'median': float(np.median(a)), 'max': a[-1], 'n': len(a)}


def leg(ms):
    """min / median / max per mode, the ratio of the medians and whether the gain exceeds the run-to-run spread of either mode."""
    s = {m: stats(ms[m]) for m in MODES}
    spread = max(s[m]['max'] - s[m]['min'] for m in MODES)
    gain = s['f16x3']['median'] - s['f16']['median']
    return {'ms': s, 'f16x3_over_f16': s['f16x3']['median'] / s['f16']['median'], 'gain_ms': gain, 'spread_ms': spread,
            'gain_exceeds_spread': bool(gain > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--points', type=int, default=1 << 22)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=334)
    ap.add_argument('--legs', default='abc', help='which legs to run')
    args = ap.parse_args()
    assert args.reps >= 5
    dev = torch.device('cuda')
    lib = L.load()
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps}

    # ---- (a) the field kernels alone
    rens = {m: bench.build_scene_c1(dev, m) for m in MODES}
    _, sdf_net, col_net, sc = rens['f16x3']
    fields = {m: PackedField('obj', sdf_net, col_net, 0.3, precision=m) for m in MODES}
    if 'a' in args.legs:
        spr = 256
        n_rays = args.points // spr
        N = n_rays * spr
        B = sc['xy'].shape[0]
        o, d = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
        L.check(lib.hn_ray_gen(L.ptr(sc['xy']), L.ptr(sc['R']), L.ptr(sc['T']), L.ptr(sc['focal']), L.ptr(sc['principal']), 1, B, L.ptr(o), L.ptr(d),
                               L.stream_ptr()), 'hn_ray_gen')
        gen = torch.Generator('cpu').manual_seed(7)
        pick = torch.randint(0, B, (n_rays,), generator=gen).to(dev)
        z = (bench.NEAR + (bench.FAR - bench.NEAR) * torch.rand(n_rays, spr, 1, generator=gen)).to(dev)
        dirs = d[pick].contiguous()
        pts = (o[pick][:, None, :] + dirs[:, None, :] * z).reshape(N, 3).contiguous()
        out = {m: (torch.empty(N, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)) for m in MODES}
        need = max(lib.hn_field_workspace_bytes(fields[m].handle, N) for m in MODES)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def full(m):
            def run():
                L.check(lib.hn_field_eval(fields[m].handle, L.ptr(pts), L.ptr(dirs), N, spr, None, None, 1, N, L.ptr(out[m][0]), L.ptr(out[m][1]),
                                          L.ptr(out[m][2]), None, L.ptr(ws), need, L.stream_ptr()), 'hn_field_eval')
            return run

        def sdf_only(m):
            def run():
                L.check(lib.hn_field_sdf(fields[m].handle, L.ptr(pts), N, None, None, 1, N, L.ptr(out[m][0]), L.ptr(ws), need, L.stream_ptr()), 'hn_field_sdf')
            return run

        res['a_field_eval'] = dict(leg(alternate({m: full(m) for m in MODES}, args.reps)), points=N,
                                   kernels={'f16x3': 'k_field2_obj<1>', 'f16': 'k_field2_obj_f16<1>'})
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
        res['a_field_eval']['f16_vs_f16x3'] = {k: rel(out['f16'][i], out['f16x3'][i]) for i, k in enumerate(('sdf', 'grad', 'rgb'))}
        res['a_field_sdf'] = dict(leg(alternate({m: sdf_only(m) for m in MODES}, args.reps)), points=N,
                                  kernels={'f16x3': 'k_field2_obj<0>', 'f16': 'k_field2_obj_f16<0>'})

    # ---- (b) the C1 frame
    c1 = {}
    if 'b' in args.legs:
        res['b_c1_frame'] = leg(alternate({m: (lambda m=m: c1.__setitem__(m, bench.render_c1(rens[m][0], rens[m][3], L))) for m in MODES}, args.reps))
        res['b_c1_frame']['f16_vs_f16x3'] = {k: rel(c1['f16'][k], c1['f16x3'][k]) for k in ('color_fine', 'weight_sum')}
    del fields

    # ---- (c) held-out views of the two-field scene
    if 'c' in args.legs:
        H, W, V = args.height, args.width, 2
        chain, j, _ = bench.build_fit_data(dev, 40, 1, halo=True)
        with torch.no_grad():
            pose = chain()
        bt_inv, T21 = pose['bt_inv'][0].detach().contiguous(), pose['T_pose_21'][0].detach().contiguous()
        Ro, To = pose['obj_r'][0].detach().contiguous(), pose['obj_t'][0].detach().contiguous()
        cams = synth.ring_cameras(V, radius=1.0, target=tuple(float(c) for c in j[9]), seed=3)
        t_rand = torch.rand(V, H * W, 1, generator=torch.Generator().manual_seed(5)).to(dev)
        imgs = {}
        # one renderer per mode (the same seeded networks): a timed call is render_views alone, not the re-pack a change of mode costs
        rens2 = {}
        for m in MODES:
            rens2[m] = bench.build_fit(dev, 40, 1, bench.FIT_RAYS, m, halo=True)[0]
            rens2[m].precision = m
        run2 = {m: (lambda m=m: imgs.__setitem__(m, harness.render_views(rens2[m], cams, H, W, bench.NEAR, bench.FAR, bt_inv, T21, Ro, To, t_rand=t_rand)))
                for m in MODES}
        res['c_render_views'] = dict(leg(alternate(run2, 5)), height=H, width=W, views=V)
        met = image_metrics(imgs['f16'], imgs['f16x3'])
        res['c_render_views']['f16_vs_f16x3'] = {'psnr': [float(x) for x in met['psnr']], 'ssim': [float(x) for x in met['ssim']],
                                                 'worst_grey_levels': int((imgs['f16'].int() - imgs['f16x3'].int()).abs().max())}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
