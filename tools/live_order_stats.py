"""What the sample ORDER of the dense hand-field launch costs on the bench frame (C2: 512 x 512 rays x 64 samples, synth_hand_pose(9),
the bench camera and pixel grid), counted on the CPU with numpy -- no GPU, no library.

A wave of the field kernel owns 32 consecutive samples and pays feature generation, the stash round trips and the Jacobian pass's
contraction for every bone whose mask is non-zero in ANY of its lanes (`nz`); the four waves of a 128-sample tile wait for the slowest
one.  The table compares the dense order (ray after ray) with the live-first order of DESIGN.md 3.1: [samples the ordering pass
classifies as live | the others], each part in dense order.

The depths are the renderer's own (k_coarse_z: the two-sided linspace + (t_rand - 0.5) * sample_dist; k_sample_points: section
mid-points), the rays _xy_to_ray_bundle's, the mask the kernel's (h_b = 1 - 1 / (1 + exp(-200 (v_b - cutoff_b))) in fp32, live where
h_b != 0), the classification the ordering pass's (far only if 200 (v_b - cutoff_b) > 17 for every bone: hn_api.hip, HAND_FAR_ABOVE).  t_rand is drawn here from
numpy's generator, not from the device's: the same distribution, other draws.

    python tools/live_order_stats.py [--seed 9] [--size 512] [--samples 64]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from honerf_amd import synth  # noqa: E402

NEAR, FAR = np.float32(0.4), np.float32(1.5)
CUTOFF = np.array([0.08, 0.03, 0.03, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02,
                   0.02], dtype=np.float32)


def bench_rays(size):
    """bench.build_scene's pixel grid through front_camera(dist=0, focal=2): unproject at depth 1 and 2, d = normalize(p2 - p1), o = p1 - d."""
    xy = synth.ndc_grid(size, size) * np.float32(0.45)
    xy[:, 1] += np.float32(0.12)
    cam = synth.front_camera(dist=0.0, focal=2.0)
    f, pp, R, T = cam['focal'][0], cam['principal'][0], cam['R'][0], cam['T'][0]

    def unproject(depth):
        z = np.full((len(xy), 1), depth, dtype=np.float32)
        xv = np.concatenate([(xy[:, 0:1] - pp[0]) * z / f[0], (xy[:, 1:2] - pp[1]) * z / f[1], z], axis=-1)
        return (xv - T) @ R.T
    p1, p2 = unproject(1.0), unproject(2.0)
    d = p2 - p1
    d = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-12).astype(np.float32)
    return (p1 - d).astype(np.float32), d.astype(np.float32)


def depths(t_rand, n):
    """k_coarse_z, then k_sample_points with mid = 1 -> the depths of the evaluated points [B, n]."""
    k = np.arange(n, dtype=np.float32)
    step = np.float32(1.0) / np.float32(n - 1)
    lin = np.where(k < n // 2, k * step, np.float32(1.0) - (np.float32(n - 1) - k) * step).astype(np.float32)
    sample_dist = np.float32((float(FAR) - float(NEAR)) / n)
    z = (NEAR + (FAR - NEAR) * lin)[None, :] + (t_rand - np.float32(0.5)) * sample_dist
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], sample_dist)], axis=-1)
    return z + dist * np.float32(0.5)


def classify(o, d, t, bt_inv, T_pose, chunk=2048):
    """-> (bits [N] uint32: bit b set where the kernel's mask of bone b is non-zero, live [N] bool: the ordering pass's classification)"""
    B, n = t.shape
    bits = np.zeros(B * n, dtype=np.uint32)
    live = np.zeros(B * n, dtype=bool)
    Rm, tm = bt_inv[:, :3, :3], bt_inv[:, :3, 3] - T_pose
    one = np.float32(1.0)
    for a in range(0, B, chunk):
        p = (o[a:a + chunk, None, :] + d[a:a + chunk, None, :] * t[a:a + chunk, :, None]).reshape(-1, 3)
        q = np.einsum('bij,nj->nbi', Rm, p) + tm
        x = np.float32(200.0) * (np.sqrt((q * q).sum(-1)) - CUTOFF)
        with np.errstate(over='ignore'):
            hh = one - one / (one + np.exp(-x))
        s = slice(a * n, a * n + len(p))
        bits[s] = ((hh != 0).astype(np.uint32) << np.arange(21, dtype=np.uint32)).sum(-1, dtype=np.uint32)
        live[s] = (~(x > np.float32(17.0))).any(-1)
    return bits, live


def popcount(v):
    v = v.astype(np.uint32)
    c = np.zeros(v.shape, dtype=np.int64)
    for b in range(21):
        c += (v >> np.uint32(b)) & np.uint32(1)
    return c


def stats(bits):
    """The figures of one order of the launch (bits in launch order)."""
    n = len(bits)
    pad = (-n) % 128
    w = np.bitwise_or.reduce(np.concatenate([bits, np.zeros(pad, dtype=np.uint32)]).reshape(-1, 32), axis=1)
    per_wave = popcount(w)
    n_waves = (n + 31) // 32
    per_wave_valid = per_wave[:n_waves]
    tiles = per_wave.reshape(-1, 4)
    return {'waves with nz != 0': 100.0 * float((per_wave_valid != 0).mean()),
            'bone-wave pairs per wave (mean nz count)': float(per_wave_valid.mean()),
            'tiles with a live wave': 100.0 * float((tiles.max(1) != 0).mean()),
            "bones of a tile's slowest wave (mean)": float(tiles.max(1).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=9, help='synth_hand_pose seed (bench.py: 9 on rank 0)')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--samples', type=int, default=64)
    args = ap.parse_args()
    bt_inv, T_pose, _ = synth.synth_hand_pose(args.seed)
    o, d = bench_rays(args.size)
    t_rand = np.random.default_rng(1).random((len(o), 1), dtype=np.float32)
    bits, live = classify(o, d, depths(t_rand, args.samples), bt_inv, T_pose)
    order = np.concatenate([np.flatnonzero(live), np.flatnonzero(~live)])      # stable: each part keeps the dense order
    dense, first = stats(bits), stats(bits[order])
    print('C2 frame: %d x %d rays x %d samples, synth_hand_pose(%d)' % (args.size, args.size, args.samples, args.seed))
    print('| quantity | dense order | live samples first (stable) |')
    print('|---|---|---|')
    print('| samples with a live bone (kernel mask) | %.1f %% | same |' % (100.0 * float((bits != 0).mean())))
    print('| samples the ordering pass puts first | %.1f %% | same |' % (100.0 * float(live.mean())))
    for k in dense:
        fmt = '| %s | %.1f %% | %.1f %% |' if k.startswith(('waves', 'tiles')) else '| %s | %.2f | %.2f |'
        print(fmt % (k, dense[k], first[k]))
    per_ray = (bits != 0).reshape(-1, args.samples).sum(1)
    print('rays with a live sample: %.1f %%, live samples on such a ray: mean %.1f' % (100.0 * float((per_ray != 0).mean()), float(per_ray[per_ray != 0].mean())))


if __name__ == '__main__':
    main()
