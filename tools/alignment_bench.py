"""Times the alignment kernels (hn_align.hip through honerf_amd.alignment) with device events.

  procrustes   F = 10 000 frames of 21 joints and of 778 vertices: the whole `procrustes` call (moments, solve, apply, RMS) and its two
               kernels alone, against the batched torch.linalg.svd formulation on the same device (centre, H = B^T A, SVD, determinant
               correction, scale, translation, apply: what a caller without this module writes).
  icp          one ICP iteration at 100 000 surface samples against a mesh of about 20 000 faces, split into its parts: apply, the
               closest-point query, the weights, moments, solve, compose.

After a warm-up round every arm runs --runs times (at least 7); min / median / max per arm.  Nothing is promised: the numbers are what
the tool measured.  Writes profiles/alignment/alignment_bench.json.

    python tools/alignment_bench.py [--runs 9] [--out profiles/alignment/alignment_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _time(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _arms(arms, runs):
    times = {k: [] for k in arms}
    for rnd in range(runs + 1):                                      # round 0 warms every arm up
        for k, fn in arms.items():
            t, _ = _time(fn)
            if rnd:
                times[k].append(t)
    return {k: dict(min_ms=float(np.min(v)), median_ms=float(np.median(v)), max_ms=float(np.max(v))) for k, v in times.items()}


def torch_svd_procrustes(a, b):
    """The batched float64 torch formulation: a, b fp32 [F, N, 3] -> (R, s, t, aligned fp32)."""
    import torch
    a, b = a.double(), b.double()
    ca, cb = a.mean(1, keepdim=True), b.mean(1, keepdim=True)
    da, db = a - ca, b - cb
    H = db.transpose(1, 2) @ da
    U, S, Vh = torch.linalg.svd(H)
    d = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))
    D = torch.ones_like(S)
    D[:, 2] = d
    R = (U * D[:, None]) @ Vh
    s = (S * D).sum(1) / (da * da).sum((1, 2))
    t = cb[:, 0] - s[:, None] * (R @ ca.transpose(1, 2))[..., 0]
    return R, s, t, (s[:, None, None] * (a @ R.transpose(1, 2)) + t[:, None]).float()


def bench_procrustes(F, N, runs):
    import torch
    from honerf_amd import alignment
    rs = np.random.RandomState(N)
    a = torch.from_numpy((0.8 + 0.05 * rs.uniform(-1, 1, (F, N, 3))).astype(np.float32)).cuda()
    b = torch.from_numpy((0.3 + 0.07 * rs.uniform(-1, 1, (F, N, 3))).astype(np.float32)).cuda()
    m = alignment._moments(a, b, None)
    arms = {'procrustes (moments + solve + apply + rms)': lambda: alignment.procrustes(a, b),
            'hn_align_moments': lambda: alignment._moments(a, b, None),
            'hn_align_solve': lambda: alignment._solve(m, True)}
    note = None
    try:
        Rt = torch_svd_procrustes(a, b)[0]
        arms['torch.linalg.svd formulation'] = lambda: torch_svd_procrustes(a, b)
        diff = float((Rt - alignment.procrustes(a, b)['R']).abs().max())
    except Exception as e:                                             # (a build of torch without a batched device SVD)
        note, diff = 'torch.linalg.svd formulation failed: %s' % (str(e).splitlines() or [''])[0], None
    rows = _arms(arms, runs)
    print('== procrustes %d x %d%s' % (F, N, '' if diff is None else ': max |R - R_svd| = %.2e' % diff))
    for k, r in rows.items():
        print('  %-46s min %9.3f  median %9.3f  max %9.3f ms' % (k, r['min_ms'], r['median_ms'], r['max_ms']))
    return dict(frames=F, points=N, arms=rows, max_R_difference_to_svd=diff, note=note)


def bench_icp(n, runs):
    import torch
    from alignment_cases import rotation
    from mesh_distance_cases import uv_sphere
    from honerf_amd import alignment
    from honerf_amd.mesh_distance import MeshIndex, sample_surface
    v, t = uv_sphere(1.0, n_lat=100, n_lon=100)                        # 19 800 faces
    d = v.astype(np.float64)
    r = 0.05 * (1.0 + 0.3 * d[:, 0] + 0.2 * d[:, 1] ** 2 - 0.25 * d[:, 1] * d[:, 2] + 0.2 * d[:, 2] ** 3)
    mesh = torch.from_numpy((d * r[:, None] + np.array([0.1, -0.2, 0.5])).astype(np.float32)).cuda(), torch.from_numpy(t).cuda()
    index = MeshIndex(mesh)
    c = mesh[0].double().mean(0).cpu().numpy()
    R0 = rotation([0.2, 1.0, -0.4], np.deg2rad(5.0))
    p = alignment.transform(sample_surface(mesh, n, seed=1)[0], R0, 1.0, c - R0 @ c + 0.003)[None].contiguous()
    dev = p.device
    acc = (torch.eye(3, dtype=torch.float64, device=dev)[None].contiguous(), torch.ones(1, dtype=torch.float64, device=dev),
           torch.zeros(1, 3, dtype=torch.float64, device=dev))
    moved = alignment._apply(p, *acc)
    q = index.closest(moved[0], want=('dist', 'point'))
    w = (q['dist'] <= 0.05).to(torch.float32)[None].contiguous()
    qp = q['point'][None].contiguous()
    m = alignment._moments(moved, qp, w)
    step = alignment._solve(m, False)[:3]
    arms = {'apply (hn_align_apply)': lambda: alignment._apply(p, *acc),
            'query (MeshIndex.closest: dist, point)': lambda: index.closest(moved[0], want=('dist', 'point')),
            'weights (torch)': lambda: (q['dist'] <= 0.05).to(torch.float32)[None].contiguous(),
            'moments (hn_align_moments)': lambda: alignment._moments(moved, qp, w),
            'solve (hn_align_solve)': lambda: alignment._solve(m, False),
            'compose (hn_align_compose)': lambda: alignment._compose(step, acc),
            'icp, 10 iterations': lambda: alignment.icp(p[0], index, iters=10, max_distance=0.05)}
    rows = _arms(arms, runs)
    print('== one ICP iteration: %d samples x %d faces' % (n, t.shape[0]))
    for k, r in rows.items():
        print('  %-46s min %9.3f  median %9.3f  max %9.3f ms' % (k, r['min_ms'], r['median_ms'], r['max_ms']))
    return dict(samples=n, faces=int(t.shape[0]), arms=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--frames', type=int, default=10000)
    ap.add_argument('--samples', type=int, default=100000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'alignment', 'alignment_bench.json'))
    args = ap.parse_args()
    if args.runs < 7:
        raise SystemExit('alignment_bench: at least 7 runs per arm')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('alignment_bench: no GPU (the timings are device events)')
    res = dict(device=torch.cuda.get_device_name(0), runs=args.runs,
               procrustes=[bench_procrustes(args.frames, 21, args.runs), bench_procrustes(args.frames, 778, args.runs)],
               icp=bench_icp(args.samples, args.runs))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
