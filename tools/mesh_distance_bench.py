"""Times the culled closest-point query (hn_meshdist.hip through honerf_amd.mesh_distance.MeshIndex) against the brute force
(hn_closest_distance) on the same points, with device events.

Cases: the synthetic hand and object of tests/test_interaction.py (tools/interaction_bench.py's) at 64^3 (get_res.py) and 256^3
(exp_runner --mode mesh).  Two queries per case, the two directions a surface comparison makes: the hand's vertices against the object
mesh (the penetration depth's query) and the object's vertices against the hand mesh.  Arms: cull on / off, triangles in Morton /
identity order, query points sorted / unsorted, and the brute force.  Every arm is a whole Python CALL of `closest` on a prepared
index (its kernel plus the Morton sort and scatter of the points where it sorts); preparing the index is timed on its own.  After a
warm-up round the arms run alternately, --runs rounds (at least 7); min / median / max per arm.  All arms' distances must be the same
bits.  Writes profiles/meshdist/mesh_distance_bench.json.

    python tools/mesh_distance_bench.py [--runs 9] [--cases hand64 hand256] [--out profiles/meshdist/mesh_distance_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _time(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def run_query(name, mesh, points, runs):
    import torch
    from honerf_amd import interaction as it
    from honerf_amd.mesh_distance import MeshIndex
    m, = it._meshes((mesh, name))
    p = it._points(points, name)
    prep = {}
    index = {}
    for order in ('morton', 'identity'):
        MeshIndex(m, order=order)                                   # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t, index[order] = _time(lambda: MeshIndex(m, order=order))
            ts.append(t)
        prep[order] = float(np.median(ts))
    arms = {'brute': lambda: it._distance(m, p)}
    for order in ('morton', 'identity'):
        for cull in (True, False):
            for sort in (True, False):
                arms['%s cull=%d sort=%d' % (order, cull, sort)] = (
                    lambda o=order, c=cull, s=sort: index[o].closest(p, cull=c, sort=s, want=('dist',))['dist'])
    times = {k: [] for k in arms}
    bits = {}
    for rnd in range(runs + 1):                                     # round 0 warms every arm up
        for k, fn in arms.items():
            t, d = _time(fn)
            if rnd:
                times[k].append(t)
            else:
                bits[k] = d.cpu().numpy().tobytes()
    same = all(b == bits['brute'] for b in bits.values())
    rows = {k: dict(min_ms=float(np.min(v)), median_ms=float(np.median(v)), max_ms=float(np.max(v))) for k, v in times.items()}
    P, T = p.shape[0], m.t.shape[0]
    print('== %s: %d points x %d triangles; prepare: morton %.3f ms, identity %.3f ms; all arms the same bits: %s' % (name, P, T, prep['morton'],
                                                                                                                   prep['identity'], same))
    for k, r in rows.items():
        print('  %-28s min %9.3f  median %9.3f  max %9.3f ms' % (k, r['min_ms'], r['median_ms'], r['max_ms']))
    assert same, '%s: an arm gave other bits than the brute force' % name
    best = rows['morton cull=1 sort=1']
    brute = rows['brute']
    gain = brute['min_ms'] > best['max_ms']                          # the medians differ by more than the arms' own min - max spread
    return dict(query=name, points=P, triangles=T, prepare_ms=prep, arms=rows, same_bits=same, culled_beats_brute_beyond_spread=bool(gain),
                speedup_median=brute['median_ms'] / best['median_ms'])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--cases', nargs='+', default=['hand64', 'hand256'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'meshdist', 'mesh_distance_bench.json'))
    args = ap.parse_args()
    if args.runs < 7:
        raise SystemExit('mesh_distance_bench: at least 7 runs per arm')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mesh_distance_bench: no GPU (the timings are device events)')
    from interaction_bench import _hand_object
    res = []
    for c in args.cases:
        hand, obj = _hand_object(int(c[4:]))
        res.append(run_query('%s: hand vertices -> object mesh' % c, obj, hand[0], args.runs))
        res.append(run_query('%s: object vertices -> hand mesh' % c, hand, obj[0], args.runs))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), runs=args.runs, queries=res), f, indent=1)
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
