"""Times the interaction kernels (hn_interact.hip through honerf_amd.interaction) with device events.

Cases: the synthetic hand and object of tests/test_interaction.py (synth_hand_pose(3), the object posed at joint 9 in a +-0.35 m box)
at 64^3 (get_res.py) and 256^3 (exp_runner --mode mesh), and a pair of analytic spheres.  Every row is a whole Python CALL timed with
device events (median of --iters): its kernels plus whatever host read-backs and torch plumbing the call makes (voxelize_surface
includes the key-total read-back and torch.unique).  Kernel times alone come from a `rocprofv3 --kernel-trace --stats` run of this
tool.  Per call: pairs per second (points x triangles; the containment pass skips points outside the mesh's bounds, so 'pairs' there
counts the points inside them) and, over the call time, the share of two ceilings for the FLOPs per pair tallied below: the
157.3 TFLOPS fp32 vector peak, which needs packed fp32 (v_pk_fma_f32), and half of it, 78.6 TFLOPS, the rate of the scalar fp32
instructions (v_fma_f32) these kernels issue.  Prints a table and one JSON line per case.

    python tools/interaction_bench.py [--iters 10] [--cases hand64 hand256 spheres]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))

PEAK_FP32 = 157.3e12                 # packed fp32
SCALAR_FP32 = PEAK_FP32 / 2          # one v_fma_f32 per lane per cycle
# FLOPs per point-triangle pair, an fma counted as 2, as the kernels spell them out
WINDING_FLOPS = dict(relative=9, lengths=3 * 5 + 3, cross=3 * 3, det=5, dots=3 * 5, den=7, atan2=30, accumulate=1)
DISTANCE_FLOPS = dict(relative=9, edges=6, d1_to_d6=6 * 5, va_vb_vc=3 * 3, regions=20, divisions=4 * 5, closest=3 * 4, norm=5, min=1)


def _events(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def _hand_object(res):
    import torch
    from honerf_amd import synth
    from honerf_amd.interaction import hand_object_meshes
    from honerf_amd.renderer import NeuSRenderer_fitting
    from helpers import product_modules
    m = product_modules()
    dual = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)
    bt, tp, j = synth.synth_hand_pose(3)
    c = j[9]
    R, tt = synth.synth_obj_pose(2, center=tuple(c))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return hand_object_meshes(dual, t(j.min(0) - 0.08), t(j.max(0) + 0.08), t(c - 0.35), t(c + 0.35), res, bt, tp,
                              t(R).T.contiguous(), t(tt))


def _spheres():
    import torch
    from test_interaction_cpu import mc_sphere
    h = mc_sphere((0.0, 0.0, 0.9), 0.05, 96)[:2]
    o = mc_sphere((0.08, 0.0, 0.9), 0.06, 96)[:2]
    dev = lambda m: (torch.from_numpy(m[0]).cuda(), torch.from_numpy(m[1]).cuda())
    return dev(h), dev(o)


def run_case(name, hand, obj, iters):
    import torch
    from honerf_amd import interaction as it
    (hv, ht), (ov, ot) = hand, obj
    vox = it.voxelize_surface(obj, 0.005)
    lo, hi = hv.amin(0), hv.amax(0)
    live_vox = int(((vox >= lo) & (vox <= hi)).all(1).sum())
    hin = it.contains(obj, hv)
    inner = hv[hin]
    wf, df = sum(WINDING_FLOPS.values()), sum(DISTANCE_FLOPS.values())
    rows = []

    def add(call, seconds, pairs, flops_per_pair):
        rows.append(dict(call=call, call_ms=seconds * 1e3, pairs=pairs, pairs_per_s=pairs / seconds if pairs else 0.0,
                         peak_share=pairs * flops_per_pair / seconds / PEAK_FP32 if pairs else 0.0,
                         scalar_share=pairs * flops_per_pair / seconds / SCALAR_FP32 if pairs else 0.0))
    add('voxelize obj (%d tris -> %d points)' % (len(ot), len(vox)), _events(lambda: it.voxelize_surface(obj, 0.005), iters), 0, 0)
    add('contains hand <- obj voxels (%d x %d)' % (len(vox), len(ht)), _events(lambda: it.contains(hand, vox), iters), live_vox * len(ht), wf)
    add('contains obj <- hand verts (%d x %d)' % (len(hv), len(ot)), _events(lambda: it.contains(obj, hv), iters), len(hv) * len(ot), wf)
    add('distance obj <- inner hand verts (%d x %d)' % (len(inner), len(ot)), _events(lambda: it.closest_distance(obj, inner), iters),
        len(inner) * len(ot), df)
    add('interaction_metrics', _events(lambda: it.interaction_metrics(hand, obj), iters), 0, 0)
    print('== %s: hand %d verts / %d tris, object %d verts / %d tris' % (name, len(hv), len(ht), len(ov), len(ot)))
    for r in rows:
        print('  %-48s %9.3f ms (call)  %10.3e pairs/s  %5.1f %% of 157.3 TF, %5.1f %% of 78.6 TF (scalar fp32)'
              % (r['call'], r['call_ms'], r['pairs_per_s'], 100 * r['peak_share'], 100 * r['scalar_share']))
    print(json.dumps(dict(case=name, winding_flops_per_pair=wf, distance_flops_per_pair=df, rows=rows)))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--cases', nargs='+', default=['hand64', 'hand256', 'spheres'])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('interaction_bench: no GPU (the timings are device events)')
    for c in args.cases:
        if c == 'spheres':
            h, o = _spheres()
        else:
            h, o = _hand_object(int(c[4:]))
        run_case(c, h, o, args.iters)
    return 0


if __name__ == '__main__':
    sys.exit(main())
