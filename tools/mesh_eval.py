"""Surface distances of predicted meshes against ground-truth meshes: Chamfer, accuracy / completeness, F-score, Hausdorff, normals.

Walks PRED (a directory of .ply files) and pairs every file with the file of the same name in GT (a directory), or with GT itself when
it is a single .ply (one CAD model or scan for every prediction).  Every pair is scored with honerf_amd.mesh_distance.surface_metrics on
the current GPU; one row per pair and the mean row are printed, distances x 1000 and labelled mm (the meshes of a run are in metres),
Chamfer-L2 x 1e6 mm^2.  The meshes are read with honerf_amd.harness.read_ply, which reads the binary little-endian float32 files that
harness.write_ply writes, not every PLY.  --clean keeps each mesh's largest component first (honerf_amd.mesh_components.largest: the
floaters of an extraction would otherwise own the Hausdorff distance).  --align icp (rigid) or icp+scale (similarity) moves every
prediction onto its ground truth by ICP first (honerf_amd.alignment.icp), so that a global pose offset stops dominating a shape score; the
rows then carry the transform and the ICP's RMS trace.  --json writes the rows, in the meshes' own units, to a file.

    python tools/mesh_eval.py PRED GT [--clean] [--align icp] [--n 100000] [--tau 0.005 --tau 0.010] [--seed 0] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred', help='a directory of predicted .ply files')
    ap.add_argument('gt', help='a directory of ground-truth .ply files with the same names, or one .ply for all')
    ap.add_argument('--clean', action='store_true', help="score each mesh's largest component")
    ap.add_argument('--align', choices=['icp', 'icp+scale'], default=None, help='align each prediction to its ground truth by ICP before scoring')
    ap.add_argument('--n', type=int, default=100000, help='samples per mesh')
    ap.add_argument('--tau', type=float, action='append', default=None, help='an F-score threshold in mesh units (repeatable; 0.005 and 0.010)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--json', default=None, help='write the rows and the mean to this file')
    args = ap.parse_args()
    taus = args.tau or [0.005, 0.010]
    from honerf_amd import harness
    from honerf_amd.mesh_distance import surface_metrics

    def load(path):
        m = harness.read_ply(path)
        if args.clean:
            from honerf_amd.mesh_components import largest
            m = largest(m)
        return m

    names = sorted(f for f in os.listdir(args.pred) if f.endswith('.ply'))
    one_gt = load(args.gt) if os.path.isfile(args.gt) else None
    rows = []
    for name in names:
        gt_path = args.gt if one_gt is not None else os.path.join(args.gt, name)
        if one_gt is None and not os.path.exists(gt_path):
            print('%s: no ground truth %s, skipped' % (name, gt_path), file=sys.stderr)
            continue
        m = surface_metrics(load(os.path.join(args.pred, name)), one_gt if one_gt is not None else load(gt_path), n=args.n, taus=taus,
                            seed=args.seed, align=args.align)
        rows.append(dict(name=name, **m))
    keys = [k for k in (rows[0] if rows else {}) if k not in ('name', 'transform', 'icp_rms')]
    mean = {k: sum(r[k] for r in rows) / len(rows) for k in keys}
    cols = ['chamfer_l1', 'accuracy', 'completeness', 'hausdorff'] + ['fscore@%g' % t for t in taus] + ['normal_consistency']
    head = ['chamfer-L1 mm', 'accuracy mm', 'complete. mm', 'hausdorff mm'] + ['F@%gmm %%' % (t * 1000) for t in taus] + ['normal cons.']

    def cell(k, v):
        return '%.3f' % (v * 1000 if k in ('chamfer_l1', 'accuracy', 'completeness', 'hausdorff') else v * 100 if k.startswith('fscore') else v)
    print('%-32s' % 'mesh' + ''.join('%15s' % h for h in head))
    for r in rows + ([dict(name='mean of %d' % len(rows), **mean)] if rows else []):
        print('%-32s' % r['name'] + ''.join('%15s' % cell(k, r[k]) for k in cols))
    if not rows:
        print('no pairs found')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(dict(pred=args.pred, gt=args.gt, n=args.n, taus=taus, seed=args.seed, clean=args.clean, align=args.align, rows=rows, mean=mean), f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
