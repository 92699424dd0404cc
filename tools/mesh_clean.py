"""Drops floaters from a tree of exported meshes: the connected components of every PLY file (honerf_amd.mesh_components, on the current
GPU), the ones that pass the criteria written to the same relative path under DST.

Walks SRC for *.ply -- the `mesh_<fit_type>/<cid>_hand.ply`, `<cid>_obj.ply` layout get_res.py writes and tools/interaction_eval.py
reads -- reads each with honerf_amd.harness.read_ply, keeps the components that pass every given criterion (they combine with AND; none
given: --largest 1) and writes the kept part with harness.write_ply.  DST/mesh_clean.json lists, per file, the component table before
(label, faces, vertices, area, volume, closed, bounds) and the component indices kept.  tools/interaction_eval.py then runs on DST
unchanged.  Components are vertex-connected: faces that share a vertex index (trimesh's split joins over shared edges; the two differ
only at pinch vertices).

    python tools/mesh_clean.py SRC DST [--largest K] [--min-faces N] [--min-area-fraction F] [--closed-only]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('src', metavar='SRC', help='a tree of PLY files')
    ap.add_argument('dst', metavar='DST', help='where the kept parts go, same relative paths')
    ap.add_argument('--largest', type=int, default=None, metavar='K', help='the K components with the most faces')
    ap.add_argument('--min-faces', type=int, default=None, metavar='N', help='components of at least N faces')
    ap.add_argument('--min-area-fraction', type=float, default=None, metavar='F', help="components of at least F of the mesh's area")
    ap.add_argument('--closed-only', action='store_true', help='closed components only')
    args = ap.parse_args()
    crit = dict(largest=args.largest, min_faces=args.min_faces, min_area_fraction=args.min_area_fraction, closed_only=args.closed_only)
    if all(v is None or v is False for v in crit.values()):
        crit['largest'] = 1
    from honerf_amd import harness, mesh_components
    report = {'criteria': crit, 'files': {}}
    for dirpath, dirnames, files in os.walk(args.src):
        dirnames.sort()
        for name in sorted(files):
            if not name.endswith('.ply'):
                continue
            src = os.path.join(dirpath, name)
            rel = os.path.relpath(src, args.src)
            mesh = harness.read_ply(src)
            comps = mesh_components.components(mesh)
            meas = mesh_components.measure(mesh, comps)
            v, t, info = mesh_components.keep(mesh, comps, **crit)
            dst = os.path.join(args.dst, rel)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            harness.write_ply(dst, v, t)
            table = {k: meas[k].cpu().tolist() for k in mesh_components.MEASURES}
            table['label'] = comps['label'].cpu().tolist()
            report['files'][rel] = dict(vertices=int(mesh[0].shape[0]), faces=int(mesh[1].shape[0]), components=table, kept=info['kept'].cpu().tolist(),
                                        kept_vertices=int(v.shape[0]), kept_faces=int(t.shape[0]))
            print('%s: %d components, kept %s: %d -> %d faces' % (rel, comps['n'], info['kept'].cpu().tolist(), mesh[1].shape[0], t.shape[0]))
    os.makedirs(args.dst, exist_ok=True)
    with open(os.path.join(args.dst, 'mesh_clean.json'), 'w') as fh:
        json.dump(report, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
