"""Times the mesh components kernels (hn_meshcc.hip through honerf_amd.mesh_components) against the same labels from torch operators and
from the host.

Meshes: the synthetic hand and object of tools/mesh_cast_bench.py (interaction.hand_object_meshes, native mesher) at 64^3 and 256^3,
and a three-blob SDF volume (min of three sphere distances over [-1, 1]^3) meshed at 256^3 by mesh.marching_cubes.

Arms, alternating in one process per mesh, after `--warmup` untimed rounds; min / median / max over `--runs`:
  native_labels   mesh_components.components: the lock-free union-find, flatten, rank (device events)
  native_all      components + measure + keep(largest=1) (device events)
  torch_labels    the same vertex labels from torch operators on the device: min-label propagation over the faces with
                  scatter_reduce_('amin') plus pointer jumping (label = label[label]), to a fixpoint checked on the host every round
                  (device events; the number of rounds is recorded)
  host_labels     the mesh copied to the host, labelled there (scipy.sparse.csgraph.connected_components when scipy imports, else the
                  sequential numpy union-find of tests/meshcc_cases.py) and the labels copied back (wall clock, `--host-runs` runs)
The arms' vertex labels are compared for equality in the same run.  Writes one JSON line to `--out` as well.  Needs a GPU.

    python tools/mesh_components_bench.py [--res 64 256] [--blob-res 256] [--runs 7] [--warmup 2] [--out profiles/meshcc/mesh_components_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

BLOBS = ((-0.45, 0.0, 0.0, 0.4), (0.5, 0.1, 0.0, 0.3), (0.0, 0.7, 0.7, 0.12))


def blob_mesh(res, dev):
    from honerf_amd.mesh import marching_cubes
    ax = torch.linspace(-1.0, 1.0, res, dtype=torch.float64, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
    d = torch.stack([torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r for cx, cy, cz, r in BLOBS]).amin(0)
    return marching_cubes(d.to(torch.float32).contiguous(), 0.0)


def torch_labels(v, t):
    """Min-label propagation with pointer jumping -> (vertex_label int64 [V], -1 where unused; rounds)."""
    V = v.shape[0]
    label = torch.arange(V, dtype=torch.int64, device=t.device)
    flat = t.reshape(-1)
    rounds = 0
    while True:
        rounds += 1
        m = label[t].amin(1)
        new = label.clone().scatter_reduce_(0, flat, m.repeat_interleave(3), 'amin')
        new = new[new]
        if bool((new == label).all()):          # the host check of the fixpoint
            break
        label = new
    used = torch.zeros(V, dtype=torch.bool, device=t.device)
    used[flat] = True
    return torch.where(used, label, torch.full_like(label, -1)), rounds


def host_labels(v, t):
    """The mesh to the host, labelled there, the labels back on the device -> (vertex_label int64 [V], which labeller)."""
    tn = t.cpu().numpy()
    V = v.shape[0]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        e = np.concatenate([tn[:, [0, 1]], tn[:, [1, 2]]])
        n, comp = connected_components(coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(V, V)), directed=False)
        smallest = np.full(n, V, np.int64)
        np.minimum.at(smallest, comp, np.arange(V))
        lab = smallest[comp]
        used = np.zeros(V, bool)
        used[tn.reshape(-1)] = True
        lab[~used] = -1
        how = 'scipy'
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from meshcc_cases import np_components
        lab = np_components(tn, V)['vertex_label'].astype(np.int64)
        how = 'numpy union-find'
    return torch.from_numpy(lab).to(t.device), how


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def stats(t):
    return dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), ms_all=t)


def bench(name, v, t, args):
    from honerf_amd import mesh_components as mc
    v, t = v.contiguous(), t.contiguous()

    def native_all():
        comps = mc.components((v, t))
        return comps, mc.measure((v, t), comps), mc.keep((v, t), comps, largest=1)
    arms = {'native_labels': lambda: mc.components((v, t)), 'native_all': native_all, 'torch_labels': lambda: torch_labels(v, t)}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times, last = {k: [] for k in arms}, {}
    for _ in range(args.runs):
        for k, fn in arms.items():
            ms, last[k] = timed(fn)
            times[k].append(ms)
    host_ms = []
    for _ in range(args.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host, how = host_labels(v, t)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    native = last['native_labels']['vertex_label'].long()
    same_torch = bool(torch.equal(native, last['torch_labels'][0]))
    same_host = bool(torch.equal(native, host))
    comps, meas, kept = last['native_all']
    row = dict(vertices=int(v.shape[0]), triangles=int(t.shape[0]), components=int(comps['n']), largest_faces=int(meas['faces'].max()) if comps['n'] else 0,
               closed_components=int(meas['closed'].sum()), kept_faces=int(kept[1].shape[0]), torch_rounds=int(last['torch_labels'][1]), host_labeller=how,
               labels_equal_torch=same_torch, labels_equal_host=same_host, host_labels=stats(host_ms), **{k: stats(x) for k, x in times.items()})
    row['torch_over_native_labels'] = row['torch_labels']['ms_median'] / row['native_labels']['ms_median']
    row['host_over_native_labels'] = row['host_labels']['ms_median'] / row['native_labels']['ms_median']
    print('%-14s %8d triangles %6d components | native labels %8.3f ms, all %8.3f ms | torch labels %9.3f ms (%d rounds) | host (%s) %9.1f ms | equal %s %s'
          % (name, row['triangles'], row['components'], row['native_labels']['ms_median'], row['native_all']['ms_median'], row['torch_labels']['ms_median'],
             row['torch_rounds'], how, row['host_labels']['ms_median'], same_torch, same_host), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--res', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--blob-res', type=int, default=256)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--host-runs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'meshcc', 'mesh_components_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_components_bench: no GPU')
    import mesh_cast_bench
    dev = torch.device('cuda')
    sc = mesh_cast_bench.scene(dev)
    rows = {}
    for res in args.res:
        hand, obj = mesh_cast_bench.meshes(*sc, res)
        rows['hand_res%d' % res] = bench('hand_res%d' % res, hand[0], hand[1], args)
        rows['obj_res%d' % res] = bench('obj_res%d' % res, obj[0], obj[1], args)
    bv, bt = blob_mesh(args.blob_res, dev)
    rows['blobs_res%d' % args.blob_res] = bench('blobs_res%d' % args.blob_res, bv, bt, args)
    line = json.dumps(dict(tool='mesh_components_bench', device=torch.cuda.get_device_name(0), runs=args.runs, host_runs=args.host_runs, warmup=args.warmup,
                           timing='device events around each arm (host_labels: wall clock with the copies), arms alternating in one process',
                           all_labels_equal=all(r['labels_equal_torch'] and r['labels_equal_host'] for r in rows.values()), rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
