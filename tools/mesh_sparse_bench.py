"""Times extract_geometry(..., mesher='sparse') (hn_mcubes_sparse.hip, honerf_amd.mesh.marching_cubes_sparse) against mesher='native'.

1. The synthetic object field (NeuSRenderer) and hand field (NeuSRenderer_fitting) at 256^3 and 512^3: the 'native' call, then the
   'sparse' call for lipschitz 0, 1, 2 and block 4, 8 in the same run: time (device events around the whole call, median of 5),
   evaluated / dense_points, grow rounds, and whether the two meshes are equal.
2. The largest finite-difference gradient norm of each field on its 256^3 grid: the evidence there is for a lipschitz value.
3. One 1024^3 sparse extraction per field (no dense counterpart: hn_mcubes refuses the grid): time, V / T, peak memory.

Usage: python tools/mesh_sparse_bench.py [--reps 5] [--res 256 512] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_bench import renderers  # noqa: E402


def timed(fn, reps):
    """Median over reps of the device time of fn() (which ends with its copies to the host), and its last result."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def field_calls(field):
    """-> geo(res, **kw): extract_geometry of the field, vol(res): its dense device volume, box (bmin, bmax)."""
    from honerf_amd import synth
    single, dual = renderers()
    if field == 'obj':
        bmin, bmax = torch.tensor([-0.6, -0.5, -0.55]), torch.tensor([0.6, 0.55, 0.5])
        return (lambda res, **kw: single.extract_geometry(bmin, bmax, res, None, None, None, None, **kw),
                lambda res: single._volume(bmin, bmax, res), (bmin, bmax))
    bt, tp, j = synth.synth_hand_pose(3)
    bmin, bmax = torch.from_numpy(j.min(0) - 0.08), torch.from_numpy(j.max(0) + 0.08)
    return (lambda res, **kw: dual.extract_geometry(bmin, bmax, res, bt, tp, None, None, 'hand', **kw),
            lambda res: dual._volume(bmin, bmax, res, bt, tp, None, None, 'hand'), (bmin, bmax))


def gradient_norm(vol, box, res):
    """Largest central-difference gradient norm of the volume, in world units: everywhere, and within 4 voxels of the level set."""
    h = [float(x) for x in ((box[1] - box[0]).double() / (res - 1.0))]
    gx, gy, gz = torch.gradient(vol, spacing=h)
    n = torch.sqrt(gx * gx + gy * gy + gz * gz)
    near = n[vol.abs() < 4 * max(h)]
    return float(n.max()), float(near.max()) if near.numel() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--res', type=int, nargs='*', default=[256, 512])
    ap.add_argument('--no-1024', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_sparse_bench needs a GPU')
    rows = []
    for field in ('obj', 'hand'):
        geo, vol, box = field_calls(field)
        geo(64, mesher='native')
        geo(64, mesher='sparse')
        g_all, g_near = gradient_norm(vol(256), box, 256)
        rows.append(dict(kind='gradient', field=field, res=256, max_norm=g_all, max_norm_near_surface=g_near))
        print('%-4s 256^3: central-difference |grad| max %.3f, within 4 voxels of the level set %.3f' % (field, g_all, g_near), flush=True)
        for res in a.res:
            ms_native, native = timed(lambda: geo(res, mesher='native'), a.reps)
            print('%-4s %4d^3 native: %.2f ms, V %d T %d' % (field, res, ms_native, len(native[0]), len(native[1])), flush=True)
            for block in (4, 8):
                for lip in (0.0, 1.0, 2.0):
                    ms, (v, t, info) = timed(lambda: geo(res, mesher='sparse', block=block, lipschitz=lip, return_info=True), a.reps)
                    equal = bool(np.array_equal(v, native[0]) and np.array_equal(t, native[1]))
                    rows.append(dict(kind='sparse', field=field, res=res, block=block, lipschitz=lip, ms_sparse=ms, ms_native=ms_native,
                                     n_verts=len(v), n_tris=len(t), equal=equal, **info))
                    print('%-4s %4d^3 b %d lipschitz %g: sparse %.2f ms, native %.2f ms (x%.1f) | evaluated %.1f %% | active %d -> %d '
                          'of %d, %d grow rounds, leaks left %d | equal %s'
                          % (field, res, block, lip, ms, ms_native, ms_native / ms, 100.0 * info['evaluated'] / info['dense_points'],
                             info['active_initial'], info['active'], info['blocks'], info['grow_rounds'], info['leaks_left'], equal),
                          flush=True)
            del native
            torch.cuda.empty_cache()
        if not a.no_1024:
            torch.cuda.reset_peak_memory_stats()
            ms, (v, t, info) = timed(lambda: geo(1024, mesher='sparse', return_info=True), 1)
            peak = torch.cuda.max_memory_allocated() / 2 ** 20
            rows.append(dict(kind='sparse-1024', field=field, res=1024, block=8, lipschitz=1.0, ms_sparse=ms, n_verts=len(v), n_tris=len(t),
                             peak_MB=peak, **info))
            print('%-4s 1024^3 b 8 lipschitz 1: sparse %.1f ms, V %d T %d | evaluated %.2f %% | active %d -> %d of %d, %d grow rounds, '
                  'leaks left %d | peak memory %.0f MB' % (field, ms, len(v), len(t), 100.0 * info['evaluated'] / info['dense_points'],
                                                           info['active_initial'], info['active'], info['blocks'], info['grow_rounds'],
                                                           info['leaks_left'], peak), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
