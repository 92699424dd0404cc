"""Times the device marching cubes (hn_mcubes.hip, honerf_amd.mesh).

1. The mesher's kernels alone on an analytic sphere volume (r = 0.3 in [-0.5, 0.5]^3) at 128^3, 256^3 and 512^3: count + scan
   and vertices + triangles, device events around launches on pre-sized buffers.  Reported as ms, as GB/s of volume bytes read
   (4 n per read), and as a share of the 6.3 TB/s measured copy rate for the bytes the four passes move (modelled below).
2. The whole extract_geometry(..., mesher='native') of the object field (NeuSRenderer) and the hand field (NeuSRenderer_fitting)
   at 64^3 and 256^3, split into the volume (hn_field_sdf) and the mesher (including the 16-byte read-back of the totals and the
   copies of the mesh to the host).

Usage: python tools/mesh_bench.py [--iters 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_TBPS = 6.3   # MI355X float4 copy rate, measured (MI355X_MICROARCH.md)


def sphere(res, dev):
    ax = torch.linspace(-0.5, 0.5, res, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
    return (torch.sqrt(x * x + y * y + z * z) - 0.3).contiguous()


def time_events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernels_alone(res, iters):
    from honerf_amd import lib as L
    lib = L.load()
    dev = torch.device('cuda')
    vol = sphere(res, dev)
    n = res ** 3
    ws = torch.empty(lib.hn_mcubes_workspace_bytes(res, res, res), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)

    def count():
        L.check(lib.hn_mcubes_count(L.ptr(vol), res, res, res, 0.0, L.ptr(totals), L.ptr(ws), ws.numel(), L.stream_ptr()), 'count')
    count()
    V, T = totals.tolist()
    verts = torch.empty(V, 3, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int64, device=dev)

    def emit():
        L.check(lib.hn_mcubes_emit(L.ptr(vol), res, res, res, 0.0, L.ptr(ws), ws.numel(), V, T, L.ptr(verts), L.ptr(tris),
                                   L.stream_ptr()), 'emit')

    def both():
        count()
        emit()
    for _ in range(3):
        both()
    torch.cuda.synchronize()
    t_count = time_events(count, iters)
    t_emit = time_events(emit, iters)
    t_all = time_events(both, iters)
    # bytes: the volume read by count and by the vertex pass; int32 vertex base + flag byte written by the vertex pass and read by
    # the triangle pass; vertices (12 B) and triangles (24 B) written
    moved = 8 * n + 2 * 5 * n + 12 * V + 24 * T
    return dict(res=res, n_verts=V, n_tris=T, ms_count_scan=t_count, ms_verts_tris=t_emit, ms_total=t_all,
                volume_GBps=4 * n / (t_all * 1e-3) / 1e9, modelled_bytes=moved,
                modelled_TBps=moved / (t_all * 1e-3) / 1e12, share_of_copy=moved / (t_all * 1e-3) / 1e12 / COPY_TBPS,
                ms_at_copy_rate=moved / (COPY_TBPS * 1e12) * 1e3)


def renderers():
    from honerf_amd import nets
    from honerf_amd.renderer import NeuSRenderer, NeuSRenderer_fitting
    dev = torch.device('cuda')
    m = {'sdf_obj': nets.SDFNetwork_OBJ(), 'color_obj': nets.RenderingNetwork_OBJ(), 'sdf_hand': nets.SDFNetwork(),
         'color_hand': nets.RenderingNetwork(use_gradients=True)}
    for k, s in (('sdf_obj', 11), ('color_obj', 12), ('sdf_hand', 21), ('color_hand', 22)):
        m[k].reset_parameters(s)
    m = {k: v.to(dev) for k, v in m.items()}
    m['var_obj'], m['var_hand'] = nets.SingleVarianceNetwork(0.3).to(dev), nets.SingleVarianceNetwork(0.27).to(dev)
    single = NeuSRenderer(m['sdf_obj'], m['var_obj'], m['color_obj'], 'obj', 32, 0, 0, 4, 1.0)
    dual = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'],
                                64, 64, 0, 4, 1.0)
    return single, dual


def extract(field, res, reps):
    from honerf_amd import synth
    from honerf_amd.mesh import marching_cubes
    single, dual = renderers()
    if field == 'obj':
        bmin, bmax = torch.tensor([-0.6, -0.5, -0.55]), torch.tensor([0.6, 0.55, 0.5])
        vol_fn = lambda: single._volume(bmin, bmax, res)
        geo_fn = lambda: single.extract_geometry(bmin, bmax, res, None, None, None, None, mesher='native')
    else:
        bt, tp, j = synth.synth_hand_pose(3)
        bmin, bmax = torch.from_numpy(j.min(0) - 0.08), torch.from_numpy(j.max(0) + 0.08)
        vol_fn = lambda: dual._volume(bmin, bmax, res, bt, tp, None, None, 'hand')
        geo_fn = lambda: dual.extract_geometry(bmin, bmax, res, bt, tp, None, None, 'hand', mesher='native')

    def mesh_host(u):
        v, t = marching_cubes(u, 0.0)
        return v.cpu().numpy(), t.cpu().numpy()
    u = vol_fn()
    mesh_host(u)
    geo_fn()
    torch.cuda.synchronize()
    tv, tm, tg = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        u = vol_fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        v, t = mesh_host(u)
        t2 = time.perf_counter()
        geo_fn()
        t3 = time.perf_counter()
        tv.append(t1 - t0)
        tm.append(t2 - t1)
        tg.append(t3 - t2)
    return dict(field=field, res=res, n_verts=len(v), n_tris=len(t), ms_volume=1e3 * float(np.median(tv)),
                ms_mesher=1e3 * float(np.median(tm)), ms_extract_geometry=1e3 * float(np.median(tg)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_bench needs a GPU')
    rows = []
    for res in (128, 256, 512):
        r = kernels_alone(res, a.iters)
        rows.append(dict(kind='kernels', **r))
        print('mesher kernels %4d^3: V %9d T %9d | count+scan %.3f ms, verts+tris %.3f ms, together %.3f ms | volume %.0f GB/s | '
              'modelled %.2f GB moved, %.2f TB/s = %.0f %% of %.1f TB/s (%.3f ms at that rate)'
              % (res, r['n_verts'], r['n_tris'], r['ms_count_scan'], r['ms_verts_tris'], r['ms_total'], r['volume_GBps'],
                 r['modelled_bytes'] / 1e9, r['modelled_TBps'], 100 * r['share_of_copy'], COPY_TBPS, r['ms_at_copy_rate']), flush=True)
        torch.cuda.empty_cache()
    for field in ('obj', 'hand'):
        for res in (64, 256):
            r = extract(field, res, a.reps)
            rows.append(dict(kind='extract_geometry', **r))
            print('extract_geometry %-4s %3d^3: V %8d T %8d | volume %.2f ms, mesher %.2f ms (incl. read-back), whole call %.2f ms'
                  % (field, res, r['n_verts'], r['n_tris'], r['ms_volume'], r['ms_mesher'], r['ms_extract_geometry']), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
