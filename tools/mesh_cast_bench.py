"""Times the mesh ray caster (hn_meshcast, ho-nerf_amd/csrc/hn_meshcast.hip) at one 512 x 334 view of the synthetic hand and object
(synth_hand_pose(3), the object posed at joint 9 in a +-0.35 m box; interaction.hand_object_meshes, native mesher) at 64^3 and 256^3.

Arms, alternating in one process, per mesh resolution and triangle order ('morton': sorted by the Morton code of the centroids;
'identity': the mesher's own order):
  cull      MeshCaster.cast(cull=True): groups and blocks whose bounds a ray misses are skipped
  no_cull   MeshCaster.cast(cull=False): every block of 64 triangles is walked by every workgroup
Device events around one cast per run; min / median / max over `--runs` alternating runs after `--warmup` untimed rounds.  The two
arms' outputs are compared bit for bit.  harness.render_view_buffers' time for the same view of the two fields is recorded beside
them, and the one-off costs: the Morton sort and hn_meshcast_prepare.  Writes one JSON line to `--out` as well.  Needs a GPU.

    python tools/mesh_cast_bench.py [--res 64 256] [--height 334] [--width 512] [--runs 7] [--warmup 2] [--out profiles/meshcast/mesh_cast_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEEDS = {'sdf_obj': 11, 'color_obj': 12, 'sdf_hand': 21, 'color_hand': 22}
VAR_OBJ, VAR_HAND = 0.3, 0.27
NEAR, FAR = 0.4, 1.5


def scene(dev):
    """The synthetic two-field renderer and its pose: (renderer, bt_inv, T_pose, joints, R_obj, t_obj)."""
    from honerf_amd import nets, synth
    from honerf_amd.renderer import NeuSRenderer_fitting
    m = {'sdf_obj': nets.SDFNetwork_OBJ(), 'color_obj': nets.RenderingNetwork_OBJ(), 'sdf_hand': nets.SDFNetwork(),
         'color_hand': nets.RenderingNetwork(use_gradients=True), 'var_obj': nets.SingleVarianceNetwork(VAR_OBJ),
         'var_hand': nets.SingleVarianceNetwork(VAR_HAND)}
    for k, s in SEEDS.items():
        m[k].reset_parameters(s)
    m = {k: v.to(dev) for k, v in m.items()}
    ren = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)
    bt_inv, T_pose, joints = synth.synth_hand_pose(3)
    R_obj, t_obj = synth.synth_obj_pose(2, center=tuple(joints[9]))
    return ren, bt_inv, T_pose, joints, R_obj, t_obj


def meshes(ren, bt_inv, T_pose, joints, R_obj, t_obj, res):
    from honerf_amd.interaction import hand_object_meshes
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    c = joints[9]
    return hand_object_meshes(ren, t(joints.min(0) - 0.08), t(joints.max(0) + 0.08), t(c - 0.35), t(c + 0.35), res, bt_inv, T_pose,
                              t(R_obj).T.contiguous(), t(t_obj))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def stats(t):
    return dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), ms_all=t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--res', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--height', type=int, default=334)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--radius', type=float, default=0.9)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'meshcast', 'mesh_cast_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_cast_bench: no GPU')
    from honerf_amd import harness, synth
    from honerf_amd.meshcast import MeshCaster, morton_order
    dev = torch.device('cuda')
    ren, bt_inv, T_pose, joints, R_obj, t_obj = scene(dev)
    cams = synth.ring_cameras(1, radius=args.radius, target=tuple(float(c) for c in joints[9]), seed=3)
    H, W = args.height, args.width
    rays_o, rays_d = harness.image_rays(cams, H, W, dev)
    rows = {}
    for res in args.res:
        hand, obj = meshes(ren, bt_inv, T_pose, joints, R_obj, t_obj, res)
        n_tris = int(hand[1].shape[0] + obj[1].shape[0])
        for order in ('morton', 'identity'):
            ms_build, caster = timed(lambda: MeshCaster([hand, obj], order=order))
            arms = {'cull': lambda: caster.cast(rays_o, rays_d, NEAR, FAR, cull=True), 'no_cull': lambda: caster.cast(rays_o, rays_d, NEAR, FAR, cull=False)}
            for _ in range(args.warmup):
                for fn in arms.values():
                    fn()
            torch.cuda.synchronize()
            times, last = {k: [] for k in arms}, {}
            for _ in range(args.runs):
                for name, fn in arms.items():
                    ms, last[name] = timed(fn)
                    times[name].append(ms)
            same = all(torch.equal(last['cull'][k], last['no_cull'][k]) for k in last['cull'])
            key = 'res%d_%s' % (res, order)
            rows[key] = dict(resolution=res, order=order, triangles=n_tris, rays=H * W, hit_rays=int(last['cull']['hit'].sum()), same_bits=bool(same),
                             caster_build_ms=ms_build, cull=stats(times['cull']), no_cull=stats(times['no_cull']),
                             no_cull_over_cull=float(np.median(times['no_cull']) / np.median(times['cull'])))
            print('%-16s %7d triangles x %d rays | cull: min %9.3f median %9.3f max %9.3f ms | no_cull: min %9.3f median %9.3f max %9.3f ms | same bits %s'
                  % (key, n_tris, H * W, min(times['cull']), float(np.median(times['cull'])), max(times['cull']), min(times['no_cull']),
                     float(np.median(times['no_cull'])), max(times['no_cull']), same), flush=True)
            if order == 'morton':
                rows[key]['morton_sort_ms'] = stats([timed(lambda: morton_order(caster.vertices[caster.triangles].reshape(-1, 9)))[0] for _ in range(5)])
            del caster
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    field = lambda: harness.render_view_buffers(ren, cams, H, W, NEAR, FAR, t(bt_inv), t(T_pose), t(R_obj), t(t_obj))
    field()
    torch.cuda.synchronize()
    field_ms = [timed(field)[0] for _ in range(3)]
    print('render_view_buffers, the same view of the two fields: min %.1f median %.1f max %.1f ms' % (min(field_ms), float(np.median(field_ms)), max(field_ms)))
    line = json.dumps(dict(tool='mesh_cast_bench', device=torch.cuda.get_device_name(0), height=H, width=W, near=NEAR, far=FAR, runs=args.runs,
                           warmup=args.warmup, rows=rows, render_view_buffers=stats(field_ms)))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
