"""The synthetic two-field scene of tools/view_buffers.py (same fields, pose, cameras and rays) as MESHES in the camera: the hand and
object meshes of interaction.hand_object_meshes (native mesher) cast through harness.render_mesh_buffers, next to the field's own
buffers from harness.render_view_buffers.  Writes, per view, `<out>/view<k>_mesh_depth.pgm` (16-bit, millimetres, 0 = nothing),
`_mesh_normal.ppm` (camera frame, (n / 2 + 1 / 2) 255) and `_mesh_label.pgm` (0 nothing, 1 hand, 2 object) beside the field's
`_color.ppm`, `_depth.pgm`, `_normal.ppm`, `_label.pgm`, and `--report` (profiles/meshcast/mesh_vs_volume.json): per view the
intersection over union of the hand and of the object label between the two, and the median and 95th percentile of
|depth_mesh - depth_field| over the pixels both label the same (not 0).  These numbers are RECORDED, not asserted: the synthetic
networks are random-initialised with inv_s about 20, so the field's depth is a soft average along the ray, not its zero level set.
Needs a GPU.

    python tools/mesh_views.py [--out view_buffers] [--views 4] [--height 96] [--width 128] [--resolution 64] [--threshold 0.5]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='view_buffers')
    ap.add_argument('--report', default=os.path.join(ROOT, 'profiles', 'meshcast', 'mesh_vs_volume.json'))
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--height', type=int, default=96)
    ap.add_argument('--width', type=int, default=128)
    ap.add_argument('--radius', type=float, default=0.6)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--threshold', type=float, default=0.5)
    ap.add_argument('--seed', type=int, default=13)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_views: no GPU')
    from honerf_amd import harness, nets, synth
    from honerf_amd.interaction import hand_object_meshes
    from honerf_amd.meshcast import MeshCaster
    from honerf_amd.renderer import NeuSRenderer_fitting
    dev = torch.device('cuda')
    m = {'sdf_obj': nets.SDFNetwork_OBJ(), 'color_obj': nets.RenderingNetwork_OBJ(), 'sdf_hand': nets.SDFNetwork(),
         'color_hand': nets.RenderingNetwork(use_gradients=True), 'var_obj': nets.SingleVarianceNetwork(VAR_OBJ),
         'var_hand': nets.SingleVarianceNetwork(VAR_HAND)}
    for k, s in SEEDS.items():
        m[k].reset_parameters(s)
    m = {k: v.to(dev) for k, v in m.items()}
    ren = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)
    bt_inv, T_pose, joints = synth.synth_hand_pose(args.seed)
    center = joints[9] + np.array([0.03, 0.0, 0.02], dtype=joints.dtype)
    R_obj, t_obj = synth.synth_obj_pose(args.seed + 3, center=tuple(center))
    cams = synth.ring_cameras(args.views, radius=args.radius, target=tuple(float(c) for c in joints[9]), seed=3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    H, W = args.height, args.width
    field = harness.render_view_buffers(ren, cams, H, W, NEAR, FAR, t(bt_inv).to(dev), t(T_pose).to(dev), t(R_obj).to(dev), t(t_obj).to(dev),
                                        opacity_threshold=args.threshold)
    hand, obj = hand_object_meshes(ren, t(joints.min(0) - 0.08), t(joints.max(0) + 0.08), t(center - 0.35), t(center + 0.35), args.resolution,
                                   bt_inv, T_pose, t(R_obj).T.contiguous(), t(t_obj))
    caster = MeshCaster([hand, obj])
    mesh = harness.render_mesh_buffers(caster, cams, H, W, NEAR, FAR)
    iou = {name: harness.label_iou(mesh['label'], field['label'], lab).tolist() for lab, name in ((1, 'hand'), (2, 'object'))}
    torch.cuda.synchronize()
    os.makedirs(args.out, exist_ok=True)
    views = []
    for v in range(args.views):
        stem = os.path.join(args.out, 'view%d' % v)
        harness.write_image(stem + '_color.ppm', field['color'][v])
        harness.write_depth(stem + '_depth.pgm', field['depth'][v])
        harness.write_image(stem + '_normal.ppm', field['normal'][v])
        harness.write_gray(stem + '_label.pgm', field['label'][v])
        harness.write_depth(stem + '_mesh_depth.pgm', mesh['depth'][v])
        harness.write_image(stem + '_mesh_normal.ppm', mesh['normal'][v])
        harness.write_gray(stem + '_mesh_label.pgm', mesh['label'][v])
        both = (mesh['label'][v] == field['label'][v]) & (mesh['label'][v] > 0)
        diff = (mesh['depth'][v] - field['depth'][v]).abs()[both].double()
        row = dict(view=v, label_iou_hand=iou['hand'][v], label_iou_object=iou['object'][v], pixels_labelled_the_same=int(both.sum()),
                   mesh_pixels=[int((mesh['label'][v] == i).sum()) for i in range(3)], field_pixels=[int((field['label'][v] == i).sum()) for i in range(3)],
                   depth_abs_diff_median_m=float(diff.median()) if diff.numel() else None,
                   depth_abs_diff_p95_m=float(torch.quantile(diff, 0.95)) if diff.numel() else None)
        views.append(row)
        print('%s: IoU hand %.3f object %.3f; |depth_mesh - depth_field| median %s p95 %s m over %d pixels'
              % (stem, row['label_iou_hand'], row['label_iou_object'], row['depth_abs_diff_median_m'], row['depth_abs_diff_p95_m'], row['pixels_labelled_the_same']))
    report = dict(tool='mesh_views', device=torch.cuda.get_device_name(0), height=H, width=W, near=NEAR, far=FAR, resolution=args.resolution,
                  opacity_threshold=args.threshold, triangles=[int(hand[1].shape[0]), int(obj[1].shape[0])], views=views)
    os.makedirs(os.path.dirname(os.path.abspath(args.report)), exist_ok=True)
    with open(args.report, 'w') as fh:
        json.dump(report, fh, indent=1)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
