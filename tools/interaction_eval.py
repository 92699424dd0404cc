"""analys_results/analys_interaction.py without trimesh: the per-class interaction volume and penetration depth of fitted frames.

Walks BASE/{1,12}/<seq>/<frame>/mesh_{1,12}/<id>_{hand,obj}.ply as the reference does (a frame counts when its fit-1 hand mesh
exists), scores every pair with honerf_amd.interaction.interaction_metrics on the current GPU and prints the reference's lines:
    object class <class> has <n> frames
    fit1_int_sum: .., fit1_dep_sum: .., fit12_int_sum: .., fit12_dep_sum: ..      (means: cm^3, mm)
A class without frames prints its 0-frame line only.  The meshes are read with honerf_amd.harness.read_ply, which reads the binary
little-endian float32 files that harness.write_ply (get_res.py through extract_geometry(..., mesher='native')) writes, not every PLY
(not trimesh's float64 exports, for one).  Unlike the reference, no pickle cache is read or written.

    python tools/interaction_eval.py BASE [--classes bean box cup meat] [--pitch 0.005]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ['bean', 'box', 'cup', 'meat']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('base', help="the reference's ./fit_res/analys_res/view_8")
    ap.add_argument('--classes', nargs='+', default=CLASSES)
    ap.add_argument('--pitch', type=float, default=0.005)
    ap.add_argument('--max-frame', type=int, default=2000, help='frame ids 0 .. max-1 are looked for (the reference: 2000)')
    args = ap.parse_args()
    from honerf_amd import harness
    from honerf_amd.interaction import interaction_metrics

    def score(hand_path, obj_path):
        m = interaction_metrics(harness.read_ply(hand_path), harness.read_ply(obj_path), pitch=args.pitch)
        return m['int_vol'], m['pen_dep']

    sub_path = os.path.join(args.base, '1')
    for cur_class in args.classes:
        sums = [0.0, 0.0, 0.0, 0.0]
        cid = 0
        for obj_name in sorted(os.listdir(sub_path)) if os.path.isdir(sub_path) else []:
            if cur_class not in obj_name:
                continue
            obj_path = os.path.join(sub_path, obj_name)
            for frame_name in sorted(os.listdir(obj_path)):
                frame_path = os.path.join(obj_path, frame_name)
                for frame_id in range(args.max_frame):
                    first_hand = os.path.join(frame_path, 'mesh_1', '%d_hand.ply' % frame_id)
                    if not os.path.exists(first_hand):
                        continue
                    first_obj = os.path.join(frame_path, 'mesh_1', '%d_obj.ply' % frame_id)
                    second = os.path.join(args.base, '12', obj_name, frame_name, 'mesh_12')
                    fi, fd = score(first_hand, first_obj)
                    si, sd = score(os.path.join(second, '%d_hand.ply' % frame_id), os.path.join(second, '%d_obj.ply' % frame_id))
                    for k, x in enumerate((fi, fd, si, sd)):
                        sums[k] += x
                    cid += 1
        print('object class %s has %d frames' % (cur_class, cid))
        if cid:
            print('fit1_int_sum: %.2lf, fit1_dep_sum: %.2lf, fit12_int_sum: %.2lf, fit12_dep_sum: %.2lf' % tuple(s / cid for s in sums))
    return 0


if __name__ == '__main__':
    sys.exit(main())
