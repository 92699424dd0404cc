"""analys_results/analys_hand_obj_pose.py and analys_acc_err.py on the device: the pose accuracy of fitted frames, per object class.

Walks BASE/view_<n>/<fit type>/<person>_<object>/<sequence>/pose_<fit type>/<id>.pickle as the reference does (the files
honerf_amd.fitting.pose_saver / harness.write_pose write; every file must hold the gt_* keys), scores every sequence with one batched
honerf_amd.pose_metrics.pose_metrics call on the current GPU and prints the reference's two lines per class:
    obj_name <class> has <n> frames
    init joint: .., ours joint: .., init ad: .., init add: .., init adds: .., ours ad: .., ours add: .., ours adds: ..
(joint and ad: mean, mm; add and adds: frames under 15 mm, %).  Without --init the init columns are left out; a class without frames
prints its first line only.  --aligned appends the Procrustes-aligned columns of the hand benchmarks (honerf_amd.pose_metrics.hand_metrics
on the joints): `pa joint` (PA-MPJPE, mm), `auc` and `pa auc` (the area under the PCK curve over 0 .. 50 mm, raw and aligned), per
method.  --init DIR holds the initial estimates as the reference reads them:
DIR/<person>_<object>/<sequence>/pred_joint3d_<n>view/<id>.pickle (key pred_joint_3d) and pred_objpose_<n>view/<id>.txt (a 4 x 4).

The object model of <object> is MODELS/<object>_cppose/<object>_ours.ply or .npy, its vertices times --model-scale (the reference's
models are in mm: 0.001).  A .ply is read with honerf_amd.harness.read_ply, which reads the binary little-endian float32 files
harness.write_ply writes, not every PLY; a .npy holds the vertices [V, 3].

--accel switches to analys_acc_err.py: for every sequence under BASE/view_<n>/1234 the frames 0 .. max-frame - 1 whose fit-12 pose
exists are read from 12/../pose_12, 123/../pose_4 and 1234/../pose_4, and the joint and vertex acceleration errors (mm) of the
three are printed, after the number of frames:
    acc_list_1_3_j: .., acc_list_1_3_v: .., acc_list_123_j: .., acc_list_123_v: .., acc_list_1234_j: .., acc_list_1234_v: ..

    python tools/pose_eval.py BASE --view-num 8 --fit-type 12 --models DIR [--init DIR] [--classes bean box cup meat] [--aligned] [--accel]
"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ['bean', 'box', 'cup', 'meat']


def load_model(models, obj, scale):
    from honerf_amd import harness
    stem = os.path.join(models, obj + '_cppose', obj + '_ours')
    if os.path.exists(stem + '.npy'):
        v = np.load(stem + '.npy')
    elif os.path.exists(stem + '.ply'):
        v = harness.read_ply(stem + '.ply')[0]
    else:
        raise FileNotFoundError('no object model %s.ply or .npy' % stem)
    return np.asarray(v, np.float64).reshape(-1, 3) * scale


def stack(poses, prefix):
    return {k: np.stack([np.asarray(p[prefix + k], np.float32) for p in poses]) for k in ('joint3d', 'Ro', 'To')}


def read_init(init, obj_name, frame_name, view_num, cid):
    with open(os.path.join(init, obj_name, frame_name, 'pred_joint3d_%sview' % view_num, cid + '.pickle'), 'rb') as f:
        joint = np.asarray(pickle.load(f)['pred_joint_3d'], np.float32).reshape(21, 3)
    pose = np.loadtxt(os.path.join(init, obj_name, frame_name, 'pred_objpose_%sview' % view_num, cid + '.txt')).astype(np.float32)
    return {'init_joint3d': joint, 'init_Ro': pose[:3, :3], 'init_To': pose[:3, 3]}


def run_pose(args):
    from honerf_amd import harness
    from honerf_amd.pose_metrics import hand_metrics, pose_metrics
    type_path = os.path.join(args.base, 'view_' + args.view_num, args.fit_type)
    for test_obj in args.classes:
        cnum = 0
        sums = {m: dict(joint=0.0, ad=0.0, add=0, adds=0, pa=0.0, auc=0.0, pa_auc=0.0) for m in ('ours', 'init')}
        for obj_name in sorted(os.listdir(type_path)) if os.path.isdir(type_path) else []:
            if test_obj not in obj_name:
                continue
            model = load_model(args.models, obj_name.split('_')[1], args.model_scale)
            obj_path = os.path.join(type_path, obj_name)
            for frame_name in sorted(os.listdir(obj_path)):
                pose_path = os.path.join(obj_path, frame_name, 'pose_' + args.fit_type)
                if not os.path.isdir(pose_path):
                    continue
                poses, inits = [], []
                for file_name in sorted(os.listdir(pose_path)):
                    poses.append(harness.read_pose(os.path.join(pose_path, file_name)))
                    if 'gt_Ro' not in poses[-1]:
                        raise ValueError('%s holds no ground truth' % os.path.join(pose_path, file_name))
                    if args.init:
                        inits.append(read_init(args.init, obj_name, frame_name, args.view_num, file_name.split('.')[0]))
                if not poses:
                    continue
                m = pose_metrics(model, stack(poses, 'pred_'), stack(poses, 'gt_'), stack(inits, 'init_') if args.init else None,
                                 threshold=args.threshold)
                for name, r in m.items():
                    s = sums[name]
                    s['joint'] += float(r['joint'].sum())
                    s['ad'] += float(r['ad'].sum())
                    s['add'] += int(r['add_ok'].sum())
                    s['adds'] += int(r['adds_ok'].sum())
                if args.aligned:                                       # (frame-weighted: every frame has the same 21 joints)
                    gt_j = stack(poses, 'gt_')['joint3d']
                    for name, js in [('ours', stack(poses, 'pred_')['joint3d'])] + ([('init', stack(inits, 'init_')['joint3d'])] if args.init else []):
                        h = hand_metrics(js, gt_j)
                        for k, key in (('pa', 'pa_mpjpe'), ('auc', 'auc'), ('pa_auc', 'pa_auc')):
                            sums[name][k] += h[key] * len(poses)
                cnum += len(poses)
        print('obj_name %s has %d frames' % (test_obj, cnum))
        if not cnum:
            continue
        col = lambda name: (sums[name]['joint'] / cnum * 1000, sums[name]['ad'] / cnum * 1000, sums[name]['add'] / cnum * 100,
                            sums[name]['adds'] / cnum * 100)
        oj, oa, odd, ods = col('ours')
        if args.init:
            ij, ia, idd, ids = col('init')
            print('init joint: %.2lf, ours joint: %.2lf, init ad: %.2lf, init add: %.2lf, init adds: %.2lf, ours ad: %.2lf, ours add: %.2lf, '
                  'ours adds: %.2lf' % (ij, oj, ia, idd, ids, oa, odd, ods))
        else:
            print('ours joint: %.2lf, ours ad: %.2lf, ours add: %.2lf, ours adds: %.2lf' % (oj, oa, odd, ods))
        if args.aligned:
            for name in ('init', 'ours') if args.init else ('ours',):
                s = sums[name]
                print('%s pa joint: %.2lf, %s auc: %.3lf, %s pa auc: %.3lf' % (name, s['pa'] / cnum * 1000, name, s['auc'] / cnum, name, s['pa_auc'] / cnum))
    return 0


def run_accel(args):
    from honerf_amd import harness
    from honerf_amd.pose_metrics import accel_metrics
    base = os.path.join(args.base, 'view_' + args.view_num)
    sub_path = os.path.join(base, '1234')
    names = ('1_3', '123', '1234')
    acc = {n: {'joint': [], 'vert': []} for n in names}
    num_all = 0
    for obj_name in sorted(os.listdir(sub_path)) if os.path.isdir(sub_path) else []:
        model = load_model(args.models, obj_name.split('_')[1], args.model_scale)
        for frame_name in sorted(os.listdir(os.path.join(sub_path, obj_name))):
            dirs = {'1_3': os.path.join(base, '12', obj_name, frame_name, 'pose_12'),
                    '123': os.path.join(base, '123', obj_name, frame_name, 'pose_4'),
                    '1234': os.path.join(base, '1234', obj_name, frame_name, 'pose_4')}
            poses = {n: [] for n in names}
            for cid in range(args.max_frame):
                file_name = '%d.pickle' % cid
                if not os.path.exists(os.path.join(dirs['1_3'], file_name)):
                    continue
                for n in names:
                    poses[n].append(harness.read_pose(os.path.join(dirs[n], file_name)))
            cnum = len(poses['123'])
            num_all += cnum
            if cnum < 3:
                continue
            m = accel_metrics(model, stack(poses['123'], 'gt_'), {n: stack(poses[n], 'pred_') for n in names})
            for n in names:
                acc[n]['joint'].append(m[n]['joint'])
                acc[n]['vert'].append(m[n]['vert'])
    print(num_all)
    mean = lambda n, k: float(np.concatenate(acc[n][k]).mean()) * 1000.0 if acc[n][k] else float('nan')
    print('acc_list_1_3_j: %.2lf, acc_list_1_3_v: %.2lf, acc_list_123_j: %.2lf,  acc_list_123_v: %.2lf,  acc_list_1234_j: %.2lf, '
          'acc_list_1234_v: %.2lf' % (mean('1_3', 'joint'), mean('1_3', 'vert'), mean('123', 'joint'), mean('123', 'vert'),
                                      mean('1234', 'joint'), mean('1234', 'vert')))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('base', help="the reference's ./fit_res")
    ap.add_argument('--view-num', default='8')
    ap.add_argument('--fit-type', default='12')
    ap.add_argument('--models', required=True, help="the reference's ./data/offline_stage_data")
    ap.add_argument('--model-scale', type=float, default=0.001, help='model units to metres (the reference: mm)')
    ap.add_argument('--init', default=None, help="the reference's ./data/catch_sequence/test")
    ap.add_argument('--classes', nargs='+', default=CLASSES)
    ap.add_argument('--threshold', type=float, default=0.015)
    ap.add_argument('--aligned', action='store_true', help='add the Procrustes-aligned joint error and the PCK AUCs, raw and aligned')
    ap.add_argument('--accel', action='store_true', help='the acceleration errors of analys_acc_err.py instead')
    ap.add_argument('--max-frame', type=int, default=2000, help='--accel: frame ids 0 .. max-1 are looked for (the reference: 2000)')
    args = ap.parse_args()
    return run_accel(args) if args.accel else run_pose(args)


if __name__ == '__main__':
    sys.exit(main())
