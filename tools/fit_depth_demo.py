"""What the depth and hand / object mask terms of fit_step do to a fit that starts with the object displaced along the
camera axis, the direction a colour + merged-mask loss sees worst.

The synthetic 'surface' scene of the whole-step tests (the object's zero level crosses the fingers), one camera.  The targets are
that camera's view of the scene AT THE TRUE POSE: colour and merged mask from `render`, depth and hand / object labels by
`synthetic_views(with_geometry=...)`.  The pose chain starts from a prediction whose object translation is `--offset` metres
further from the camera along its mean ray; `--iters` Adam steps of fit type '12' follow, once without and once with
geometry=dict(depth_weight=.., mask_weight=..), on the same jitter.  Prints the object's translation error (metres) and the error
along the camera axis at the start and after each fit.  Nothing is asserted.  Needs a GPU.

The loss of fit type '12' holds the object to its predicted pose with 20 x the mean vertex distance (fitting_single.py:283), a pull
of constant size towards the wrong start; the depth term's pull is depth_weight x (the opacity-weighted share of object rays), ~0.3
per unit weight here, so weights of the order of 100 are what moves the object against the regulariser.

    python tools/fit_depth_demo.py [--offset 0.01] [--iters 120] [--depth-weight 200] [--mask-weight 0.5] [--seed 40]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--offset', type=float, default=0.01)
    ap.add_argument('--iters', type=int, default=120)
    ap.add_argument('--depth-weight', type=float, default=200.0)
    ap.add_argument('--mask-weight', type=float, default=0.5)
    ap.add_argument('--seed', type=int, default=40)
    ap.add_argument('--rays', type=int, default=196)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fit_depth_demo: no GPU')
    import bench
    from honerf_amd import fitting as F, lib as L, synth
    dev = torch.device('cuda')
    ren, _ = bench.build_fit_nets(dev, 1, 'f16x3')
    bt, tp, j = synth.synth_hand_pose(args.seed)
    R, tt = synth.synth_obj_pose(args.seed + 1, center=tuple(j[9] + np.array([0.0, 0.30, 0.0])))
    rng = np.random.RandomState(args.seed)
    u = rng.standard_normal((2000, 3))
    verts = (u / np.linalg.norm(u, axis=1, keepdims=True) * 0.025).astype(np.float32)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    truth = dict(renderer=ren, near=bench.NEAR, far=bench.FAR, bt_inv=c(bt), T_pose_21=c(tp), Ro=c(R).T.contiguous(), To=c(tt), opacity_threshold=0.5)
    view = F.synthetic_views(1, 1, args.rays, args.seed, j[9], device=dev, with_geometry=truth)[0]
    rays_o, rays_d = F._rays(L, view['xy'], view['cam'], 1, args.rays)
    with torch.no_grad():
        seen = ren.render(rays_o, rays_d, bench.NEAR, bench.FAR, truth['bt_inv'], truth['T_pose_21'], None, truth['Ro'], truth['To'])
    view['true_rgb'] = seen['color_fine'].detach().clone()
    view['true_mask'] = (seen['weight_sum'].detach() > 0.5).float()
    axis = torch.nn.functional.normalize(rays_d.mean(0), dim=0).cpu().numpy().astype(np.float64)
    start = tt + args.offset * axis
    n_seen = [int((view['true_label'] == k).sum()) for k in (0, 1, 2)]
    print('%d rays: %d background, %d hand, %d object; the object starts %.4f m behind its place along the camera axis'
          % (args.rays, n_seen[0], n_seen[1], n_seen[2], args.offset), flush=True)
    jitter = [torch.rand(args.rays, 1, generator=torch.Generator().manual_seed(1000 + k)).to(dev) for k in range(args.iters)]
    rows = {}
    for name, geometry in (('colour + merged mask', None), ('with depth and hand / object masks', dict(depth_weight=args.depth_weight, mask_weight=args.mask_weight))):
        chain = F.RigidPoseChain(bt[None], tp[None], j[None], R[None], start[None].astype(np.float32), verts, device=dev)
        opt = F.make_optimizer(chain, video=False)
        for k in range(args.iters):
            terms = F.fit_step(ren, view, chain, opt, bench.NEAR, bench.FAR, '12', t_rand=jitter[k], geometry=geometry)
        torch.cuda.synchronize()
        with torch.no_grad():
            err = chain(None)['obj_t'][0].double().cpu().numpy() - tt
        rows[name] = dict(translation_error_m=float(np.linalg.norm(err)), along_camera_axis_m=float(err @ axis),
                          last_terms={k: float(v.detach()) for k, v in terms.items()})
        print('%-36s |t - t_true| = %.5f m, along the camera axis %+.5f m (start: %.5f)' % (name, np.linalg.norm(err), err @ axis, args.offset), flush=True)
    print(json.dumps(dict(tool='fit_depth_demo', offset_m=args.offset, iters=args.iters, depth_weight=args.depth_weight, mask_weight=args.mask_weight,
                          seed=args.seed, rays=args.rays, labels=n_seen, rows=rows)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
