#!/usr/bin/env python3
"""Generate tests/golden/gbuffer_dual.npz: the REFERENCE's own `NeuSRenderer_fitting.get_alpha_sample_color` (utils/renderer.py:360-422)
for the hand and for the object on 8 rays x 192 given depths, and the geometry buffers formed in float64 numpy from what it returns.
Run in the build container only:

    python tests/golden/make_golden_gbuffer.py

Weights come from honerf_amd.synth (as in make_golden.py).  The fixture holds what hn_gbuffer2 takes (the reference's per-sample sdf
and gradients, the depths, both ray directions, Ro, both inv_s, sample_dist), the reference's alpha of both fields, and

    T_k = prod_{j<k} (1 - a^h_j + 1e-7)(1 - a^o_j + 1e-7), w^f = a^f T         (utils/renderer.py:512-520, on the reference's alpha)
    opacity^f = sum_k w^f_k, depth^f = sum_k w^f_k m_k, normal^f = sum_k w^f_k grad^f_k, the object's as Ro^T n

with m the section mid-points of the depths.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference)

N_RAYS, S = 8, 192
NEAR, FAR, N_SAMPLES = 0.4, 1.5, 64


def main():
    torch.manual_seed(0)
    _, nets = mg.build_nets()
    o, d, bt_inv, T_pose, joints = mg.hand_scene_rays(N_RAYS, 17)
    R_obj, t_obj = mg.synth.synth_obj_pose(5, center=tuple(joints[9] + np.array([0.03, 0.0, 0.02])))
    Ro = torch.from_numpy(R_obj).T.contiguous()
    To = torch.from_numpy(t_obj).clone()
    ren = mg.rr.NeuSRenderer_fitting(nets['sdf_hand'], nets['var_hand'], nets['color_hand'], nets['sdf_obj'], nets['var_obj'],
                                     nets['color_obj'], N_SAMPLES, 64, 0, 4, 1.0)
    g = torch.Generator().manual_seed(77)
    z = torch.sort(0.8 + 0.4 * torch.rand(N_RAYS, S, generator=g), -1)[0]       # around the hand (joints at z ~ 0.9 - 1.07)
    sample_dist = float(np.float32((FAR - NEAR) / N_SAMPLES))
    with torch.no_grad():
        o_l, d_l = ren.convert_obj_to_local(o, d, Ro, To)
    alpha_h, _, sdf_h, _, grad_h = ren.get_alpha_sample_color(o, d, bt_inv, T_pose, z, sample_dist, 'hand')
    alpha_o, _, sdf_o, _, grad_o = ren.get_alpha_sample_color(o_l, d_l, bt_inv, T_pose, z, sample_dist, 'obj')
    inv_s_h = nets['var_hand'](torch.zeros([1, 3]))[:, :1].clip(1e-6, 1e6)
    inv_s_o = nets['var_obj'](torch.zeros([1, 3]))[:, :1].clip(1e-6, 1e6)

    f64 = lambda t: mg.np_(t).astype(np.float64)
    ah, ao = f64(alpha_h), f64(alpha_o)
    zz = f64(z)
    dists = np.concatenate([zz[:, 1:] - zz[:, :-1], np.full((N_RAYS, 1), sample_dist)], -1)
    mid = zz + 0.5 * dists
    fac = (1.0 - ah + 1e-7) * (1.0 - ao + 1e-7)
    T = np.cumprod(np.concatenate([np.ones((N_RAYS, 1)), fac], -1), -1)[:, :-1]
    out = {}
    for f, a, grad in (('hand', ah, grad_h), ('obj', ao, grad_o)):
        w = a * T
        out['opacity_' + f] = w.sum(-1)
        out['depth_' + f] = (w * mid).sum(-1)
        out['normal_' + f] = (w[:, :, None] * f64(grad).reshape(N_RAYS, S, 3)).sum(1)
    out['normal_obj'] = out['normal_obj'] @ f64(Ro)          # row vectors: Ro^T n
    mg.save('gbuffer_dual', rays_d=d, rays_d_obj=d_l, Ro=Ro, z_vals=z, sample_dist=np.float32(sample_dist), inv_s_hand=inv_s_h.reshape(()),
            inv_s_obj=inv_s_o.reshape(()), sdf_hand=sdf_h, sdf_obj=sdf_o, grad_hand=grad_h, grad_obj=grad_o, alpha_hand=alpha_h,
            alpha_obj=alpha_o, **out)
    print('opacity hand', out['opacity_hand'].round(3), 'obj', out['opacity_obj'].round(3))


if __name__ == '__main__':
    main()
