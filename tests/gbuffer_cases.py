"""Cases of the geometry-buffer kernels (ho-nerf_amd/csrc/hn_gbuffer.hip): seeded fp32 inputs, the shape tables and the reference.
A plain module, in the manner of composite_cases: tests/test_gbuffer_cpu.py (is the fp32 oracle within 5e-6 of float64 on these
inputs?) and tests/test_gpu_gbuffer.py (are the kernels within 2e-5 of float64?) both import it.

The reference is the definition of the buffers stated with the oracle's own pieces (oracle.render.mid_points, sdf_to_alpha,
composite_single / composite_dual) at the dtype asked for, on the SAME fp32 input values cast up; inv_s and sample_dist are rounded
to fp32 first, as the C ABI takes them.

    dist_k = z_{k+1} - z_k (the last one sample_dist), m_k = z_k + dist_k / 2, alpha_k / c_k = sdf_to_alpha per field
    two fields: w^f = composite_dual's weights; one field: composite_single's (transmittance seeded with c_0)
    opacity^f = sum_k w^f_k, depth^f = sum_k w^f_k m_k, normal^f = sum_k w^f_k grad^f_k; the object's normal times Ro (row vector:
    Ro^T n), with the frame's Ro

The shapes are the smallest that reach every path of the dispatcher (gbuffer_launch):
  k_gbuffer_rows<4 / 8 / 12, NF>  S = 64 / 128 / 192 (4 rays per wave, 16 per block: 1, 5 and 37 rays leave partial waves and blocks)
  k_gbuffer<NF>                   every other S (1 and 2: a ray shorter than a wave; 63, 65, 193: around a 64-sample segment; 320:
                                  five segments), and S = 64 with a depth buffer that is not 16-byte aligned
  grid stride                     the grids stop at 2048 blocks: beyond 8 192 rays (generic), 32 768 (rows)
  per-frame Ro                    2 frames x 5 rays at S = 192"""
import os

import numpy as np
import torch

from composite_cases import FAR, NEAR, f32_scalar, gen, rel_err  # noqa: F401  (rel_err: for the importers)
from oracle import render as orr

# family -> inv_s of (every) field.  surface: a sign change of the sdf inside the ray, at inv_s = 3000 the sample behind it has an
# alpha of exactly 1; thin: the sdf stays 0.06 - 0.31 above the surface, alpha is O(1 / S) along the whole ray and the transmittance
# behind the last sample is ~ e^-1; back: back-facing gradients (rays_d . grad > 0, iter_cos clamps to 0: alpha = 1e-5 / (c + 1e-5)).
# The thin sdf rises along the ray, as composite_cases' two-field ramp does and for its reason: in fp32 every factor 1 - a + 1e-7 is
# +1.9e-8 off on average, the transmittance in front of sample k carries k (2 k with two fields) of them, and with a flat sdf of
# 0.15 - 0.25 the fp32 oracle's depth at S = 320 was 6.0 - 7.2e-6 from float64; with the weight on the early samples it is 3.6e-6.
FAMILIES = {'surface': 3000.0, 'thin': 14.9, 'back': 300.0}
RAYS = (1, 5, 37)
S_ALL = (1, 2, 63, 64, 65, 128, 192, 193, 320)
FRAMES_CASE = (2, 5, 192)                      # n_frames, rays per frame, S
GRID = ((8197, 33), (32773, 64))               # n_rays x S just beyond the 2048-block cap: generic, rows
ARG_S = (64, 65)                               # NULL outputs: once for a row kernel, once for the generic one
ARG_RAYS = 37


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def _rotations(n, g):
    """n random rotation matrices [n,3,3] (QR of a Gaussian matrix, made proper), float64."""
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    return q * torch.linalg.det(q)[:, None, None]


def _field(z_mid, d, family, g):
    """sdf [N,S] and grad [N,S,3] of one field along rays of direction d [N,3] (that field's frame) at the section mid-points."""
    N, S = z_mid.shape
    cos = 0.3 + 0.7 * torch.rand(N, 1, generator=g, dtype=torch.float64)
    r = torch.randn(N, S, 3, generator=g, dtype=torch.float64)
    dd = d[:, None, :]
    perp = r - (r * dd).sum(-1, keepdim=True) * dd
    perp = 0.4 * _unit(perp)
    if family == 'surface':
        z_s = NEAR + (FAR - NEAR) * (0.25 + 0.5 * torch.rand(N, 1, generator=g, dtype=torch.float64))
        sdf = (z_s - z_mid) * cos + 0.0005 * torch.randn(N, S, generator=g, dtype=torch.float64)
        grad = -cos[:, :, None] * dd + perp
    elif family == 'thin':
        sdf = 0.06 + 0.22 * torch.linspace(0.0, 1.0, S, dtype=torch.float64) + 0.03 * torch.rand(N, S, generator=g, dtype=torch.float64)
        grad = -cos[:, :, None] * dd + perp
    else:
        assert family == 'back', family
        sdf = 0.05 * torch.randn(N, S, generator=g, dtype=torch.float64)
        grad = cos[:, :, None] * dd + perp
    return sdf.float(), grad.float()


def inputs(n_frames, rays_per_frame, S, family, fields):
    """fields = 2: hand and object (`sdf_h`, `grad_h`, `d_h`, `sdf_o`, `grad_o`, `d_o`, `Ro` [n_frames,3,3]); fields = 1: `sdf`, `grad`,
    `d`.  Both: `z` [N,S] sorted in [NEAR, FAR] with one repeated depth per ray (S >= 2: a section of length 0), unit directions,
    `inv_s` per field, `sample_dist` = (FAR - NEAR) / S, all as the kernel sees them (fp32)."""
    N = n_frames * rays_per_frame
    g = gen(7, n_frames, rays_per_frame, S, list(FAMILIES).index(family), fields)
    z = torch.sort(NEAR + (FAR - NEAR) * torch.rand(N, S, generator=g), -1)[0]
    if S >= 2:
        z[:, S // 2] = z[:, S // 2 - 1]
    sample_dist = f32_scalar((FAR - NEAR) / S)
    zd = z.double()
    dists = torch.cat([zd[:, 1:] - zd[:, :-1], torch.full((N, 1), sample_dist, dtype=torch.float64)], -1)
    mid = zd + 0.5 * dists
    d = _unit(torch.randn(N, 3, generator=g, dtype=torch.float64))
    x = {'z': z, 'sample_dist': sample_dist, 'n_frames': n_frames, 'rays_per_frame': rays_per_frame, 'S': S, 'fields': fields}
    inv_s = f32_scalar(FAMILIES[family])
    if fields == 1:
        x['sdf'], x['grad'] = _field(mid, d, family, g)
        x['d'], x['inv_s'] = d.float(), inv_s
        return x
    Ro = _rotations(n_frames, g)
    d_o = _unit(torch.einsum('fij,fpj->fpi', Ro, d.reshape(n_frames, rays_per_frame, 3)).reshape(N, 3))
    x['sdf_h'], x['grad_h'] = _field(mid, d, family, g)
    x['sdf_o'], x['grad_o'] = _field(mid, d_o, family, g)
    x['d_h'], x['d_o'], x['Ro'] = d.float(), d_o.float(), Ro.float()
    x['inv_s_h'] = x['inv_s_o'] = inv_s
    return x


def _mid(z, sample_dist):
    if z.shape[-1] == 1:      # (mid_points shapes the last section after the differences, of which one sample has none)
        dists = torch.full_like(z, sample_dist)
        return z + dists * 0.5, dists
    return orr.mid_points(z, sample_dist)


def _alpha(sdf, grad, d, dists, inv_s, dtype):
    N, S = sdf.shape
    dirs = d.to(dtype)[:, None, :].expand(N, S, 3).reshape(-1, 3)
    a, c = orr.sdf_to_alpha(sdf.to(dtype).reshape(-1, 1), grad.to(dtype).reshape(-1, 3), dirs, dists.reshape(-1, 1),
                            torch.tensor(inv_s, dtype=dtype))
    return a.reshape(N, S), c.reshape(N, S)


def buffers(w, mid, grad):
    """opacity [N], depth [N], normal [N,3] of one field from its weights [N,S]."""
    return w.sum(-1), (w * mid).sum(-1), (w[:, :, None] * grad).sum(1)


def oracle(x, dtype, rotate=True, with_alpha=False):
    """fields = 2 -> opacity [N,2], depth [N,2], normal [N,2,3] (hand, obj; the object's normal in the world frame unless `rotate`
    is off); fields = 1 -> opacity [N], depth [N], normal [N,3]; with_alpha: alpha_h, alpha_o / alpha [N,S] as well."""
    mid, dists = _mid(x['z'].to(dtype), x['sample_dist'])
    if x['fields'] == 1:
        a, c = _alpha(x['sdf'], x['grad'], x['d'], dists, x['inv_s'], dtype)
        g = x['grad'].to(dtype)
        w, _ = orr.composite_single(a, c, g)
        op, dp, nr = buffers(w, mid, g)
        return {'opacity': op, 'depth': dp, 'normal': nr, **({'alpha': a} if with_alpha else {})}
    ah, _ = _alpha(x['sdf_h'], x['grad_h'], x['d_h'], dists, x['inv_s_h'], dtype)
    ao, _ = _alpha(x['sdf_o'], x['grad_o'], x['d_o'], dists, x['inv_s_o'], dtype)
    gh, go = x['grad_h'].to(dtype), x['grad_o'].to(dtype)
    _, _, wh, wo = orr.composite_dual(ah, gh, ao, go)
    oh, dh, nh = buffers(wh, mid, gh)
    oo, do, no = buffers(wo, mid, go)
    if rotate:
        F, P = x['n_frames'], x['rays_per_frame']
        no = torch.einsum('fpj,fji->fpi', no.reshape(F, P, 3), x['Ro'].to(dtype)).reshape(F * P, 3)
    return {'opacity': torch.stack([oh, oo], -1), 'depth': torch.stack([dh, do], -1), 'normal': torch.stack([nh, no], 1),
            **({'alpha_h': ah, 'alpha_o': ao} if with_alpha else {})}


def all_cases():
    """(n_frames, rays_per_frame, S) of every shape but the grid-stride ones."""
    return [(1, n, S) for S in S_ALL for n in RAYS] + [FRAMES_CASE]


def golden_inputs():
    """tests/golden/gbuffer_dual.npz (make_golden_gbuffer.py) -> (the file, its inputs as `inputs` shapes them)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gbuffer_dual.npz'))
    N, S = g['z_vals'].shape
    t = torch.from_numpy
    x = {'sdf_h': t(g['sdf_hand']).reshape(N, S), 'grad_h': t(g['grad_hand']).reshape(N, S, 3), 'sdf_o': t(g['sdf_obj']).reshape(N, S),
         'grad_o': t(g['grad_obj']).reshape(N, S, 3), 'd_h': t(g['rays_d']), 'd_o': t(g['rays_d_obj']), 'z': t(g['z_vals']),
         'Ro': t(g['Ro']).reshape(1, 3, 3), 'inv_s_h': float(g['inv_s_hand']), 'inv_s_o': float(g['inv_s_obj']),
         'sample_dist': float(g['sample_dist']), 'n_frames': 1, 'rays_per_frame': N, 'S': S, 'fields': 2}
    return g, x
