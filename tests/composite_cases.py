"""Cases of the alpha, compositing and sample-point kernels (ho-nerf_amd/csrc/hn_composite.hip, the sample-point part of
hn_sampling.hip): seeded fp32 inputs, the shape tables, and the references.  A plain module: tests/test_composite_cases_cpu.py
(is the fp32 oracle within 5e-6 of float64 on these inputs?) and tests/test_gpu_composite.py (are the kernels within 2e-5 of
float64?) both import it.

The references are the oracle's own statements (oracle.render.sdf_to_alpha, composite_single, composite_dual, eikonal, mid_points,
_pts, and torch.autograd.grad of them) run at the dtype asked for on the SAME fp32 input values cast up; a scalar the kernels take
as a C float (inv_s, sample_dist) is rounded to fp32 first.

The shapes are the smallest that reach each path of the host dispatchers:
  hn_composite1      k_composite1_rows<4,8> at S = 32, <4,16> / <8,16> / <12,16> at 64 / 128 / 192, k_composite1 at every other S;
                     4 rays per block (generic), 4 or 8 rays per wave (rows): 1, 5 and 37 rays leave partial blocks and groups
  hn_composite2      the same without an S = 32 form
  hn_composite*_bwd  k_*_bwd_wave<1..4> at S <= 64 / 128 / 192 / 256 (full and partly empty waves), the thread-per-ray kernel
                     beyond (64 rays per block: 65 rays take two)
  grid stride        the forward grids stop at 2048 blocks: beyond 8 192 rays (generic), 32 768 (16-lane rows), 65 536 (8-lane)
  hn_alpha_bwd       wave-reduced g_rays_d where all 64 lanes of a wave belong to one ray, one atomic per lane elsewhere
  hn_sample_points   k_sample_points_t when n % 4 == 0 and the buffers are 16-byte aligned, k_sample_points otherwise"""
import numpy as np
import torch

from oracle import render as orr

FAMILIES = ('thin', 'surface')
RAYS = (1, 5, 37)
FWD_S = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 320)
FWD_SHAPES = [(n, S) for S in FWD_S for n in RAYS]
GRID1 = ((8197, 33), (32773, 64), (65545, 32))           # n_rays x S: generic, 16-lane rows, 8-lane rows
GRID2 = ((8197, 33), (32773, 64))
ARG_S = (64, 65)                                         # optional arguments: once for a row kernel, once for the generic one
ARG_RAYS = 37
BWD_S = (1, 2, 63, 64, 65, 100, 128, 129, 191, 192, 193, 255, 256, 257, 320)
BWD_SHAPES = [(n, S) for S in BWD_S for n in RAYS] + [(65, 257)]
INV_S = (14.9, 300.0, 3000.0)
ALPHA_SHAPES = ((23, 1), (23, 37), (7, 64), (23, 100), (3, 192), (1, 1))      # n_rays x samples per ray
PTS_N = (1, 4, 5, 40, 41, 64, 130, 132)
PTS_B = (1, 77)
PTS_BWD_N = (1, 63, 65)
NEAR, FAR = 0.4, 1.5


def gen(*key):
    """A generator seeded by a tuple of integers (the same on every run and every machine)."""
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def f32_scalar(v):
    """The value a kernel sees when the C ABI takes `v` as a float."""
    return float(np.float32(v))


def rel_err(a, b):
    """max |a - b| / max |b| (helpers.rel_err; restated so that this module needs nothing of the product)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- compositing ------------------------------------------------------------------------------------------------------------
def alphas(n_rays, S, family, g, fields=1):
    """thin: uniform in [0, 2 / S] (capped at 1, alpha's range: S = 1 only), the transmittance behind the last sample stays
    ~ e^-1, so a wrong carry between lanes or 64-sample segments shows in the late weights.  surface: uniform in [0, 0.3]
    with an exact 0 at sample 0, exact 1 (a 1e-7 transmittance factor, what the no-division adjoint is for) at S // 3, twice in
    a row at S // 2 (S > 4), and at S - 1 in every third ray; planted in that order (at S <= 2 the later one wins).

    thin with fields = 2 (each of the two fields of hn_composite2): the same draw times a ramp from 1.75 at the first sample to
    0.25 at the last (the same optical depth, ~ e^-2 behind the last sample with both fields).  In fp32 every factor
    1 - a + 1e-7 is +1.9e-8 off on average (next to 1 - a in [0.5, 1) the 1e-7 rounds to 2 ulp = 1.19e-7), in the oracle as in
    the kernels; the transmittance in front of sample k carries 2 k of them with two fields, and with the flat profile the fp32
    oracle's weight_sum and colour at S = 320 were 4.9 - 5.9e-6 from float64 over a handful of seeds.  The ramp moves weight to the
    early samples, whose transmittance carries less of it (3.8 - 4.6e-6), and leaves every late weight non-zero."""
    if family == 'thin':
        a = torch.rand(n_rays, S, generator=g) * min(2.0 / S, 1.0)
        return a if fields == 1 else (a * torch.linspace(1.75, 0.25, S)).clamp(max=1.0)
    assert family == 'surface', family
    a = torch.rand(n_rays, S, generator=g) * 0.3
    a[:, 0] = 0.0
    a[:, S // 3] = 1.0
    if S > 4:
        a[:, S // 2] = 1.0
        a[:, S // 2 + 1] = 1.0
    a[::3, S - 1] = 1.0
    return a


def eik_grads(n_rays, S, g):
    """Field gradients for the eikonal term (|grad| - 1)^2: random directions, lengths in [0, 0.7] or [1.3, 2].  (A length within
    rounding of 1 makes the term a cancellation: with N(0,1) gradients the fp32 oracle itself is 9e-6 from float64 on a single
    sample of length 1.007, so |length - 1| >= 0.3 here and the sum stays conditioned at every size down to one sample.)"""
    u = torch.nn.functional.normalize(torch.randn(n_rays, S, 3, generator=g), dim=-1)
    r = torch.rand(n_rays, S, 1, generator=g)
    return u * torch.where(r < 0.5, 1.4 * r, 0.6 + 1.4 * r)


def g_wsums(n_rays, g):
    """The upstream gradient of weight_sum, 0.25 N(0,1).  In fp32, 1 - a + 1e-7 is +1.9e-8 off on average (next to 1 - a in
    [0.5, 1) the 1e-7 rounds to 2 ulp = 1.19e-7), in the oracle as in the kernels; dL/dw_k = g_color . rgb_k + g_wsum has one sign
    along a ray when g_wsum dominates, the adjoint then adds that bias up over all S factors, and with N(0,1) here the fp32 oracle
    was 5.0 - 6.2e-6 from float64 on the thin family at S >= 255 (two fields).  At 0.25 a dropped g_wsum is still an error of
    order 0.1."""
    return 0.25 * torch.randn(n_rays, generator=g)


def composite1_inputs(n_rays, S, family):
    g = gen(1, n_rays, S, FAMILIES.index(family))
    return {'alpha': alphas(n_rays, S, family, g), 'c': torch.rand(n_rays, S, generator=g), 'rgb': torch.rand(n_rays, S, 3, generator=g),
            'grad': eik_grads(n_rays, S, g), 'g_color': torch.randn(n_rays, 3, generator=g),
            'g_wsum': g_wsums(n_rays, g)}


def composite2_inputs(n_rays, S, family):
    g = gen(2, n_rays, S, FAMILIES.index(family))
    x = {}
    for f in ('h', 'o'):        # drawn independently for the hand and the object
        x['alpha_' + f] = alphas(n_rays, S, family, g, fields=2)
        x['rgb_' + f] = torch.rand(n_rays, S, 3, generator=g)
        x['grad_' + f] = eik_grads(n_rays, S, g)
    x['g_color'] = torch.randn(n_rays, 3, generator=g)
    x['g_wsum'] = g_wsums(n_rays, g)
    return x


def _detached(d):
    return {k: v.detach() for k, v in d.items()}


def composite1_oracle(x, dtype, adjoint=False, with_wsum=True):
    """colour [B,3], weights [B,S], weight_sum / weight_max [B], eik_sum () = sum (|grad| - 1)^2; with `adjoint`, g_alpha, g_c,
    g_rgb of sum(colour g_color) [+ sum(weight_sum g_wsum)]."""
    a, c, rgb = (x[k].to(dtype).requires_grad_(adjoint) for k in ('alpha', 'c', 'rgb'))
    w, col = orr.composite_single(a, c, rgb)
    out = {'color': col, 'weights': w, 'weight_sum': w.sum(-1), 'weight_max': w.max(-1)[0],
           'eik_sum': orr.eikonal(x['grad'].to(dtype), tuple(a.shape)) * a.numel()}
    if adjoint:
        loss = (col * x['g_color'].to(dtype)).sum()
        if with_wsum:
            loss = loss + (w.sum(-1) * x['g_wsum'].to(dtype)).sum()
        out['g_alpha'], out['g_c'], out['g_rgb'] = torch.autograd.grad(loss, [a, c, rgb])
    return _detached(out)


def composite2_oracle(x, dtype, adjoint=False, with_wsum=True):
    """colour [B,3], weight_sum [B], w_hand / w_obj [B,S], eik_h / eik_o (); with `adjoint`, g_alpha_h, g_rgb_h, g_alpha_o, g_rgb_o."""
    ah, rh, ao, ro = (x[k].to(dtype).requires_grad_(adjoint) for k in ('alpha_h', 'rgb_h', 'alpha_o', 'rgb_o'))
    col, ws, wh, wo = orr.composite_dual(ah, rh, ao, ro)
    out = {'color': col, 'weight_sum': ws[:, 0], 'w_hand': wh, 'w_obj': wo,
           'eik_h': orr.eikonal(x['grad_h'].to(dtype), tuple(ah.shape)) * ah.numel(),
           'eik_o': orr.eikonal(x['grad_o'].to(dtype), tuple(ao.shape)) * ao.numel()}
    if adjoint:
        loss = (col * x['g_color'].to(dtype)).sum()
        if with_wsum:
            loss = loss + (ws[:, 0] * x['g_wsum'].to(dtype)).sum()
        out['g_alpha_h'], out['g_rgb_h'], out['g_alpha_o'], out['g_rgb_o'] = torch.autograd.grad(loss, [ah, rh, ao, ro])
    return _detached(out)


# ---- sdf -> alpha -------------------------------------------------------------------------------------------------------------
def alpha_inputs(n_rays, spr, inv_s):
    """sdf ~ 0.05 N(0,1) [N,1], grad ~ N(0,1) [N,3], unit rays_d [n_rays,3], dists in [0, 0.02] [N,1], upstream g_alpha, g_c ~ N(0,1).
    Where |dir . grad| < 1e-3 the gradient gets 0.01 dir on top: fp32 and float64 then take the same side of min(dir . grad, 0).
    Sample 0 is planted on the surface, facing the ray: sdf = 0, grad = -dir, a section of min(0.02, 1 / inv_s) and upstream
    gradients of 1.  rel_err is relative to the tensor's largest magnitude, and without such a sample a small tensor may hold none
    at the operation's own scale: at inv_s = 3000 nearly every sigmoid of sdf ~ 0.05 N(0,1) is saturated (23 x 1: the fp32 oracle's
    g_grad was 1e-1 from float64, all of it rounding of ~0), and a back-facing sample's alpha is 1e-5 / (c + 1e-5), whose sdf
    gradient is a difference of O(inv_s) terms that nearly cancel (1 x 1: 5e-3)."""
    g = gen(3, n_rays, spr)
    n = n_rays * spr
    sdf = 0.05 * torch.randn(n, 1, generator=g)
    grad = torch.randn(n, 3, generator=g)
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    dists = 0.02 * torch.rand(n, 1, generator=g)
    g_alpha, g_c = torch.randn(n, 1, generator=g), torch.randn(n, 1, generator=g)
    dirs = d[:, None, :].expand(n_rays, spr, 3).reshape(-1, 3)
    sdf[0], grad[0], dists[0], g_alpha[0], g_c[0] = 0.0, -dirs[0], min(0.02, 1.0 / inv_s), 1.0, 1.0
    tc = (dirs.double() * grad.double()).sum(-1, keepdim=True)
    grad = torch.where(tc.abs() < 1e-3, grad + 0.01 * dirs, grad)
    tc = (dirs.double() * grad.double()).sum(-1)
    assert float(tc.abs().min()) >= 9e-4, 'alpha inputs: a sample sits on the min(dir . grad, 0) branch'
    return {'sdf': sdf, 'grad': grad, 'rays_d': d, 'dists': dists, 'g_alpha': g_alpha, 'g_c': g_c, 'n_rays': n_rays, 'spr': spr,
            'inv_s': f32_scalar(inv_s)}


def alpha_oracle(x, dtype, adjoint=False, with_gc=True):
    """alpha, c [N]; with `adjoint`, g_sdf [N], g_grad [N,3], g_rays_d [n_rays,3] of sum(alpha g_alpha) [+ sum(c g_c)]."""
    sdf, grad, d = (x[k].to(dtype).requires_grad_(adjoint) for k in ('sdf', 'grad', 'rays_d'))
    dirs = d[:, None, :].expand(x['n_rays'], x['spr'], 3).reshape(-1, 3)
    a, c = orr.sdf_to_alpha(sdf, grad, dirs, x['dists'].to(dtype), torch.tensor(x['inv_s'], dtype=dtype))
    out = {'alpha': a[:, 0], 'c': c[:, 0]}
    if adjoint:
        loss = (a * x['g_alpha'].to(dtype)).sum()
        if with_gc:
            loss = loss + (c * x['g_c'].to(dtype)).sum()
        g_sdf, out['g_grad'], out['g_rays_d'] = torch.autograd.grad(loss, [sdf, grad, d])
        out['g_sdf'] = g_sdf[:, 0]
    return _detached(out)


# ---- sample points ------------------------------------------------------------------------------------------------------------
def points_inputs(n_rays, n):
    """Sorted depths in [NEAR, FAR] [B,n], origins ~ N(0,1), unit directions, sample_dist (FAR - NEAR) / n as the kernel sees it,
    an upstream g_pts ~ N(0,1) [B n,3]."""
    g = gen(4, n_rays, n)
    z = torch.sort(NEAR + (FAR - NEAR) * torch.rand(n_rays, n, generator=g), -1)[0]
    return {'z': z, 'rays_o': torch.randn(n_rays, 3, generator=g),
            'rays_d': torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1),
            'sample_dist': f32_scalar((FAR - NEAR) / n), 'g_pts': torch.randn(n_rays * n, 3, generator=g)}


def points_oracle(x, mid, dtype, adjoint=False):
    """pts [B n,3] (at the section mid-points with `mid`, then dists [B,n] as well); with `adjoint`, g_rays_o, g_rays_d [B,3]."""
    o, d = (x[k].to(dtype).requires_grad_(adjoint) for k in ('rays_o', 'rays_d'))
    z = x['z'].to(dtype)
    out = {}
    if mid and z.shape[1] == 1:     # (mid_points shapes the last section after the differences, of which one sample has none)
        out['dists'] = torch.full_like(z, x['sample_dist'])
        z = z + out['dists'] * 0.5
    elif mid:
        z, out['dists'] = orr.mid_points(z, x['sample_dist'])
    out['pts'] = orr._pts(o, d, z).reshape(-1, 3)
    if adjoint:
        out['g_rays_o'], out['g_rays_d'] = torch.autograd.grad((out['pts'] * x['g_pts'].to(dtype)).sum(), [o, d])
    return _detached(out)
