"""Cases of the geometry buffers' adjoint kernels (hn_gbuffer1_bwd / hn_gbuffer2_bwd, ho-nerf_amd/csrc/hn_gbuffer.hip): the inputs of
gbuffer_cases, seeded upstream gradients and the reference.  A plain module: tests/test_gbuffer_grad_cpu.py (how far is the fp32
autograd of the oracle from float64 on these inputs?) and tests/test_gpu_gbuffer_grad.py (the kernels against float64) import it.

The reference is torch.autograd.grad of sum(upstream * gbuffer_cases.oracle(x, dtype, rotate=False)) w.r.t. the sdf, the field
gradients and the ray directions, at the dtype asked for, on the same fp32 input values cast up.  The object's normal stays in
the object's frame (rotate=False), as the kernels take its upstream gradient.

Families.  The forward suite's `surface` (inv_s 3000) and `back` (300) are kept out of the value comparisons: at those inv_s the
sigmoids are saturated on all but a sample or two per ray, so whole gradient arrays are 1e-14 .. 1e-50 in float64 and an error
relative to an array's maximum says nothing there; `surface` also sits on the clip (alphas of exactly 1), where the one-sided
derivative is a convention.  So:
  thin     as in gbuffer_cases (inv_s 14.9)
  soft     the `surface` geometry (a sign change of the sdf inside the ray) at inv_s = 20, what the synthetic variance 0.3 gives
  back20   the `back` geometry (back-facing gradients: iter_cos clamps to 0 and true_cos gets no gradient) at inv_s = 20
  surface  as in gbuffer_cases (inv_s 3000; alphas of exactly 1, factors of 1e-7): only "every output is finite"
"""
import functools

import torch

import gbuffer_cases as gc
from composite_cases import f32_scalar, gen, rel_err  # noqa: F401  (rel_err: for the importers)

# family -> (geometry of gbuffer_cases, inv_s)
FAMILIES = {'thin': ('thin', 14.9), 'soft': ('surface', 20.0), 'back20': ('back', 20.0)}
FINITE_ONLY = {'surface': ('surface', 3000.0)}
MISALIGNED = (1, 37, 64)                       # the S = 64 case whose depths start 4 bytes off a 16-byte boundary: the generic kernel
WRT = {2: ('sdf_h', 'grad_h', 'd_h', 'sdf_o', 'grad_o', 'd_o'), 1: ('sdf', 'grad', 'd')}
UP = ('opacity', 'depth', 'normal')

# The worst error of the fp32 autograd of the oracle against float64 over every shape of a family (per array: the maximum error over
# the array's largest float64 value), rounded up, on the arrays fp32 arithmetic resolves; test_gbuffer_grad_cpu.py asserts these and
# names the arrays it does not hold to them (`ill_conditioned`).  Observed: thin 1.33e-5 (sdf_h, 5 x 320), soft 9.0e-6 (d, 5 x 320),
# back20 1.12e-5 (grad_o, 1 x 320).  The GPU tests hold the kernels to four times these, the ratio of the forward pair (5e-6 and 2e-5).
FP32_WORST = {'thin': 1.4e-5, 'soft': 1.4e-5, 'back20': 1.2e-5}
GPU_FACTOR = 4.0


def ill_conditioned(family, name, n_rays, S):
    """Arrays whose fp32 autograd of the oracle is further than FP32_WORST from float64, and why (None: held to FP32_WORST):
      back20, the sdf   with iter_cos clamped to 0 both cdf values are equal and d alpha / d sdf is the difference of two terms that
                        agree to 5 digits ((B - A) / B^2 - 1 / B at B - A = c): 1e-4 .. 3e-3 at every S
      soft, S <= 2      one or two samples per ray: sdf and direction gradients are 1e-3 .. 1e-2 of the case's largest gradient and
                        carry the absolute error of that scale (up to 6e-4 of their own maximum)
      soft, one ray     the array's maximum is a single ray's: up to 4.1e-5 (sdf_h, 1 x 320)
    The GPU test holds these to helpers.assert_parity's rule instead: at least as close to float64 as the fp32 oracle, x1.5 + 1e-5."""
    if family == 'back20' and name.startswith('sdf'):
        return 'equal cdf values: d alpha / d sdf cancels'
    if family == 'soft' and S <= 2:
        return 'one or two samples per ray'
    if family == 'soft' and n_rays == 1:
        return 'a single ray'
    return None


def shapes():
    """(n_frames, rays_per_frame, S) of every shape: gbuffer_cases' table, the frames case, the two grid-stride shapes."""
    return gc.all_cases() + [(1, n, S) for n, S in gc.GRID]


def inputs(n_frames, rays_per_frame, S, family, fields):
    """gbuffer_cases.inputs of the family's geometry with the family's inv_s; a new dictionary per call."""
    geometry, inv_s = {**FAMILIES, **FINITE_ONLY}[family]
    x = dict(gc.inputs(n_frames, rays_per_frame, S, geometry, fields))
    v = f32_scalar(inv_s)
    for k in ('inv_s', 'inv_s_h', 'inv_s_o'):
        if k in x:
            x[k] = v
    x['family'] = family
    return x


def upstream(x):
    """Seeded standard-normal g_opacity / g_depth / g_normal in the outputs' shapes (fp32)."""
    N, S = x['z'].shape
    g = gen(11, x['n_frames'], x['rays_per_frame'], S, x['fields'])
    lead = (N, 2) if x['fields'] == 2 else (N,)
    return {'opacity': torch.randn(*lead, generator=g), 'depth': torch.randn(*lead, generator=g), 'normal': torch.randn(*lead, 3, generator=g)}


def reference(x, up, dtype, only=UP):
    """{name: gradient} of sum_k (up[k] * buffer_k) for k in `only`, w.r.t. WRT[fields], by autograd of the oracle at `dtype`."""
    names = WRT[x['fields']]
    y = dict(x)
    for k in names:
        y[k] = x[k].to(dtype).clone().requires_grad_(True)
    out = gc.oracle(y, dtype, rotate=False)
    total = sum((up[k].to(dtype) * out[k]).sum() for k in only)
    grads = torch.autograd.grad(total, [y[k] for k in names])
    return {k: g.detach() for k, g in zip(names, grads)}


@functools.lru_cache(maxsize=None)
def case(n_frames, rays_per_frame, S, family, fields):
    """(inputs, upstream, float64 reference, fp32 reference) of a case, computed once and shared; treat as read-only."""
    x = inputs(n_frames, rays_per_frame, S, family, fields)
    up = upstream(x)
    return x, up, reference(x, up, torch.float64), reference(x, up, torch.float32)
