"""Conditioning of the inputs of tests/test_gpu_composite.py (needs no GPU): on every shape and family of composite_cases the
fp32 oracle agrees with the float64 oracle to 5e-6 (rel_err: the maximum error over the tensor's maximum magnitude), for values
and for gradients.  The GPU tests hold the kernels to 2e-5 against float64 on the same inputs, four times this bound; an input
on which fp32 arithmetic itself cannot get within 5e-6 would make that bound a statement about the input, not the kernel, so
such an input is changed (in composite_cases), never the bound."""
import pytest
import torch

import composite_cases as cc

FP32_BOUND = 5e-6


def _agree(f32, f64, what):
    assert f32.keys() == f64.keys()
    for k in f64:
        assert f32[k].dtype == torch.float32 and f64[k].dtype == torch.float64, (what, k)
        e = cc.rel_err(f32[k].numpy(), f64[k].numpy())
        assert e <= FP32_BOUND, '%s: %s: fp32 oracle is %.3e from float64 (> %.0e)' % (what, k, e, FP32_BOUND)


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('S', cc.FWD_S)
def test_composite_forward_inputs(S, family):
    for n_rays in cc.RAYS:
        x = cc.composite1_inputs(n_rays, S, family)
        _agree(cc.composite1_oracle(x, torch.float32), cc.composite1_oracle(x, torch.float64), 'composite1 %d x %d %s' % (n_rays, S, family))
        x = cc.composite2_inputs(n_rays, S, family)
        _agree(cc.composite2_oracle(x, torch.float32), cc.composite2_oracle(x, torch.float64), 'composite2 %d x %d %s' % (n_rays, S, family))


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('n_rays,S', cc.GRID1)
def test_composite_grid_stride_inputs(n_rays, S, family):
    x = cc.composite1_inputs(n_rays, S, family)
    _agree(cc.composite1_oracle(x, torch.float32), cc.composite1_oracle(x, torch.float64), 'composite1 %d x %d %s' % (n_rays, S, family))
    if (n_rays, S) in cc.GRID2:
        x = cc.composite2_inputs(n_rays, S, family)
        _agree(cc.composite2_oracle(x, torch.float32), cc.composite2_oracle(x, torch.float64), 'composite2 %d x %d %s' % (n_rays, S, family))


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('S', cc.BWD_S)
def test_composite_adjoint_inputs(S, family):
    for n_rays, s in cc.BWD_SHAPES:
        if s != S:
            continue
        for with_wsum in (True, False):
            tag = '%d x %d %s%s' % (n_rays, S, family, '' if with_wsum else ' g_weight_sum NULL')
            x = cc.composite1_inputs(n_rays, S, family)
            _agree(cc.composite1_oracle(x, torch.float32, True, with_wsum), cc.composite1_oracle(x, torch.float64, True, with_wsum), 'composite1_bwd ' + tag)
            x = cc.composite2_inputs(n_rays, S, family)
            _agree(cc.composite2_oracle(x, torch.float32, True, with_wsum), cc.composite2_oracle(x, torch.float64, True, with_wsum), 'composite2_bwd ' + tag)


@pytest.mark.parametrize('inv_s', cc.INV_S)
@pytest.mark.parametrize('n_rays,spr', cc.ALPHA_SHAPES)
def test_alpha_inputs(n_rays, spr, inv_s):
    x = cc.alpha_inputs(n_rays, spr, inv_s)
    for with_gc in (True, False):
        _agree(cc.alpha_oracle(x, torch.float32, True, with_gc), cc.alpha_oracle(x, torch.float64, True, with_gc),
               'alpha %d x %d inv_s=%g%s' % (n_rays, spr, inv_s, '' if with_gc else ' g_c NULL'))


@pytest.mark.parametrize('n', sorted(set(cc.PTS_N + cc.PTS_BWD_N)))
def test_sample_point_inputs(n):
    for B in cc.PTS_B:
        x = cc.points_inputs(B, n)
        for mid in (0, 1):
            _agree(cc.points_oracle(x, mid, torch.float32, True), cc.points_oracle(x, mid, torch.float64, True), 'sample_points %d x %d mid=%d' % (B, n, mid))


def test_planted_values_are_where_the_tables_say():
    """The surface family's exact values (the 1e-7 transmittance factors) and the thin family's range."""
    a = cc.alphas(37, 192, 'surface', cc.gen(0))
    assert (a[:, 0] == 0.0).all() and (a[:, 64] == 1.0).all() and (a[:, 96] == 1.0).all() and (a[:, 97] == 1.0).all()
    assert (a[::3, 191] == 1.0).all() and (a[1::3, 191] < 0.3).all() and float(a.max()) == 1.0
    assert float(((a == 1.0).sum(1)).max()) == 4
    for S in cc.FWD_S:
        t = cc.alphas(37, S, 'thin', cc.gen(S))
        assert float(t.min()) >= 0.0 and float(t.max()) <= min(2.0 / S, 1.0)
        if S >= 31:     # the transmittance behind the last sample: what a wrong carry would change is not rounded away
            assert float((1.0 - t.double()).prod(1).min()) > 0.1, S
