"""What the tests of the geometry buffers' adjoint (tests/test_gpu_gbuffer_grad.py) rest on, without a GPU.

Conditioning of the cases of gbuffer_grad_cases: the fp32 autograd of the oracle against its float64 autograd, per gradient array
(rel_err: the maximum error over the array's largest float64 value).  Every array is held to gbuffer_grad_cases.FP32_WORST of its
family except the ones `ill_conditioned` names with a reason; those are not given a looser number here -- the GPU test holds a
kernel on them to the rule of helpers.assert_parity (at least as close to float64 as this fp32 oracle is, x1.5 + 1e-5).  The worst
value per family and array is recorded (held arrays) or printed (the others).

Observed (per family, worst over the shapes): thin 1.33e-5 (sdf_h, 5 x 320); soft 9.0e-6 (d, 5 x 320) on the arrays held to the
bound, up to 6.0e-4 (d_h, 5 x 1) on the ill-conditioned ones; back20 1.12e-5 (grad_o, 1 x 320) and up to 3.1e-3 on the sdf arrays
(1.0 on the one-field 1 x 1 case, whose sdf gradient is 5e-12).

Also here: the float64 reference itself against central differences (the reference is autograd of the forward oracle, so this
checks the harness, not the oracle) and fitting.geometry_loss_terms against a float64 numpy statement of its three formulas."""
import numpy as np
import pytest
import torch

import gbuffer_cases as gc
import gbuffer_grad_cases as gg
from helpers import record


@pytest.mark.parametrize('family', list(gg.FAMILIES))
def test_fp32_oracle_gradients_against_float64(family):
    worst = {}
    for n_frames, n_rays, S in gg.shapes():
        for fields in (2, 1):
            if fields == 1 and n_frames != 1:
                continue
            x, up, r64, r32 = gg.case(n_frames, n_rays, S, family, fields)
            for k in gg.WRT[fields]:
                assert r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32 and r64[k].shape == x[k].shape
                assert bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all())
                e = gg.rel_err(r32[k].numpy(), r64[k].numpy())
                why = gg.ill_conditioned(family, k, n_frames * n_rays, S)
                key = (k, 'held' if why is None else 'ill-conditioned')
                worst[key] = max(worst.get(key, 0.0), e)
                if why is None:
                    assert e <= gg.FP32_WORST[family], 'gbuffer%d %d x %d x %d %s: %s: fp32 autograd of the oracle is %.3e from float64 (> %.1e)' % (
                        fields, n_frames, n_rays, S, family, k, e, gg.FP32_WORST[family])
    for (k, kind), e in sorted(worst.items()):
        if kind == 'held':
            record('fp32 oracle gradient %s %s' % (family, k), e, gg.FP32_WORST[family])
        else:
            print('fp32 oracle gradient %s %s (ill-conditioned arrays, no bound): worst %.3e' % (family, k, e))
    held = max(e for (k, kind), e in worst.items() if kind == 'held')
    assert held > 0.05 * gg.FP32_WORST[family], 'FP32_WORST[%s] = %.1e is far above what is observed (%.2e)' % (family, gg.FP32_WORST[family], held)


@pytest.mark.parametrize('fields', (2, 1))
def test_float64_reference_against_central_differences(fields):
    x = gg.inputs(1, 5, 65, 'thin', fields)
    up = gg.upstream(x)
    ref = gg.reference(x, up, torch.float64)

    def value(y):
        out = gc.oracle(y, torch.float64, rotate=False)
        return float(sum((up[k].double() * out[k]).sum() for k in gg.UP))
    g = torch.Generator().manual_seed(5)
    for k in gg.WRT[fields]:
        y = {n: (v.double() if isinstance(v, torch.Tensor) else v) for n, v in x.items()}
        v = torch.randn(x[k].shape, generator=g, dtype=torch.float64)
        h = 1e-6
        y[k] = x[k].double() + h * v
        up_v = value(y)
        y[k] = x[k].double() - h * v
        fd = (up_v - value(y)) / (2 * h)
        an = float((ref[k] * v).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (k, fd, an)


def test_upstream_and_inputs_are_seeded():
    a, b = gg.inputs(1, 5, 64, 'soft', 2), gg.inputs(1, 5, 64, 'soft', 2)
    assert a is not b and all(torch.equal(a[k], b[k]) for k in gg.WRT[2]) and a['inv_s_h'] == a['inv_s_o'] == np.float32(20.0)
    assert gc.FAMILIES == {'surface': 3000.0, 'thin': 14.9, 'back': 300.0}, 'gbuffer_cases is left as it was'
    u, v = gg.upstream(a), gg.upstream(b)
    assert all(torch.equal(u[k], v[k]) for k in gg.UP) and u['normal'].shape == (5, 2, 3)
    assert gg.upstream(gg.inputs(1, 5, 64, 'thin', 1))['opacity'].shape == (5,)


def test_geometry_loss_terms_against_numpy():
    from honerf_amd import fitting
    rng = np.random.RandomState(4)
    P = 41
    b = {k: rng.uniform(0.0, 1.0, size=(P, 1)) for k in ('opacity_hand', 'opacity_obj')}
    b['opacity_hand'][:3, 0] = (0.0, 1.0, 5e-4)            # the clip is hit from both sides
    b['opacity_obj'][3:5, 0] = (1.0 - 1e-4, 0.0)
    b.update({k: rng.uniform(0.0, 1.2, size=(P, 1)) for k in ('depth_hand', 'depth_obj')})
    td = rng.uniform(0.4, 1.5, size=P)
    td[::4] = 0.0
    lab = rng.randint(0, 3, size=P)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in b.items()}
    got = fitting.geometry_loss_terms(t, torch.tensor(td), torch.tensor(lab))
    oh, oo = b['opacity_hand'][:, 0], b['opacity_obj'][:, 0]
    valid = td > 0
    want = {'depth': np.abs(b['depth_hand'][:, 0] + b['depth_obj'][:, 0] - (oh + oo) * td)[valid].mean()}
    for k, o, l in (('mask_hand', oh, 1), ('mask_obj', oo, 2)):
        c, y = np.clip(o, 1e-3, 1.0 - 1e-3), (lab == l).astype(np.float64)
        want[k] = -(y * np.log(c) + (1.0 - y) * np.log(1.0 - c)).mean()
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dim() == 0 and abs(float(got[k].detach()) - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])
    sum(got.values()).backward()
    assert all(bool(torch.isfinite(v.grad).all()) for v in t.values())
    assert sorted(fitting.geometry_loss_terms(t, true_label=torch.tensor(lab))) == ['mask_hand', 'mask_obj']
    assert sorted(fitting.geometry_loss_terms(t, true_depth=torch.tensor(td))) == ['depth']
    none = fitting.geometry_loss_terms(t, torch.zeros(P, dtype=torch.float64), None)
    assert float(none['depth'].detach()) == 0.0, 'no ray with a measurement: the term is 0, not NaN'
