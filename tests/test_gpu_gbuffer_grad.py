"""GPU tests of the geometry buffers' adjoint: the kernels of ho-nerf_amd/csrc/hn_gbuffer.hip through the C ABI (hn_gbuffer1_bwd /
hn_gbuffer2_bwd) against the float64 autograd of the definition on the same fp32 inputs (tests/gbuffer_grad_cases.py: inputs,
upstream gradients, references, families; tests/test_gbuffer_grad_cpu.py: how far the fp32 autograd of the oracle is from float64
on every one of them), then the layers above: autograd.gbuffer1 / gbuffer2, render_buffers(graph=True) of both two-field renderer
classes, gradients through the whole render, fitting.geometry_loss_terms and fit_step(geometry=...).

Which case launches which kernel (gbuffer_bwd_launch):
  k_gbuffer_bwd_rows<4 / 8 / 12, NF>  S = 64 / 128 / 192; grid stride 32773 x 64; 2 frames x 5 rays x 192; every renderer test (S = 192)
  k_gbuffer_bwd<NF>                   every other S (1, 2: a ray shorter than a wave; 63, 65: around a segment; 193, 320: the carries across
                                      4 and 5 segments, forward for T and backward for the suffix sums); grid stride 8197 x 33; S = 64 with
                                      depths that are not 16-byte aligned

Bounds.  Kernel against float64, per gradient array (rel_err: maximum error over the array's largest float64 value): four times
gbuffer_grad_cases.FP32_WORST of the family (what the fp32 autograd of the oracle is held to on the same inputs; the ratio of the
forward pair, 5e-6 and 2e-5).  An array beyond that is held to helpers.assert_parity's rule: at least as close to float64 as the
fp32 oracle is, x1.5 + 1e-5.  Every output sits between NaN guards."""
import numpy as np
import pytest
import torch

import gbuffer_cases as gc
import gbuffer_grad_cases as gg
import test_gpu_gbuffer as fw
from helpers import bounded, record

pytestmark = pytest.mark.gpu
Out = fw.Out


@pytest.fixture(scope='module')
def L():
    from honerf_amd import lib
    return lib


@pytest.fixture(scope='module')
def lib(L):
    return L.load()


def _dev(x):
    return x.detach().to('cuda', torch.float32).contiguous()


def _outs(x):
    return {k: Out(*x[k].shape) for k in gg.WRT[x['fields']]}


def _run(L, lib, x, up, only=gg.UP, rays_d=True, z_dev=None, dev=None):
    """One launch -> {name: Out}; `only`: the upstream gradients that are passed (the others NULL); rays_d False: g_rays_d NULL."""
    N, S = x['z'].shape
    f2 = x['fields'] == 2
    names = gg.WRT[x['fields']]
    d = dev if dev is not None else {k: _dev(x[k]) for k in names + ('z',)}
    z = d['z'] if z_dev is None else z_dev
    u = {k: _dev(up[k]) for k in gg.UP}
    pu = [L.ptr(u[k]) if k in only else None for k in gg.UP]
    o = _outs(x)
    po = {k: (L.ptr(o[k].t) if (rays_d or not k.startswith('d')) else None) for k in names}
    if f2:
        rc = lib.hn_gbuffer2_bwd(L.ptr(d['sdf_h']), L.ptr(d['grad_h']), L.ptr(d['d_h']), x['inv_s_h'], L.ptr(d['sdf_o']), L.ptr(d['grad_o']),
                                 L.ptr(d['d_o']), x['inv_s_o'], L.ptr(z), x['n_frames'], x['rays_per_frame'], S, x['sample_dist'], pu[0], pu[1], pu[2],
                                 po['sdf_h'], po['grad_h'], po['sdf_o'], po['grad_o'], po['d_h'], po['d_o'], L.stream_ptr())
    else:
        rc = lib.hn_gbuffer1_bwd(L.ptr(d['sdf']), L.ptr(d['grad']), L.ptr(d['d']), L.ptr(z), N, S, x['sample_dist'], x['inv_s'], pu[0], pu[1], pu[2],
                                 po['sdf'], po['grad'], po['d'], L.stream_ptr())
    L.check(rc, 'hn_gbuffer%d_bwd' % x['fields'])
    torch.cuda.synchronize()
    return o


def _values(o, tag, rays_d=True):
    out = {}
    for k, v in o.items():
        if k.startswith('d') and not rays_d:
            v.untouched('%s %s (NULL)' % (tag, k))
        else:
            out[k] = v.check('%s %s' % (tag, k))
    return out


def _check(got, r64, r32, family, tag):
    bound = gg.GPU_FACTOR * gg.FP32_WORST[family]
    for k, v in got.items():
        e = gg.rel_err(v.numpy(), r64[k].numpy())
        what = '%s: %s' % (tag, k)
        if e <= bound:
            record(what, e, bound)
            continue
        e_ref = gg.rel_err(r32[k].numpy(), r64[k].numpy())
        print('%s: %.3e from float64 (bound %.1e); the fp32 oracle is %.3e from it' % (what, e, bound, e_ref))
        bounded(what, e, 1.5 * e_ref + 1e-5, kind='rel, conditioning-aware', ref32_vs_fp64=e_ref)


def _cases(S):
    return [c for c in gc.all_cases() if c[2] == S]


# ---- the kernels, case by case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', list(gg.FAMILIES))
@pytest.mark.parametrize('S', gc.S_ALL)
@pytest.mark.parametrize('fields', (2, 1))
def test_gbuffer_bwd(L, lib, fields, S, family):
    for n_frames, n_rays, _ in _cases(S):
        if fields == 1 and n_frames != 1:
            continue
        x, up, r64, r32 = gg.case(n_frames, n_rays, S, family, fields)
        tag = 'hn_gbuffer%d_bwd %d x %d x %d %s' % (fields, n_frames, n_rays, S, family)
        _check(_values(_run(L, lib, x, up), tag), r64, r32, family, tag)


@pytest.mark.parametrize('family', list(gg.FAMILIES))
@pytest.mark.parametrize('n_rays,S', gc.GRID)
@pytest.mark.parametrize('fields', (2, 1))
def test_gbuffer_bwd_grid_stride(L, lib, fields, n_rays, S, family):
    x, up, r64, r32 = gg.case(1, n_rays, S, family, fields)
    tag = 'hn_gbuffer%d_bwd grid stride %d x %d %s' % (fields, n_rays, S, family)
    _check(_values(_run(L, lib, x, up), tag), r64, r32, family, tag)


@pytest.mark.parametrize('family', list(gg.FAMILIES))
def test_gbuffer2_bwd_misaligned_depths(L, lib, family):
    """S = 64 with depths 4 bytes off a 16-byte boundary: the generic kernel, the same values."""
    n_frames, n_rays, S = gg.MISALIGNED
    x, up, r64, r32 = gg.case(n_frames, n_rays, S, family, 2)
    buf = torch.empty(n_rays * S + 1, device='cuda')
    z = buf[1:].view(n_rays, S)
    z.copy_(x['z'])
    assert z.data_ptr() % 16 == 4
    tag = 'hn_gbuffer2_bwd S=64 misaligned z %s' % family
    _check(_values(_run(L, lib, x, up, z_dev=z), tag), r64, r32, family, tag)


@pytest.mark.parametrize('fields', (2, 1))
@pytest.mark.parametrize('S', gc.S_ALL)
def test_gbuffer_bwd_saturated_inputs_stay_finite(L, lib, S, fields):
    """The forward suite's surface family (inv_s 3000: alphas of exactly 1, factors of 1e-7, sigmoids at 0 and 1): every output is
    written and finite (Out.check: no NaN; and no infinity)."""
    for n_frames, n_rays, _ in _cases(S):
        if fields == 1 and n_frames != 1:
            continue
        x = gg.inputs(n_frames, n_rays, S, 'surface', fields)
        got = _values(_run(L, lib, x, gg.upstream(x)), 'hn_gbuffer%d_bwd surface S=%d' % (fields, S))
        assert all(bool(torch.isfinite(v).all()) for v in got.values())


# ---- NULL upstream / NULL output combinations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fields', (2, 1))
@pytest.mark.parametrize('S', gc.ARG_S)
def test_gbuffer_bwd_null_arguments(L, lib, S, fields):
    """One buffer's upstream gradient alone gives the bits of the full call with the other two zero; g_rays_d NULL changes no other
    output's bits and leaves those buffers alone."""
    x, up, r64, r32 = gg.case(1, gc.ARG_RAYS, S, 'thin', fields)
    tag = 'hn_gbuffer%d_bwd S=%d' % (fields, S)
    full = _values(_run(L, lib, x, up), tag)
    for k in gg.UP:
        alone = _values(_run(L, lib, x, up, only=(k,)), '%s only g_%s' % (tag, k))
        zeroed = {n: (v if n == k else torch.zeros_like(v)) for n, v in up.items()}
        same = _values(_run(L, lib, x, zeroed), '%s g_%s and zeros' % (tag, k))
        for n in alone:
            assert torch.equal(alone[n], same[n]), '%s: %s with only g_%s differs from the call with zeros' % (tag, n, k)
        ref = gg.reference(x, up, torch.float64, only=(k,))
        for n in alone:
            e = gg.rel_err(alone[n].numpy(), ref[n].numpy())
            bounded('%s only g_%s: %s' % (tag, k, n), e, gg.GPU_FACTOR * gg.FP32_WORST['thin'])
    part = _values(_run(L, lib, x, up, rays_d=False), tag + ' g_rays_d NULL', rays_d=False)
    for n, v in part.items():
        assert torch.equal(v, full[n]), '%s: %s changes when g_rays_d is NULL' % (tag, n)


def test_gbuffer_bwd_refusals(L, lib):
    """S = 0, a negative count, a NULL input or required output, and all three upstream gradients NULL are HN_EINVAL with a message;
    no rays is a no-op that returns 0.  Nothing is launched: the outputs stay NaN."""
    x2 = gg.inputs(1, 5, 64, 'thin', 2)
    x1 = gg.inputs(1, 5, 64, 'thin', 1)
    up2, up1 = gg.upstream(x2), gg.upstream(x1)
    d2 = {k: _dev(x2[k]) for k in gg.WRT[2] + ('z',)}
    d1 = {k: _dev(x1[k]) for k in gg.WRT[1] + ('z',)}
    u2, u1 = {k: _dev(v) for k, v in up2.items()}, {k: _dev(v) for k, v in up1.items()}
    o2, o1 = _outs(x2), _outs(x1)

    def call2(S=64, n_frames=1, P=5, null=()):
        a = {k: (None if k in null else L.ptr(v)) for k, v in d2.items()}
        g = {k: (None if 'g_' + k in null else L.ptr(v)) for k, v in u2.items()}
        q = {k: (None if 'o_' + k in null else L.ptr(v.t)) for k, v in o2.items()}
        return lib.hn_gbuffer2_bwd(a['sdf_h'], a['grad_h'], a['d_h'], x2['inv_s_h'], a['sdf_o'], a['grad_o'], a['d_o'], x2['inv_s_o'], a['z'], n_frames, P, S,
                                   x2['sample_dist'], g['opacity'], g['depth'], g['normal'], q['sdf_h'], q['grad_h'], q['sdf_o'], q['grad_o'], q['d_h'],
                                   q['d_o'], L.stream_ptr())

    def call1(S=64, N=5, null=()):
        a = {k: (None if k in null else L.ptr(v)) for k, v in d1.items()}
        g = {k: (None if 'g_' + k in null else L.ptr(v)) for k, v in u1.items()}
        q = {k: (None if 'o_' + k in null else L.ptr(v.t)) for k, v in o1.items()}
        return lib.hn_gbuffer1_bwd(a['sdf'], a['grad'], a['d'], a['z'], N, S, x1['sample_dist'], x1['inv_s'], g['opacity'], g['depth'], g['normal'],
                                   q['sdf'], q['grad'], q['d'], L.stream_ptr())

    all_up = ('g_opacity', 'g_depth', 'g_normal')
    for call, word in ((lambda: call2(S=0), 'S = 0'), (lambda: call1(S=0), 'S = 0'), (lambda: call2(P=-1), '-1'), (lambda: call1(N=-1), '-1'),
                       (lambda: call2(null=('grad_o',)), 'NULL'), (lambda: call2(null=('z',)), 'NULL'), (lambda: call1(null=('sdf',)), 'NULL'),
                       (lambda: call1(null=('d',)), 'NULL'), (lambda: call2(null=('o_sdf_o',)), 'required'), (lambda: call1(null=('o_grad',)), 'required'),
                       (lambda: call2(null=all_up), 'upstream'), (lambda: call1(null=all_up), 'upstream')):
        assert call() == -1
        msg = lib.hn_last_error().decode()
        assert word in msg and 'hn_gbuffer' in msg and '_bwd' in msg, msg
    assert call2(P=0) == 0 and call2(n_frames=0) == 0 and call1(N=0) == 0
    assert call2(P=0, null=('sdf_h', 'z') + all_up) == 0, 'no rays: the arguments are not looked at'
    torch.cuda.synchronize()
    for o in (o1, o2):
        for k, v in o.items():
            v.untouched('a refused / empty call: ' + k)


@pytest.mark.parametrize('fields', (2, 1))
@pytest.mark.parametrize('S', (192, 193))
def test_gbuffer_bwd_repeats_and_other_stream(L, lib, S, fields):
    """No atomics: two calls give identical bits, and so does a call on a current stream that is not the default one."""
    x, up, _, _ = gg.case(1, 37, S, 'soft', fields)
    tag = 'hn_gbuffer%d_bwd S=%d' % (fields, S)
    a = _values(_run(L, lib, x, up), tag)
    b = _values(_run(L, lib, x, up), tag + ' again')
    side = torch.cuda.Stream()
    dev = {k: _dev(x[k]) for k in gg.WRT[fields] + ('z',)}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert L.stream_ptr().value == side.cuda_stream
        c = _values(_run(L, lib, x, up, dev=dev), tag + ' on a side stream')
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), '%s: %s differs between calls' % (tag, k)


# ---- autograd.gbuffer1 / gbuffer2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', (128, 65))
def test_autograd_gbuffer2(L, lib, S):
    """Forward: hn_gbuffer2's bits with Ro = NULL; backward: the raw launch's bits; an unused buffer costs nothing (None upstream);
    the depths get no gradient."""
    from honerf_amd import autograd as A
    x, up, _, _ = gg.case(1, 37, S, 'soft', 2)
    leaves = {k: _dev(x[k]).requires_grad_(True) for k in gg.WRT[2]}
    z = _dev(x['z']).requires_grad_(True)
    op, dp, nr = A.gbuffer2(leaves['sdf_h'].reshape(-1, 1), leaves['grad_h'].reshape(-1, 3), leaves['d_h'], x['inv_s_h'], leaves['sdf_o'].reshape(-1, 1),
                            leaves['grad_o'].reshape(-1, 3), leaves['d_o'], x['inv_s_o'], z, 1, x['sample_dist'])
    raw = fw._run2(L, lib, x, with_Ro=False)
    for k, v in (('opacity', op), ('depth', dp), ('normal', nr)):
        assert torch.equal(v.detach().cpu(), raw[k].check(k)), 'autograd.gbuffer2: %s is not hn_gbuffer2\'s' % k
    u = {k: _dev(v) for k, v in up.items()}
    ((op * u['opacity']).sum() + (dp * u['depth']).sum() + (nr * u['normal']).sum()).backward(retain_graph=True)
    want = _values(_run(L, lib, x, up), 'raw')
    for k in gg.WRT[2]:
        assert leaves[k].grad.shape == leaves[k].shape and torch.equal(leaves[k].grad.cpu(), want[k]), 'autograd.gbuffer2: d / d %s is not the raw launch\'s' % k
    assert z.grad is None
    for v in leaves.values():
        v.grad = None
    (dp * u['depth']).sum().backward()
    want = _values(_run(L, lib, x, up, only=('depth',)), 'raw, depth only')
    for k in gg.WRT[2]:
        assert torch.equal(leaves[k].grad.cpu(), want[k]), 'autograd.gbuffer2 (depth only): d / d %s' % k


@pytest.mark.parametrize('S', (64, 2))
def test_autograd_gbuffer1(L, lib, S):
    from honerf_amd import autograd as A
    x, up, _, _ = gg.case(1, 37, S, 'thin', 1)
    leaves = {k: _dev(x[k]).requires_grad_(True) for k in gg.WRT[1]}
    op, dp, nr = A.gbuffer1(leaves['sdf'], leaves['grad'], leaves['d'], x['inv_s'], _dev(x['z']), x['sample_dist'])
    raw = fw._run1(L, lib, x)
    for k, v in (('opacity', op), ('depth', dp), ('normal', nr)):
        assert torch.equal(v.detach().cpu(), raw[k].check(k)), 'autograd.gbuffer1: %s is not hn_gbuffer1\'s' % k
    u = {k: _dev(v) for k, v in up.items()}
    ((op * u['opacity']).sum() + (dp * u['depth']).sum() + (nr * u['normal']).sum()).backward()
    want = _values(_run(L, lib, x, up), 'raw')
    for k in gg.WRT[1]:
        assert torch.equal(leaves[k].grad.cpu(), want[k]), 'autograd.gbuffer1: d / d %s is not the raw launch\'s' % k
    only_sdf = _dev(x['sdf']).requires_grad_(True)
    op2, _, _ = A.gbuffer1(only_sdf, _dev(x['grad']), _dev(x['d']), x['inv_s'], _dev(x['z']), x['sample_dist'])
    op2.sum().backward()
    assert only_sdf.grad is not None and bool(torch.isfinite(only_sdf.grad).all())


# ---- render_buffers(graph=True) -----------------------------------------------------------------------------------------------------------
BUFFERS = ('opacity_hand', 'opacity_obj', 'depth_hand', 'depth_obj', 'depth', 'normal_hand', 'normal_obj', 'normal')
ROTATED = ('normal_obj', 'normal')        # the object's normal goes to the world frame by a torch operator with graph=True, inside the kernel without


def _frames(F, P, seed):
    frames = [fw._scene(P, seed + f) for f in range(F)]
    return tuple(torch.stack([fr[i] for fr in frames]) for i in range(6))


def _scene_args(batched, F, P, seed):
    if batched:
        o, d, bt_inv, T_pose, Ro, To = _frames(F, P, seed)
        t_rand = torch.rand(F, P, 1, generator=torch.Generator().manual_seed(9)).cuda()
    else:
        o, d, bt_inv, T_pose, Ro, To, _ = fw._scene(P, seed)
        t_rand = torch.rand(P, 1, generator=torch.Generator().manual_seed(8)).cuda()
    return o, d, bt_inv, T_pose, Ro, To, t_rand


@pytest.mark.parametrize('batched', (False, True))
def test_render_buffers_graph_values(batched):
    """graph=True with every input detached: no graph is built, and the keys, shapes and values are graph=False's (to the bit, but for
    the object's world normal, rotated by a torch operator: within 1e-6 absolute).  With inputs that require grad the default still
    refuses; graph=True returns the same keys and shapes attached to the graph.  `render` itself then runs its differentiable form
    (the taped final evaluation), whose per-sample values are not graph=False's to the bit: the attached buffers are held to the
    float64 restatement on that render's own per-sample outputs and depths, as test_gpu_gbuffer holds graph=False's (2e-5), and the
    distance of the two renders' sdf is printed."""
    F, P = (2, 5) if batched else (1, 37)
    o, d, bt_inv, T_pose, Ro, To, t_rand = _scene_args(batched, F, P, 30 if batched else 13)
    ren = fw._dual(batched)
    plain = ren.render_buffers(o, d, fw.NEAR, fw.FAR, bt_inv, T_pose, None, Ro, To, t_rand=t_rand)
    detached = ren.render_buffers(o, d, fw.NEAR, fw.FAR, bt_inv, T_pose, None, Ro, To, t_rand=t_rand, graph=True)
    assert set(detached) == set(plain)
    assert all(not v.requires_grad and v.grad_fn is None for v in detached.values() if isinstance(v, torch.Tensor)), 'detached inputs: no graph'
    leaves = [x.clone().requires_grad_(True) for x in (bt_inv, Ro, To)]
    with pytest.raises(ValueError, match='render'):
        ren.render_buffers(o, d, fw.NEAR, fw.FAR, leaves[0], T_pose, None, leaves[1], leaves[2], t_rand=t_rand)
    out = ren.render_buffers(o, d, fw.NEAR, fw.FAR, leaves[0], T_pose, None, leaves[1], leaves[2], t_rand=t_rand, graph=True)
    assert set(out) == set(plain)
    name = 'batched' if batched else 'fitting'
    for k in BUFFERS + ('color_fine', 'weight_sum', 'sdf_hand', 'sdf_obj', 'gradient_hand', 'gradient_obj'):
        assert detached[k].shape == plain[k].shape == out[k].shape, (k, detached[k].shape, out[k].shape, plain[k].shape)
        if k in ROTATED:
            bounded('render_buffers(graph=True) %s detached: %s against graph=False (absolute)' % (name, k),
                    float((detached[k] - plain[k]).abs().max()), 1e-6, kind='abs')
        else:
            assert torch.equal(detached[k], plain[k]), 'render_buffers(graph=True), detached inputs: %s differs from graph=False' % k
    print('render_buffers(graph=True) %s attached: sdf_hand is %.3e (absolute) from graph=False\'s: the taped against the untaped evaluation'
          % (name, float((out['sdf_hand'].detach() - plain['sdf_hand']).abs().max())))
    ref = fw._dual_reference(ren, {k: v.detach() for k, v in out.items()}, d, Ro, F, P)
    for k, v in ref.items():
        fw._close(out[k], v.reshape(out[k].shape), 'render_buffers(graph=True) %s attached: %s' % (name, k))
    assert all(out[k].requires_grad for k in BUFFERS)
    assert float(plain['opacity_hand'].max()) > 0.05 and float(plain['opacity_obj'].max()) > 0.05, 'the rays must see both fields'


# the bounds of test_gpu_parity.REF_DEPTH_GRAD for the same inputs (gradients through a render on given depths against the fp32
# reference's gradients), copied
REF_DEPTH_GRAD = {'Ro': 1e-4, 'To': 1e-4, 'bt_inv': 1.9e-3}


def _oracle_buffer_grads(fields, o, d, bt_inv, T_pose, Ro, To, z, up, dtype, batched, inv_s):
    """autograd of sum(up * buffers) through the oracle's fields at the depths z -> gradients w.r.t. (bt_inv, Ro, To)."""
    from oracle import render as orr
    hand, obj = fields
    c = lambda x: x.detach().cpu().to(dtype)
    leaves = [c(x).clone().requires_grad_(True) for x in (bt_inv, Ro, To)]
    ro, rd, tp, zz = c(o), c(d), c(T_pose), c(z).reshape(*o.shape[:-1], -1)
    sample_dist = float(gc.f32_scalar((fw.FAR - fw.NEAR) / fw.N_SAMPLES))
    o_o, d_o = orr.obj_local(ro, rd, leaves[1], leaves[2], repeat=True)
    _, _, sdf_h, _, g_h = orr._alpha_sample_color(hand, ro, rd, zz, sample_dist, leaves[0], tp, batched)
    _, _, sdf_o, _, g_o = orr._alpha_sample_color(obj, o_o, d_o, zz, sample_dist, leaves[0], tp, batched)
    F, P = (o.shape[0], o.shape[1]) if batched else (1, o.shape[0])
    N, S = F * P, zz.shape[-1]
    x = {'sdf_h': sdf_h.reshape(N, S), 'grad_h': g_h.reshape(N, S, 3), 'sdf_o': sdf_o.reshape(N, S), 'grad_o': g_o.reshape(N, S, 3),
         'd_h': rd.reshape(N, 3), 'd_o': d_o.reshape(N, 3), 'z': zz.reshape(N, S), 'Ro': leaves[1].reshape(F, 3, 3), 'inv_s_h': inv_s[0], 'inv_s_o': inv_s[1],
         'sample_dist': sample_dist, 'n_frames': F, 'rays_per_frame': P, 'S': S, 'fields': 2}
    r = gc.oracle(x, dtype)
    total = sum((c(up[k]).reshape(r[k].shape) * r[k]).sum() for k in gg.UP)
    return dict(zip(('bt_inv', 'Ro', 'To'), torch.autograd.grad(total, leaves)))


@pytest.mark.parametrize('batched', (False, True))
def test_gradients_through_the_render(batched):
    """d sum(upstream * buffers) / d (bt_inv, Ro, To) through render_buffers(graph=True) -- DualRenderFn, ObjLocalFn, gbuffer2 and the
    normal's rotation -- against the fp32 oracle's autograd of the same composition at the product's own final depths (last_z_vals),
    to test_gpu_parity.REF_DEPTH_GRAD's bounds; the float64 oracle's figures go to the report beside them."""
    from helpers import oracle_fields, oracle_fields_fp64
    F, P = (2, 16) if batched else (1, 32)
    o, d, bt_inv, T_pose, Ro, To, t_rand = _scene_args(batched, F, P, 30 if batched else 13)
    ren = fw._dual(batched)
    leaves = {k: v.clone().requires_grad_(True) for k, v in (('bt_inv', bt_inv), ('Ro', Ro), ('To', To))}
    out = ren.render_buffers(o, d, fw.NEAR, fw.FAR, leaves['bt_inv'], T_pose, None, leaves['Ro'], leaves['To'], t_rand=t_rand, graph=True)
    N = F * P
    g = torch.Generator().manual_seed(21)
    up = {'opacity': torch.randn(N, 2, generator=g), 'depth': torch.randn(N, 2, generator=g), 'normal': torch.randn(N, 2, 3, generator=g)}
    u = {k: v.cuda() for k, v in up.items()}
    total = sum((out[k + '_hand'].reshape(N, -1) * u[k][:, 0].reshape(N, -1)).sum() + (out[k + '_obj'].reshape(N, -1) * u[k][:, 1].reshape(N, -1)).sum()
                for k in gg.UP)
    total.backward()
    z = ren.last_z_vals
    hand, obj = ren.fields()
    inv_s = (gc.f32_scalar(hand.inv_s), gc.f32_scalar(obj.inv_s))
    r32 = _oracle_buffer_grads(oracle_fields(), o, d, bt_inv, T_pose, Ro, To, z, up, torch.float32, batched, inv_s)
    r64 = _oracle_buffer_grads(oracle_fields_fp64(), o, d, bt_inv, T_pose, Ro, To, z, up, torch.float64, batched, inv_s)
    sel = lambda name, x: x[..., :3, :] if name == 'bt_inv' else x
    tag = 'batched 2 x 16' if batched else 'fitting 32'
    for k in ('bt_inv', 'Ro', 'To'):
        got = sel(k, leaves[k].grad.detach().cpu()).numpy()
        e32, e64 = gg.rel_err(got, sel(k, r32[k]).numpy()), gg.rel_err(got, sel(k, r64[k]).numpy())
        print('d buffers / d %s (%s): %.3e from the fp32 oracle, %.3e from float64; the fp32 oracle is %.3e from float64'
              % (k, tag, e32, e64, gg.rel_err(sel(k, r32[k]).numpy(), sel(k, r64[k]).numpy())))
        bounded('d sum(upstream * buffers) / d %s through render_buffers(graph=True), %s' % (k, tag), e32, REF_DEPTH_GRAD[k], hip_vs_fp64=e64)


# ---- the loss terms and the fitting step ---------------------------------------------------------------------------------------------------
def test_geometry_loss_terms_on_the_device():
    from honerf_amd import fitting as F
    rng = np.random.RandomState(6)
    P = 53
    b = {k: rng.uniform(0.0, 1.0, size=(P, 1)).astype(np.float32) for k in ('opacity_hand', 'opacity_obj')}
    b['opacity_hand'][:2, 0] = (0.0, 1.0)
    b.update({k: rng.uniform(0.0, 1.2, size=(P, 1)).astype(np.float32) for k in ('depth_hand', 'depth_obj')})
    td = rng.uniform(0.4, 1.5, size=P).astype(np.float32)
    td[::3] = 0.0
    lab = rng.randint(0, 3, size=P).astype(np.uint8)
    got = F.geometry_loss_terms({k: torch.from_numpy(v).cuda() for k, v in b.items()}, torch.from_numpy(td).cuda(), torch.from_numpy(lab).cuda())
    d = {k: v.astype(np.float64)[:, 0] for k, v in b.items()}
    valid = td > 0
    want = {'depth': np.abs(d['depth_hand'] + d['depth_obj'] - (d['opacity_hand'] + d['opacity_obj']) * td.astype(np.float64))[valid].mean()}
    for k, o, l in (('mask_hand', d['opacity_hand'], 1), ('mask_obj', d['opacity_obj'], 2)):
        c, y = np.clip(o, 1e-3, 1.0 - 1e-3), (lab == l).astype(np.float64)
        want[k] = -(y * np.log(c) + (1.0 - y) * np.log(1.0 - c)).mean()
    assert sorted(got) == sorted(want)
    for k in want:      # fp32 sums of 53 terms of order 1: 53 half-ulps at most, 4e-6 relative
        bounded('geometry_loss_terms: %s against float64 numpy' % k, abs(float(got[k]) - want[k]) / abs(want[k]), 4e-6)


def _fit_scene(seed=5, rays=24, with_geometry=True, ren=None):
    from honerf_amd import fitting as F, synth
    bt, tp, j = synth.synth_hand_pose(seed)
    R, tt = synth.synth_obj_pose(seed + 1, center=tuple(j[9] + np.array([0.02, 0.0, 0.01])))
    rng = np.random.RandomState(seed)
    u = rng.standard_normal((400, 3))
    verts = (u / np.linalg.norm(u, axis=1, keepdims=True) * 0.02).astype(np.float32)
    chain = F.RigidPoseChain(bt[None], tp[None], j[None], R[None], tt[None], verts)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().cuda()
    geo = dict(renderer=ren, near=0.4, far=1.5, bt_inv=c(bt), T_pose_21=c(tp), Ro=c(R).T.contiguous(), To=c(tt), opacity_threshold=0.1) if with_geometry else None
    views = F.synthetic_views(2, 1, rays, seed, j[9], with_geometry=geo)
    return chain, views


def test_fit_step_with_geometry():
    """fit_step(geometry=...): the extra terms come back, and the pose gradients are autograd's of step_loss + the weighted terms
    assembled by hand from render_buffers(graph=True) on the same jitter."""
    from honerf_amd import fitting as F
    ren = fw._dual(False)
    chain, views = _fit_scene(ren=ren)
    view = views[0]
    assert view['true_depth'].shape == (24,) and view['true_label'].shape == (24,) and view['true_label'].dtype == torch.uint8
    assert bool(((view['true_depth'] > 0) == (view['true_label'] > 0)).all()) and int((view['true_label'] > 0).sum()) > 0
    geometry = dict(depth_weight=3.0, mask_weight=0.25)
    t_rand = torch.rand(24, 1, generator=torch.Generator().manual_seed(3)).cuda()
    terms = F.fit_backward(ren, view, chain, 0.4, 1.5, '12', t_rand=t_rand, geometry=geometry)
    assert {'depth', 'mask_hand', 'mask_obj', 'loss', 'color', 'mask', 'contact', 'penetration'} <= set(terms)
    assert all(bool(torch.isfinite(v).all()) for v in terms.values())
    got = [p.grad.detach().clone() for p in chain.parameters()]
    # by hand
    for p in chain.parameters():
        p.grad = None
    pose = chain(None)
    from honerf_amd import lib as L_
    rays_o, rays_d = F._rays(L_, view['xy'], view['cam'], 1, 24)
    first = lambda x: x.reshape(x.shape[1:])
    out = ren.render_buffers(rays_o, rays_d, 0.4, 1.5, first(pose['bt_inv']), first(pose['T_pose_21']), None, first(pose['obj_r']).T, first(pose['obj_t']),
                             t_rand=t_rand, graph=True)
    base = F.step_loss(out, view['true_rgb'], view['true_mask'], pose, '12')
    gt = F.geometry_loss_terms(out, view['true_depth'], view['true_label'])
    loss = base['loss'] + ((3.0 * gt['depth'] + 0.25 * gt['mask_hand']) + 0.25 * gt['mask_obj'])      # fit_backward's association
    loss.backward()
    for k in ('depth', 'mask_hand', 'mask_obj'):
        assert torch.equal(terms[k].detach(), gt[k].detach()), k
    assert torch.equal(terms['loss'].detach(), loss.detach())
    for a, p in zip(got, chain.parameters()):
        assert torch.equal(a, p.grad), 'fit_step(geometry=...): a pose gradient differs from the hand-assembled loss\'s'
    base_only = sum(float(p.grad.abs().sum()) for p in chain.parameters())
    assert base_only > 0
    # the terms do contribute: without them the gradient differs
    F.fit_backward(ren, view, chain, 0.4, 1.5, '12', t_rand=t_rand)
    assert any(not torch.equal(a, p.grad) for a, p in zip(got, chain.parameters()))
    # a view without the targets: geometry changes nothing
    chain2, plain_views = _fit_scene(with_geometry=False)
    a = F.fit_backward(ren, plain_views[0], chain2, 0.4, 1.5, '12', t_rand=t_rand, geometry=geometry)
    assert 'depth' not in a and 'mask_hand' not in a


def test_fit_step_without_geometry_is_unchanged():
    """geometry=None: two runs of the same steps from the same start give the same bits (the suite's reproducibility of fit_step,
    test_gpu_surface), with and without an explicit geometry=None."""
    from honerf_amd import fitting as F
    ren = fw._dual(False)
    finals = []
    for kwargs in ({}, {'geometry': None}):
        chain, views = _fit_scene(with_geometry=False)
        opt = F.make_optimizer(chain)
        for k in range(3):
            t_rand = torch.rand(24, 1, generator=torch.Generator().manual_seed(40 + k)).cuda()
            terms = F.fit_step(ren, views[k % 2], chain, opt, 0.4, 1.5, '12', t_rand=t_rand, **kwargs)
        torch.cuda.synchronize()
        finals.append(([p.detach().clone() for p in chain.parameters()], {k: v.detach().clone() for k, v in terms.items()}))
    for a, b in zip(finals[0][0], finals[1][0]):
        assert torch.equal(a, b)
    assert set(finals[0][1]) == set(finals[1][1]) == {'loss', 'color', 'mask', 'contact', 'penetration', 'joint', 'obj_verts'}
    for k in ('color', 'mask', 'contact', 'penetration', 'joint', 'obj_verts'):
        assert torch.equal(finals[0][1][k], finals[1][1][k]), k


def test_graphless_drivers_refuse_geometry():
    from honerf_amd import fitting as F
    geometry = dict(depth_weight=1.0, mask_weight=1.0)
    with pytest.raises(ValueError, match='fit_step'):
        F.PipelinedSingleFit(None, None, None, 0.4, 1.5, '12', geometry=geometry)
    with pytest.raises(ValueError, match='fit_step'):
        F.PipelinedSingleFit.step(None, None, geometry=geometry)
    with pytest.raises(ValueError, match='fit_step'):
        F.fit_frames_batched(None, [], 0.4, 1.5, geometry=geometry)
    with pytest.raises(ValueError, match='fit_step'):
        F.step_loss({}, None, None, {}, geometry=geometry)
    with pytest.raises(ValueError, match='depth_weight'):
        F._geometry_weights(dict(depth=1.0))
