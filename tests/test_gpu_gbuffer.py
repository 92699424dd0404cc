"""GPU tests of the geometry buffers: the kernels of ho-nerf_amd/csrc/hn_gbuffer.hip through the C ABI (hn_gbuffer1 / hn_gbuffer2)
against the definition run in float64 on the same fp32 inputs (tests/gbuffer_cases.py: the inputs, the reference and the shape
tables; tests/test_gbuffer_cpu.py: the fp32 oracle is within 5e-6 of float64 on every one of these inputs), then the Python surface
on top of them: `render_buffers` of the three renderer classes and `harness.render_view_buffers`.

Which case launches which kernel (gbuffer_launch):
  k_gbuffer_rows<4, NF>   test_gbuffer*[S=64], grid stride 32773 x 64, test_gbuffer*_null_outputs[64], error / no-op cases
  k_gbuffer_rows<8, NF>   test_gbuffer*[S=128]
  k_gbuffer_rows<12, NF>  test_gbuffer*[S=192], 2 frames x 5 rays (NF = 2), the golden, every renderer test
  k_gbuffer<NF>           test_gbuffer*[every other S], grid stride 8197 x 33, test_gbuffer*_null_outputs[65],
                          test_gbuffer2_misaligned_depths (S = 64 from a buffer that is not 16-byte aligned)

Every output is a view into a NaN-filled flat tensor with GUARD NaN floats in front of it and behind it (test_gpu_composite.Out's
pattern): after the launch the guards are still NaN and the output holds no NaN; an output passed as NULL is NaN throughout."""
import numpy as np
import pytest
import torch

import gbuffer_cases as gc
from helpers import assert_close, bounded

pytestmark = pytest.mark.gpu

# Against float64: four times the 5e-6 the fp32 oracle is held to on the same inputs (test_gbuffer_cpu.py), the project's ratio for
# these stages (test_gpu_composite.RT).  Observed on MI355X (worst over all cases of an entry point;
# profiles/gbuffer/parity_report.json has every row):
#   hn_gbuffer1 3.7e-6 (depth, S = 320 thin)                 hn_gbuffer2 3.5e-6 (depth, S = 320 thin)
#   the golden 1.9e-6 (depth)                                render_view_buffers' depth 9.9e-8
#   render_buffers: hand 1.9e-6, obj 1.2e-6 (opacity)        fitting 6.7e-6 (opacity_hand), batched 6.8e-6 (normal_hand)
# The thin family at the largest S leads, as in test_gpu_composite: fp32's 1 - a + 1e-7 is +1.9e-8 off per factor.
RT = 2e-5
GUARD = 64


@pytest.fixture(scope='module')
def L():
    from honerf_amd import lib
    return lib


@pytest.fixture(scope='module')
def lib(L):
    return L.load()


def _dev(x):
    return x.detach().to('cuda', torch.float32).contiguous()


class Out:
    """An output buffer of `shape` inside a NaN-filled flat tensor, GUARD NaN floats in front and GUARD behind."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.flat = torch.full((GUARD + self.n + GUARD,), float('nan'), device='cuda')
        self.t = self.flat[GUARD:GUARD + self.n].view(*shape)

    def check(self, what):
        assert bool(torch.isnan(self.flat[:GUARD]).all()) and bool(torch.isnan(self.flat[GUARD + self.n:]).all()), what + ': wrote outside its buffer'
        assert not bool(torch.isnan(self.t).any()), what + ': left part of its output unwritten (or wrote NaN)'
        return self.t.cpu()

    def untouched(self, what):
        assert bool(torch.isnan(self.flat).all()), what + ': wrote a buffer it must leave alone'


KEYS = ('opacity', 'depth', 'normal')


def _outs(N, fields):
    return {'opacity': Out(N, 2), 'depth': Out(N, 2), 'normal': Out(N, 2, 3)} if fields == 2 else \
        {'opacity': Out(N), 'depth': Out(N), 'normal': Out(N, 3)}


def _run2(L, lib, x, want=KEYS, with_Ro=True, z_dev=None):
    N, S = x['z'].shape
    d = {k: _dev(x[k]) for k in ('sdf_h', 'grad_h', 'd_h', 'sdf_o', 'grad_o', 'd_o', 'z', 'Ro')}
    z = d['z'] if z_dev is None else z_dev
    o = _outs(N, 2)
    p = {k: (L.ptr(o[k].t) if k in want else None) for k in KEYS}
    L.check(lib.hn_gbuffer2(L.ptr(d['sdf_h']), L.ptr(d['grad_h']), L.ptr(d['d_h']), x['inv_s_h'], L.ptr(d['sdf_o']), L.ptr(d['grad_o']),
                            L.ptr(d['d_o']), x['inv_s_o'], L.ptr(z), x['n_frames'], x['rays_per_frame'], S, x['sample_dist'],
                            L.ptr(d['Ro']) if with_Ro else None, p['opacity'], p['depth'], p['normal'], L.stream_ptr()), 'hn_gbuffer2')
    torch.cuda.synchronize()
    return o


def _run1(L, lib, x, want=KEYS):
    N, S = x['z'].shape
    d = {k: _dev(x[k]) for k in ('sdf', 'grad', 'd', 'z')}
    o = _outs(N, 1)
    p = {k: (L.ptr(o[k].t) if k in want else None) for k in KEYS}
    L.check(lib.hn_gbuffer1(L.ptr(d['sdf']), L.ptr(d['grad']), L.ptr(d['d']), L.ptr(d['z']), N, S, x['sample_dist'], x['inv_s'],
                            p['opacity'], p['depth'], p['normal'], L.stream_ptr()), 'hn_gbuffer1')
    torch.cuda.synchronize()
    return o


def _check(o, ref, tag, ctx, want=KEYS):
    for k in KEYS:
        if k not in want:
            o[k].untouched('%s %s (NULL)' % (tag, k))
            continue
        try:
            assert_close(o[k].check('%s %s' % (tag, k)).reshape(ref[k].shape), ref[k], RT, '%s: %s' % (tag, k))
        except AssertionError as e:
            raise AssertionError('%s [%s]' % (e, ctx)) from None


# ---- the kernels, case by case ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', list(gc.FAMILIES))
@pytest.mark.parametrize('S', gc.S_ALL)
def test_gbuffer2(L, lib, S, family):
    for n_rays in gc.RAYS:
        x = gc.inputs(1, n_rays, S, family, 2)
        _check(_run2(L, lib, x), gc.oracle(x, torch.float64), 'hn_gbuffer2 S=%d %s' % (S, family), '%d rays' % n_rays)


@pytest.mark.parametrize('family', list(gc.FAMILIES))
@pytest.mark.parametrize('S', gc.S_ALL)
def test_gbuffer1(L, lib, S, family):
    for n_rays in gc.RAYS:
        x = gc.inputs(1, n_rays, S, family, 1)
        _check(_run1(L, lib, x), gc.oracle(x, torch.float64), 'hn_gbuffer1 S=%d %s' % (S, family), '%d rays' % n_rays)


@pytest.mark.parametrize('family', list(gc.FAMILIES))
def test_gbuffer2_frames(L, lib, family):
    """Two frames, each with its own Ro; and Ro = NULL leaves the object's normal in the object's frame."""
    x = gc.inputs(*gc.FRAMES_CASE, family, 2)
    tag = 'hn_gbuffer2 %d frames x %d rays S=%d %s' % (gc.FRAMES_CASE + (family,))
    _check(_run2(L, lib, x), gc.oracle(x, torch.float64), tag, '')
    _check(_run2(L, lib, x, with_Ro=False), gc.oracle(x, torch.float64, rotate=False), tag + ' Ro NULL', '')
    one = gc.oracle(dict(x, Ro=x['Ro'][:1].expand(2, 3, 3)), torch.float64)['normal'][:, 1]     # (what one Ro for both frames would give)
    assert gc.rel_err(one.numpy(), gc.oracle(x, torch.float64)['normal'][:, 1].numpy()) > 0.1, 'the two frames do not tell their Ro apart'


@pytest.mark.parametrize('family', ('surface', 'thin'))
@pytest.mark.parametrize('n_rays,S', gc.GRID)
def test_gbuffer_grid_stride(L, lib, n_rays, S, family):
    """More rays than 2048 blocks take in one pass: every block loops, the last pass is partial."""
    x = gc.inputs(1, n_rays, S, family, 2)
    _check(_run2(L, lib, x), gc.oracle(x, torch.float64), 'hn_gbuffer2 grid stride %d x %d %s' % (n_rays, S, family), '')
    x = gc.inputs(1, n_rays, S, family, 1)
    _check(_run1(L, lib, x), gc.oracle(x, torch.float64), 'hn_gbuffer1 grid stride %d x %d %s' % (n_rays, S, family), '')


@pytest.mark.parametrize('S', gc.ARG_S)
def test_gbuffer_null_outputs(L, lib, S):
    """Each output alone NULL, and all but one: a NULL output is left untouched, the others are as before."""
    x2, x1 = gc.inputs(1, gc.ARG_RAYS, S, 'thin', 2), gc.inputs(1, gc.ARG_RAYS, S, 'thin', 1)
    r2, r1 = gc.oracle(x2, torch.float64), gc.oracle(x1, torch.float64)
    for k in KEYS:
        others = tuple(j for j in KEYS if j != k)
        _check(_run2(L, lib, x2, want=others), r2, 'hn_gbuffer2 S=%d %s NULL' % (S, k), '', want=others)
        _check(_run2(L, lib, x2, want=(k,)), r2, 'hn_gbuffer2 S=%d only %s' % (S, k), '', want=(k,))
        _check(_run1(L, lib, x1, want=others), r1, 'hn_gbuffer1 S=%d %s NULL' % (S, k), '', want=others)
        _check(_run1(L, lib, x1, want=(k,)), r1, 'hn_gbuffer1 S=%d only %s' % (S, k), '', want=(k,))
    _check(_run2(L, lib, x2, want=()), r2, 'hn_gbuffer2 S=%d no output' % S, '', want=())


def test_gbuffer2_misaligned_depths(L, lib):
    """S = 64 with depths that start 4 bytes into their allocation: the 16-byte loads of the row kernel are not used."""
    x = gc.inputs(1, 5, 64, 'surface', 2)
    buf = torch.zeros(5 * 64 + 4, device='cuda')
    z = buf[1:1 + 5 * 64].view(5, 64)
    z.copy_(x['z'])
    assert z.data_ptr() % 16 == 4
    _check(_run2(L, lib, x, z_dev=z), gc.oracle(x, torch.float64), 'hn_gbuffer2 S=64 misaligned z', '')


def test_gbuffer_golden(L, lib):
    """The reference's own get_alpha_sample_color outputs (tests/golden/make_golden_gbuffer.py) through the kernel."""
    g, x = gc.golden_inputs()
    o = _run2(L, lib, x)
    ref = {k: torch.from_numpy(np.stack([g[k + '_hand'], g[k + '_obj']], 1)) for k in KEYS}
    _check(o, ref, 'hn_gbuffer2 golden', '')


def test_gbuffer_refusals(L, lib):
    """S = 0 and a NULL input are HN_EINVAL with a message; no rays is a no-op that returns 0.  Nothing is launched: the outputs stay NaN."""
    x = gc.inputs(1, 5, 64, 'thin', 2)
    d = {k: _dev(x[k]) for k in ('sdf_h', 'grad_h', 'd_h', 'sdf_o', 'grad_o', 'd_o', 'z', 'Ro')}
    o, o1 = _outs(5, 2), _outs(5, 1)

    def call2(S=64, n_frames=1, P=5, **null):
        a = {k: (None if k in null else L.ptr(v)) for k, v in d.items()}
        return lib.hn_gbuffer2(a['sdf_h'], a['grad_h'], a['d_h'], x['inv_s_h'], a['sdf_o'], a['grad_o'], a['d_o'], x['inv_s_o'], a['z'], n_frames, P, S,
                               x['sample_dist'], a['Ro'], L.ptr(o['opacity'].t), L.ptr(o['depth'].t), L.ptr(o['normal'].t), L.stream_ptr())

    def call1(S=64, N=5, **null):
        a = {k: (None if k in null else L.ptr(v)) for k, v in d.items()}
        return lib.hn_gbuffer1(a['sdf_h'], a['grad_h'], a['d_h'], a['z'], N, S, x['sample_dist'], x['inv_s_h'], L.ptr(o1['opacity'].t),
                               L.ptr(o1['depth'].t), L.ptr(o1['normal'].t), L.stream_ptr())

    for call, word in ((lambda: call2(S=0), 'S = 0'), (lambda: call1(S=0), 'S = 0'), (lambda: call2(P=-1), '-1'), (lambda: call1(N=-1), '-1'),
                       (lambda: call2(grad_o=1), 'NULL'), (lambda: call2(z=1), 'NULL'), (lambda: call1(sdf_h=1), 'NULL'), (lambda: call1(d_h=1), 'NULL')):
        assert call() == -1
        assert word in lib.hn_last_error().decode(), lib.hn_last_error()
    assert call2(P=0) == 0 and call2(n_frames=0) == 0 and call1(N=0) == 0
    assert call2(P=0, sdf_h=1, z=1) == 0, 'no rays: the inputs are not looked at'
    torch.cuda.synchronize()
    for k in KEYS:
        o[k].untouched('a refused / empty call: ' + k)
        o1[k].untouched('a refused / empty call: ' + k)


# ---- through the renderers ------------------------------------------------------------------------------------------------------------
NEAR, FAR, N_SAMPLES, N_IMPORTANCE = 0.4, 1.5, 64, 64


def _scene(n_rays, seed):
    """n_rays rays through the synthetic hand (tests/golden/make_golden.py's hand_scene_rays) and an object pose next to its palm ->
    device tensors rays_o, rays_d [n,3], bt_inv [21,4,4], T_pose [21,3], Ro (the matrix render takes: p' = Ro (p - To)), To."""
    from honerf_amd import synth
    from oracle.render import rays_from_xy
    bt_inv, T_pose, joints = synth.synth_hand_pose(seed)
    rng = np.random.RandomState(seed + 100)
    cam = synth.front_camera(dist=0.0, focal=2.0)
    tgt = joints[rng.randint(0, 21, size=n_rays)] + 0.012 * rng.standard_normal((n_rays, 3))
    xy = np.stack([tgt[:, 0] / tgt[:, 2] * 2.0, tgt[:, 1] / tgt[:, 2] * 2.0], -1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    o, d = rays_from_xy(t(xy), t(cam['R'][0]), t(cam['T'][0]), t(cam['focal'][0]), t(cam['principal'][0]))
    R_obj, t_obj = synth.synth_obj_pose(seed + 3, center=tuple(joints[9] + np.array([0.03, 0.0, 0.02])))
    c = lambda a: (a if isinstance(a, torch.Tensor) else t(a)).float().cuda().contiguous()
    return c(o), c(d), c(bt_inv), c(T_pose), c(R_obj).T.contiguous(), c(t_obj), joints


def _single(kind):
    from honerf_amd.renderer import NeuSRenderer
    from helpers import product_modules
    m = product_modules()
    return NeuSRenderer(m['sdf_' + kind], m['var_' + kind], m['color_' + kind], kind, N_SAMPLES, N_IMPORTANCE, 0, 4, 1.0)


def _dual(batched=False):
    from honerf_amd.renderer import NeuSRenderer_fitting
    from honerf_amd.renderer_batch import NeuSRenderer_fitting as Batched
    from helpers import product_modules
    m = product_modules()
    cls = Batched if batched else NeuSRenderer_fitting
    return cls(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], N_SAMPLES, N_IMPORTANCE, 0, 4, 1.0)


def _close(got, ref, what):
    return assert_close(got.detach().cpu().reshape(ref.shape), ref, RT, what)


@pytest.mark.parametrize('kind', ['hand', 'obj'])
def test_render_buffers_single(kind):
    """NeuSRenderer.render_buffers on 37 rays: render's own outputs bit for bit, opacity = weight_sum, and the three buffers against the
    float64 restatement on the field's values at that render's depths."""
    from honerf_amd import lib as L_
    from honerf_amd.renderer import _points
    o, d, bt_inv, T_pose, Ro, To, _ = _scene(37, 13)
    ren = _single(kind)
    t_rand = torch.rand(37, 1, generator=torch.Generator().manual_seed(8)).cuda()
    args = (o, d, NEAR, FAR, bt_inv, T_pose, None, Ro, To, 0)
    with torch.no_grad():
        plain = ren.render(*args, t_rand=t_rand)
    out = ren.render_buffers(*args, t_rand=t_rand)
    assert set(out) == set(plain) | {'opacity', 'depth', 'normal'}
    for k in ('color_fine', 'weight_sum', 'weight_max', 'cdf_fine'):      # (gradient_error is a sum by atomics: its last bits vary from run to run)
        assert torch.equal(out[k], plain[k]), '%s render_buffers: %s differs from render' % (kind, k)
    assert out['opacity'].shape == (37, 1) and out['depth'].shape == (37, 1) and out['normal'].shape == (37, 3)
    _close(out['opacity'], plain['weight_sum'].cpu(), kind + ' render_buffers: opacity against weight_sum')
    z = ren.last_z_vals
    S = z.shape[1]
    assert S == N_SAMPLES + N_IMPORTANCE
    sample_dist = gc.f32_scalar((FAR - NEAR) / N_SAMPLES)
    ol, dl = ren.convert_obj_to_local(o, d, Ro, To) if kind == 'obj' else (o, d)
    pts, _ = _points(L_.load(), ol, dl, z, 1, sample_dist)
    with torch.no_grad():
        sdf, grad, _ = ren.field().evaluate(pts, dl, S, bt_inv.reshape(1, 21, 4, 4), T_pose.reshape(1, 21, 3)) if kind == 'hand' else \
            ren.field().evaluate(pts, dl, S)
    x = {'sdf': sdf.reshape(37, S).cpu(), 'grad': grad.reshape(37, S, 3).cpu(), 'd': dl.cpu(), 'z': z.cpu(), 'inv_s': gc.f32_scalar(ren.field().inv_s),
         'sample_dist': sample_dist, 'n_frames': 1, 'rays_per_frame': 37, 'S': S, 'fields': 1}
    ref = gc.oracle(x, torch.float64)
    if kind == 'obj':
        ref['normal'] = ref['normal'] @ Ro.cpu().double()
    for k in KEYS:
        _close(out[k], ref[k].reshape(out[k].shape), '%s render_buffers: %s' % (kind, k))
    assert float(out['opacity'].max()) > 0.05, 'the rays must see the field'
    with pytest.raises(ValueError, match='render'):
        ren.render_buffers(o, d.clone().requires_grad_(True), NEAR, FAR, bt_inv, T_pose, None, Ro, To, 0, t_rand=t_rand)


def _dual_reference(ren, out, d, Ro, F, P):
    """The float64 restatement on a two-field render's own per-sample outputs and depths -> the eight buffers, flat [N, ..]."""
    N = F * P
    z = ren.last_z_vals.reshape(N, -1)
    S = z.shape[1]
    hand, obj = ren.fields()
    _, d_o = ren.convert_obj_to_local(d, d, Ro, torch.zeros_like(Ro[..., 0]))
    x = {'sdf_h': out['sdf_hand'].reshape(N, S).cpu(), 'grad_h': out['gradient_hand'].reshape(N, S, 3).cpu(), 'sdf_o': out['sdf_obj'].reshape(N, S).cpu(),
         'grad_o': out['gradient_obj'].reshape(N, S, 3).cpu(), 'd_h': d.reshape(N, 3).cpu(), 'd_o': d_o.reshape(N, 3).cpu(), 'z': z.cpu(),
         'Ro': Ro.reshape(F, 3, 3).cpu(), 'inv_s_h': gc.f32_scalar(hand.inv_s), 'inv_s_o': gc.f32_scalar(obj.inv_s),
         'sample_dist': gc.f32_scalar((FAR - NEAR) / N_SAMPLES), 'n_frames': F, 'rays_per_frame': P, 'S': S, 'fields': 2}
    r = gc.oracle(x, torch.float64)
    return {'opacity_hand': r['opacity'][:, :1], 'opacity_obj': r['opacity'][:, 1:], 'depth_hand': r['depth'][:, :1], 'depth_obj': r['depth'][:, 1:],
            'depth': r['depth'].sum(1, keepdim=True), 'normal_hand': r['normal'][:, 0], 'normal_obj': r['normal'][:, 1], 'normal': r['normal'].sum(1)}


def _check_dual(tag, ren, args, t_rand, d, Ro, F, P, lead):
    with torch.no_grad():
        plain = ren.render(*args, t_rand=t_rand)
    out = ren.render_buffers(*args, t_rand=t_rand)
    ref = _dual_reference(ren, out, d, Ro, F, P)
    assert set(out) == set(plain) | set(ref)
    for k in ('color_fine', 'weight_sum', 'sdf_hand', 'sdf_obj', 'gradient_hand', 'gradient_obj'):      # (gradient_error_*: sums by atomics)
        assert torch.equal(out[k], plain[k]), '%s: %s differs from render' % (tag, k)
    for k, v in ref.items():
        assert tuple(out[k].shape) == lead + (v.shape[-1],), (k, out[k].shape)
        _close(out[k], v.reshape(out[k].shape), '%s: %s' % (tag, k))
    _close(out['opacity_hand'] + out['opacity_obj'], plain['weight_sum'].cpu(), tag + ': opacity_hand + opacity_obj against weight_sum')
    assert float(out['opacity_hand'].max()) > 0.05 and float(out['opacity_obj'].max()) > 0.05, 'the rays must see both fields'
    return out


def test_render_buffers_fitting():
    o, d, bt_inv, T_pose, Ro, To, _ = _scene(37, 13)
    ren = _dual()
    t_rand = torch.rand(37, 1, generator=torch.Generator().manual_seed(8)).cuda()
    _check_dual('fitting render_buffers', ren, (o, d, NEAR, FAR, bt_inv, T_pose, None, Ro, To), t_rand, d, Ro, 1, 37, (37,))
    with pytest.raises(ValueError, match='render'):
        ren.render_buffers(o, d, NEAR, FAR, bt_inv, T_pose, None, Ro.clone().requires_grad_(True), To, t_rand=t_rand)


def test_render_buffers_batched():
    """The frame-batched class, 2 frames x 5 rays, each frame with its own pose: [F, P, ..] buffers."""
    frames = [_scene(5, 30 + f) for f in range(2)]
    o, d, bt_inv, T_pose, Ro, To = (torch.stack([fr[i] for fr in frames]) for i in range(6))
    ren = _dual(batched=True)
    t_rand = torch.rand(2, 5, 1, generator=torch.Generator().manual_seed(9)).cuda()
    _check_dual('batched render_buffers', ren, (o, d, NEAR, FAR, bt_inv, T_pose, None, Ro, To), t_rand, d, Ro, 2, 5, (2, 5))
    with pytest.raises(ValueError, match='render'):
        ren.render_buffers(o.clone().requires_grad_(True), d, NEAR, FAR, bt_inv, T_pose, None, Ro, To, t_rand=t_rand)


def test_render_view_buffers():
    """Two ring cameras at 16 x 12: shapes and dtypes, render_views' colour bits, and the depth / normal / label rules restated in torch
    from render_buffers' floats of the same chunks.  Pixels whose opacity, or whose opacity_hand - opacity_obj, is within 1e-4 of a
    decision threshold are left out of the label and zero-mask comparisons: at most 5 % of them."""
    from honerf_amd import harness, synth
    _, _, bt_inv, T_pose, Ro_t, To, joints = _scene(1, 13)
    Ro = Ro_t.T.contiguous()            # (render_view_buffers takes the pose, as render_views does, and passes its transpose on)
    ren = _dual()
    H, W, V, step = 12, 16, 2, 80
    B = H * W
    cams = synth.ring_cameras(V, radius=0.6, target=tuple(float(c) for c in joints[9]), seed=3)
    t_rand = torch.rand(V, B, 1, generator=torch.Generator().manual_seed(5)).cuda()
    for thr in (0.5, 0.1):
        got = harness.render_view_buffers(ren, cams, H, W, NEAR, FAR, bt_inv, T_pose, Ro, To, batch_size=step, t_rand=t_rand, opacity_threshold=thr)
        assert set(got) == {'color', 'depth', 'normal', 'label'} and all(v.is_cuda for v in got.values())
        assert got['color'].dtype == torch.uint8 and tuple(got['color'].shape) == (V, H, W, 3)
        assert got['depth'].dtype == torch.float32 and tuple(got['depth'].shape) == (V, H, W)
        assert got['normal'].dtype == torch.uint8 and tuple(got['normal'].shape) == (V, H, W, 3)
        assert got['label'].dtype == torch.uint8 and tuple(got['label'].shape) == (V, H, W)
        assert torch.equal(got['color'], harness.render_views(ren, cams, H, W, NEAR, FAR, bt_inv, T_pose, Ro, To, batch_size=step, t_rand=t_rand))
        left_out = 0
        for v in range(V):
            ro, rd = harness.image_rays({k: np.asarray(a)[v:v + 1] for k, a in cams.items()}, H, W, torch.device('cuda'))
            chunks = [ren.render_buffers(ro[s:s + step], rd[s:s + step], NEAR, FAR, bt_inv, T_pose, None, Ro_t, To, t_rand=t_rand[v, s:s + step])
                      for s in range(0, B, step)]
            f = {k: torch.cat([c[k] for c in chunks]).double().cpu() for k in ('opacity_hand', 'opacity_obj', 'depth', 'normal')}
            oh, oo = f['opacity_hand'][:, 0], f['opacity_obj'][:, 0]
            op = oh + oo
            sure = ((op - thr).abs() > 1e-4) & ((oh - oo).abs() > 1e-4)
            left_out += int((~sure).sum())
            seen = op >= thr
            label = torch.where(seen, torch.where(oh >= oo, 1, 2), 0)
            assert torch.equal(got['label'][v].reshape(B).cpu().long()[sure], label[sure]), 'view %d: label' % v
            depth = torch.where(seen, f['depth'][:, 0] / op.clamp_min(1e-30), torch.zeros_like(op))
            g_depth = got['depth'][v].reshape(B).cpu().double()
            assert bool(((g_depth == 0) == ~seen)[sure].all()), 'view %d: where the depth is 0' % v
            bounded('render_view_buffers view %d threshold %g: depth' % (v, thr),
                    float((g_depth - depth)[sure].abs().max() / max(float(depth.max()), 1e-30)), RT)
            assert bool(((g_depth[seen & sure] > NEAR) & (g_depth[seen & sure] < FAR + (FAR - NEAR) / N_SAMPLES)).all())
            n = torch.nn.functional.normalize(f['normal'] @ torch.from_numpy(np.asarray(cams['R'])[v]).double(), dim=-1)
            level = (n * 0.5 + 0.5) * 255.0
            g_normal = got['normal'][v].reshape(B, 3).cpu().double()
            assert bool((g_normal[~seen & sure] == 0).all()), 'view %d: normal where nothing is seen' % v
            # truncation: a float64 level within 1e-3 of an integer may fall on either side in fp32
            diff = (g_normal - level.clamp(0, 255).floor())[seen & sure]
            near_int = ((level - level.round()).abs() < 1e-3)[seen & sure]
            assert bool(((diff == 0) | (near_int & (diff.abs() <= 1))).all()), 'view %d: normal levels' % v
        assert left_out <= 0.05 * V * B, '%d of %d pixels sit on a decision threshold' % (left_out, V * B)
        counts = [int((got['label'] == i).sum()) for i in range(3)]
        print('render_view_buffers threshold %g: %d background, %d hand, %d object pixels; %d left out' % (thr, *counts, left_out))
        if thr == 0.1:
            assert counts[1] > 0 and counts[0] > 0, counts
