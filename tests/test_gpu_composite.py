"""GPU tests of the alpha, compositing and sample-point kernels (ho-nerf_amd/csrc/hn_composite.hip and the sample-point part of
hn_sampling.hip), one entry point at a time through the C ABI, against the oracle's statements run in float64 on the same fp32
inputs (tests/composite_cases.py: the inputs, the references and the shape tables; tests/test_composite_cases_cpu.py: the fp32
oracle is within 5e-6 of float64 on every one of these inputs).

Which case launches which kernel (host dispatchers composite1 / composite2 / composite1_bwd / composite2_bwd / alpha / alpha_bwd /
sample_points / sample_points_bwd):
  k_composite1_rows<4,8>        test_composite1[S=32], grid stride 65545 x 32
  k_composite1_rows<4,16>       test_composite1[S=64], grid stride 32773 x 64, test_composite1_optional_arguments[64]
  k_composite1_rows<8,16>       test_composite1[S=128]
  k_composite1_rows<12,16>      test_composite1[S=192]
  k_composite1                  test_composite1[every other S], grid stride 8197 x 33, test_composite1_optional_arguments[65]
  k_composite2_rows<4,16>       test_composite2[S=64], grid stride 32773 x 64, test_composite2_optional_arguments[64]
  k_composite2_rows<8,16>       test_composite2[S=128]
  k_composite2_rows<12,16>      test_composite2[S=192]
  k_composite2                  test_composite2[every other S], grid stride 8197 x 33, test_composite2_optional_arguments[65]
  k_composite{1,2}_bwd_wave<1>  test_composite{1,2}_bwd[S=1, 2, 63, 64]
  k_composite{1,2}_bwd_wave<2>  test_composite{1,2}_bwd[S=65, 100, 128]
  k_composite{1,2}_bwd_wave<3>  test_composite{1,2}_bwd[S=129, 191, 192]
  k_composite{1,2}_bwd_wave<4>  test_composite{1,2}_bwd[S=193, 255, 256]
  k_composite{1,2}_bwd          test_composite{1,2}_bwd[S=257 (1, 5, 37 and 65 rays), 320]
  k_alpha, k_alpha_bwd          test_alpha_and_adjoint (wave-reduced g_rays_d: 7 x 64, 3 x 192, the whole waves of 23 x 100; one
                                atomic per lane: spr 1, 37, the straddling waves of 23 x 100, every last, partial wave)
  k_sample_points_t             test_sample_points[n=4, 40, 64, 132]
  k_sample_points               test_sample_points[n=1, 5, 41, 130], test_sample_points_misaligned
  k_sample_points_bwd           test_sample_points_adjoint_sizes

Every output is a view into a NaN-filled flat tensor with GUARD NaN floats in front of it and behind it: after the launch the
guards are still NaN (nothing was written outside) and the output holds no NaN (everything inside was written)."""
import numpy as np
import pytest
import torch

import composite_cases as cc
from helpers import assert_close, bounded

pytestmark = pytest.mark.gpu

# Values and gradients against float64: the bound the project holds these stages to (test_alpha_and_composite*), four times the 5e-6
# the fp32 oracle itself is held to on the same inputs.  Observed on MI355X (worst over all cases of an entry point;
# profiles/composite/parity_report.json has every row):
#   hn_alpha 1.1e-6 (alpha, 23 x 37 at inv_s = 300)        hn_alpha_bwd 4.1e-6 (g_sdf, 23 x 1 at inv_s = 14.9, g_c NULL)
#   hn_composite1 2.8e-6 (weight_sum, S = 320 thin)          hn_composite1_bwd 5.6e-6 (g_c, S = 128 thin, g_weight_sum NULL)
#   hn_composite2 3.3e-6 (weight_sum, S = 320 thin)          hn_composite2_bwd 3.9e-6 (g_alpha_o, S = 257 thin)
#   eik_sum 1.2e-6 (65545 x 32)
# The thin family at the largest S leads everywhere: fp32's 1 - a + 1e-7 is +1.9e-8 off per factor (composite_cases.alphas).
RT = 2e-5
RT_PTS = 1e-6              # sample points (test_coarse_z_and_points); dists are bit-exact.  Observed: 2.0e-7; misaligned vs aligned launch: 0
RT_PTS_BWD = 1e-5          # hn_sample_points_bwd (test_sample_points_adjoint).  Observed: 1.3e-7
GUARD = 64                 # floats; a multiple of 4, so that a guarded view is 16-byte aligned as a tensor of its own would be
EIK0 = 0.125               # what eik_sum holds before a launch: the kernels add to it


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
    """An output buffer of `shape` inside a NaN-filled flat tensor, GUARD (+ `shift`) NaN floats in front and GUARD behind."""

    def __init__(self, *shape, fill=float('nan'), shift=0):
        self.n = int(np.prod(shape))
        self.lo = GUARD + shift
        self.flat = torch.full((self.lo + self.n + GUARD,), float('nan'), device='cuda')
        self.t = self.flat[self.lo:self.lo + self.n].view(*shape)
        if fill == fill:
            self.t.fill_(fill)

    def check(self, what):
        assert bool(torch.isnan(self.flat[:self.lo]).all()) and bool(torch.isnan(self.flat[self.lo + self.n:]).all()), what + ': wrote outside its buffer'
        assert not bool(torch.isnan(self.t).any()), what + ': left part of its output unwritten (or wrote NaN)'
        return self.t.cpu()

    def untouched(self, what):
        assert bool(torch.isnan(self.flat).all()), what + ': wrote a buffer it must leave alone'


def _close(got, ref, bound, what, ctx):
    """assert_close with the case (`ctx`: what the report's row leaves out, so that it keeps one row per path) in the message."""
    try:
        return assert_close(got.reshape(ref.shape), ref, bound, what)
    except AssertionError as e:
        raise AssertionError('%s [%s]' % (e, ctx)) from None


def _eik(got, ref, what, ctx):
    """eik_sum held EIK0 before the launch: it holds EIK0 + the sum now."""
    try:
        return bounded(what, abs(float(got) - (EIK0 + float(ref))) / (EIK0 + float(ref)), RT)
    except AssertionError as e:
        raise AssertionError('%s [%s]' % (e, ctx)) from None


# ---- hn_composite1 ----------------------------------------------------------------------------------------------------------
def _run_composite1(L, lib, x, weights=True, weight_max=True, grad=True, eik=True):
    n_rays, S = x['alpha'].shape
    d = {k: _dev(x[k]) for k in ('alpha', 'c', 'rgb', 'grad')}
    o = {'color': Out(n_rays, 3), 'weights': Out(n_rays, S), 'weight_sum': Out(n_rays), 'weight_max': Out(n_rays), 'eik_sum': Out(1, fill=EIK0)}
    L.check(lib.hn_composite1(L.ptr(d['alpha']), L.ptr(d['c']), L.ptr(d['rgb']), L.ptr(d['grad']) if grad else None, n_rays, S, L.ptr(o['color'].t),
                              L.ptr(o['weights'].t) if weights else None, L.ptr(o['weight_sum'].t), L.ptr(o['weight_max'].t) if weight_max else None,
                              L.ptr(o['eik_sum'].t) if eik else None, L.stream_ptr()), 'hn_composite1')
    torch.cuda.synchronize()
    return o


def _check_composite1(o, ref, tag, ctx, skip=()):
    for k in ('color', 'weights', 'weight_sum', 'weight_max'):
        if k in skip:
            o[k].untouched('%s %s (NULL)' % (tag, k))
        else:
            _close(o[k].check(tag + ' ' + k), ref[k], RT, '%s: %s' % (tag, k), ctx)


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('S', cc.FWD_S)
def test_composite1(L, lib, S, family):
    for n_rays in cc.RAYS:
        x = cc.composite1_inputs(n_rays, S, family)
        ref = cc.composite1_oracle(x, torch.float64)
        tag, ctx = 'hn_composite1 S=%d %s' % (S, family), '%d rays' % n_rays
        o = _run_composite1(L, lib, x)
        _check_composite1(o, ref, tag, ctx)
        _eik(o['eik_sum'].check(tag + ' eik_sum')[0], ref['eik_sum'], tag + ': eik_sum', ctx)


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('n_rays,S', cc.GRID1)
def test_composite1_grid_stride(L, lib, n_rays, S, family):
    """More rays than 2048 blocks take in one pass: every block loops, the last pass is partial."""
    x = cc.composite1_inputs(n_rays, S, family)
    ref = cc.composite1_oracle(x, torch.float64)
    tag = 'hn_composite1 grid stride %d x %d %s' % (n_rays, S, family)
    o = _run_composite1(L, lib, x)
    _check_composite1(o, ref, tag, '')
    _eik(o['eik_sum'].check(tag + ' eik_sum')[0], ref['eik_sum'], tag + ': eik_sum', '')


@pytest.mark.parametrize('S', cc.ARG_S)
def test_composite1_optional_arguments(L, lib, S):
    x = cc.composite1_inputs(cc.ARG_RAYS, S, 'thin')
    ref = cc.composite1_oracle(x, torch.float64)
    tag = 'hn_composite1 S=%d' % S
    o = _run_composite1(L, lib, x, weights=False)
    _check_composite1(o, ref, tag + ' weights NULL', '', skip=('weights',))
    _eik(o['eik_sum'].check(tag)[0], ref['eik_sum'], tag + ' weights NULL: eik_sum', '')
    o = _run_composite1(L, lib, x, weight_max=False)
    _check_composite1(o, ref, tag + ' weight_max NULL', '', skip=('weight_max',))
    _eik(o['eik_sum'].check(tag)[0], ref['eik_sum'], tag + ' weight_max NULL: eik_sum', '')
    o = _run_composite1(L, lib, x, grad=False)
    _check_composite1(o, ref, tag + ' grad NULL', '')
    assert float(o['eik_sum'].check(tag)[0]) == EIK0, tag + ' grad NULL: eik_sum was touched'
    o = _run_composite1(L, lib, x, eik=False)
    _check_composite1(o, ref, tag + ' eik_sum NULL', '')
    assert float(o['eik_sum'].check(tag)[0]) == EIK0


# ---- hn_composite2 ----------------------------------------------------------------------------------------------------------
def _run_composite2(L, lib, x, w_hand=True, w_obj=True, grad_h=True, grad_o=True):
    n_rays, S = x['alpha_h'].shape
    d = {k: _dev(x[k]) for k in ('alpha_h', 'rgb_h', 'grad_h', 'alpha_o', 'rgb_o', 'grad_o')}
    o = {'color': Out(n_rays, 3), 'weight_sum': Out(n_rays), 'w_hand': Out(n_rays, S), 'w_obj': Out(n_rays, S), 'eik_sum': Out(2, fill=EIK0)}
    L.check(lib.hn_composite2(L.ptr(d['alpha_h']), L.ptr(d['rgb_h']), L.ptr(d['grad_h']) if grad_h else None, L.ptr(d['alpha_o']), L.ptr(d['rgb_o']),
                              L.ptr(d['grad_o']) if grad_o else None, n_rays, S, L.ptr(o['color'].t), L.ptr(o['weight_sum'].t),
                              L.ptr(o['w_hand'].t) if w_hand else None, L.ptr(o['w_obj'].t) if w_obj else None, L.ptr(o['eik_sum'].t), L.stream_ptr()),
            'hn_composite2')
    torch.cuda.synchronize()
    return o


def _check_composite2(o, ref, tag, ctx, skip=(), grad_h=True, grad_o=True):
    for k in ('color', 'weight_sum', 'w_hand', 'w_obj'):
        if k in skip:
            o[k].untouched('%s %s (NULL)' % (tag, k))
        else:
            _close(o[k].check(tag + ' ' + k), ref[k], RT, '%s: %s' % (tag, k), ctx)
    eik = o['eik_sum'].check(tag + ' eik_sum')
    for slot, (given, k) in enumerate(((grad_h, 'eik_h'), (grad_o, 'eik_o'))):
        if given:
            _eik(eik[slot], ref[k], '%s: eik_sum[%d]' % (tag, slot), ctx)
        else:
            assert float(eik[slot]) == EIK0, '%s: eik_sum[%d] was touched without its gradient' % (tag, slot)


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('S', cc.FWD_S)
def test_composite2(L, lib, S, family):
    for n_rays in cc.RAYS:
        x = cc.composite2_inputs(n_rays, S, family)
        _check_composite2(_run_composite2(L, lib, x), cc.composite2_oracle(x, torch.float64), 'hn_composite2 S=%d %s' % (S, family), '%d rays' % n_rays)


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('n_rays,S', cc.GRID2)
def test_composite2_grid_stride(L, lib, n_rays, S, family):
    x = cc.composite2_inputs(n_rays, S, family)
    _check_composite2(_run_composite2(L, lib, x), cc.composite2_oracle(x, torch.float64), 'hn_composite2 grid stride %d x %d %s' % (n_rays, S, family), '')


@pytest.mark.parametrize('S', cc.ARG_S)
def test_composite2_optional_arguments(L, lib, S):
    x = cc.composite2_inputs(cc.ARG_RAYS, S, 'thin')
    ref = cc.composite2_oracle(x, torch.float64)
    tag = 'hn_composite2 S=%d' % S
    _check_composite2(_run_composite2(L, lib, x, w_hand=False), ref, tag + ' w_hand NULL', '', skip=('w_hand',))
    _check_composite2(_run_composite2(L, lib, x, w_obj=False), ref, tag + ' w_obj NULL', '', skip=('w_obj',))
    _check_composite2(_run_composite2(L, lib, x, grad_o=False), ref, tag + ' grad_h only', '', grad_o=False)
    _check_composite2(_run_composite2(L, lib, x, grad_h=False), ref, tag + ' grad_o only', '', grad_h=False)
    _check_composite2(_run_composite2(L, lib, x, grad_h=False, grad_o=False), ref, tag + ' no gradients', '', grad_h=False, grad_o=False)


# ---- hn_composite1_bwd / hn_composite2_bwd ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('S', cc.BWD_S)
def test_composite1_bwd(L, lib, S, family):
    for n_rays in [n for n, s in cc.BWD_SHAPES if s == S]:
        x = cc.composite1_inputs(n_rays, S, family)
        d = {k: _dev(x[k]) for k in ('alpha', 'c', 'rgb', 'g_color', 'g_wsum')}
        for with_wsum in (True, False):
            ref = cc.composite1_oracle(x, torch.float64, adjoint=True, with_wsum=with_wsum)
            tag = 'hn_composite1_bwd S=%d %s%s' % (S, family, '' if with_wsum else ' g_weight_sum NULL')
            ctx = '%d rays' % n_rays
            o = {'g_alpha': Out(n_rays, S), 'g_c': Out(n_rays, S), 'g_rgb': Out(n_rays, S, 3)}
            L.check(lib.hn_composite1_bwd(L.ptr(d['alpha']), L.ptr(d['c']), L.ptr(d['rgb']), L.ptr(d['g_color']), L.ptr(d['g_wsum']) if with_wsum else None,
                                          n_rays, S, L.ptr(o['g_alpha'].t), L.ptr(o['g_c'].t), L.ptr(o['g_rgb'].t), L.stream_ptr()), 'hn_composite1_bwd')
            torch.cuda.synchronize()
            got = {k: v.check('%s %s' % (tag, k)) for k, v in o.items()}
            for k in ('g_alpha', 'g_c', 'g_rgb'):
                _close(got[k], ref[k], RT, '%s: %s' % (tag, k), ctx)
            assert int(torch.count_nonzero(got['g_c'][:, 1:])) == 0, '%s: g_c behind sample 0 is not exactly 0 [%s]' % (tag, ctx)


@pytest.mark.parametrize('family', cc.FAMILIES)
@pytest.mark.parametrize('S', cc.BWD_S)
def test_composite2_bwd(L, lib, S, family):
    for n_rays in [n for n, s in cc.BWD_SHAPES if s == S]:
        x = cc.composite2_inputs(n_rays, S, family)
        d = {k: _dev(x[k]) for k in ('alpha_h', 'rgb_h', 'alpha_o', 'rgb_o', 'g_color', 'g_wsum')}
        for with_wsum in (True, False):
            ref = cc.composite2_oracle(x, torch.float64, adjoint=True, with_wsum=with_wsum)
            tag = 'hn_composite2_bwd S=%d %s%s' % (S, family, '' if with_wsum else ' g_weight_sum NULL')
            o = {'g_alpha_h': Out(n_rays, S), 'g_rgb_h': Out(n_rays, S, 3), 'g_alpha_o': Out(n_rays, S), 'g_rgb_o': Out(n_rays, S, 3)}
            L.check(lib.hn_composite2_bwd(L.ptr(d['alpha_h']), L.ptr(d['rgb_h']), L.ptr(d['alpha_o']), L.ptr(d['rgb_o']), L.ptr(d['g_color']),
                                          L.ptr(d['g_wsum']) if with_wsum else None, n_rays, S, L.ptr(o['g_alpha_h'].t), L.ptr(o['g_rgb_h'].t),
                                          L.ptr(o['g_alpha_o'].t), L.ptr(o['g_rgb_o'].t), L.stream_ptr()), 'hn_composite2_bwd')
            torch.cuda.synchronize()
            for k, v in o.items():
                _close(v.check('%s %s' % (tag, k)), ref[k], RT, '%s: %s' % (tag, k), '%d rays' % n_rays)


# ---- hn_alpha / hn_alpha_bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inv_s', cc.INV_S)
@pytest.mark.parametrize('n_rays,spr', cc.ALPHA_SHAPES)
def test_alpha_and_adjoint(L, lib, n_rays, spr, inv_s):
    x = cc.alpha_inputs(n_rays, spr, inv_s)
    n = n_rays * spr
    d = {k: _dev(x[k]) for k in ('sdf', 'grad', 'rays_d', 'dists', 'g_alpha', 'g_c')}
    tag = 'hn_alpha %d x %d inv_s=%g' % (n_rays, spr, inv_s)
    ref = cc.alpha_oracle(x, torch.float64)
    for with_c in (True, False):
        o = {'alpha': Out(n), 'c': Out(n)}
        L.check(lib.hn_alpha(L.ptr(d['sdf']), L.ptr(d['grad']), L.ptr(d['rays_d']), L.ptr(d['dists']), n, spr, inv_s, L.ptr(o['alpha'].t),
                             L.ptr(o['c'].t) if with_c else None, L.stream_ptr()), 'hn_alpha')
        torch.cuda.synchronize()
        t = tag + ('' if with_c else ' c NULL')
        _close(o['alpha'].check(t + ' alpha'), ref['alpha'], RT, t + ': alpha', '')
        if with_c:
            _close(o['c'].check(t + ' c'), ref['c'], RT, t + ': c', '')
        else:
            o['c'].untouched(t + ' c (NULL)')
    tag = 'hn_alpha_bwd %d x %d inv_s=%g' % (n_rays, spr, inv_s)
    for with_gc, with_gd in ((True, True), (False, True), (True, False)):
        ref = cc.alpha_oracle(x, torch.float64, adjoint=True, with_gc=with_gc)
        o = {'g_sdf': Out(n), 'g_grad': Out(n, 3), 'g_rays_d': Out(n_rays, 3)}      # g_rays_d NaN as well: the entry point zeroes it
        L.check(lib.hn_alpha_bwd(L.ptr(d['sdf']), L.ptr(d['grad']), L.ptr(d['rays_d']), L.ptr(d['dists']), L.ptr(d['g_alpha']),
                                 L.ptr(d['g_c']) if with_gc else None, n, spr, inv_s, L.ptr(o['g_sdf'].t), L.ptr(o['g_grad'].t),
                                 L.ptr(o['g_rays_d'].t) if with_gd else None, L.stream_ptr()), 'hn_alpha_bwd')
        torch.cuda.synchronize()
        t = tag + ('' if with_gc else ' g_c NULL') + ('' if with_gd else ' g_rays_d NULL')
        for k in ('g_sdf', 'g_grad'):
            _close(o[k].check('%s %s' % (t, k)), ref[k], RT, '%s: %s' % (t, k), '')
        if with_gd:
            _close(o['g_rays_d'].check(t + ' g_rays_d'), ref['g_rays_d'], RT, t + ': g_rays_d', '')
        else:
            o['g_rays_d'].untouched(t + ' g_rays_d (NULL)')


# ---- hn_sample_points / _bwd ---------------------------------------------------------------------------------------------------
def _run_points(L, lib, x, mid, shift=0):
    """`shift`: z, pts and dists start that many floats into their (16-byte aligned) buffers."""
    B, n = x['z'].shape
    zbuf = torch.zeros(B * n + shift, device='cuda')
    zbuf[shift:] = _dev(x['z']).reshape(-1)
    o, d = _dev(x['rays_o']), _dev(x['rays_d'])
    out = {'pts': Out(B * n, 3, shift=shift), 'dists': Out(B, n, shift=shift)}
    for buf in (zbuf[shift:], out['pts'].t, out['dists'].t):
        assert buf.data_ptr() % 16 == 4 * (shift % 4), 'test buffers: not at the alignment the case is about'
    L.check(lib.hn_sample_points(L.ptr(o), L.ptr(d), L.ptr(zbuf[shift:]), B, n, mid, x['sample_dist'], L.ptr(out['pts'].t),
                                 L.ptr(out['dists'].t) if mid else None, L.stream_ptr()), 'hn_sample_points')
    torch.cuda.synchronize()
    return out


def _check_points(out, x, mid, tag):
    ref = cc.points_oracle(x, mid, torch.float64)
    pts = out['pts'].check(tag + ' pts')
    assert_close(pts, ref['pts'], RT_PTS, tag + ': pts')
    if mid:
        assert np.array_equal(out['dists'].check(tag + ' dists').numpy(), cc.points_oracle(x, 1, torch.float32)['dists'].numpy()), tag + ': dists not bit-exact'
    else:
        out['dists'].untouched(tag + ' dists (NULL)')
    return pts


@pytest.mark.parametrize('mid', [0, 1])
@pytest.mark.parametrize('B', cc.PTS_B)
@pytest.mark.parametrize('n', cc.PTS_N)
def test_sample_points(L, lib, n, B, mid):
    x = cc.points_inputs(B, n)
    _check_points(_run_points(L, lib, x, mid), x, mid, 'hn_sample_points %d x %d mid=%d' % (B, n, mid))


@pytest.mark.parametrize('mid', [0, 1])
def test_sample_points_misaligned(L, lib, mid):
    """n % 4 == 0 but z, pts and dists one float past a 16-byte boundary: the dispatcher must take the scalar kernel (the vector
    one would fault or write elsewhere), and the result is the aligned launch's."""
    x = cc.points_inputs(77, 40)
    tag = 'hn_sample_points 77 x 40 mid=%d' % mid
    a_out = _run_points(L, lib, x, mid)
    m_out = _run_points(L, lib, x, mid, shift=1)
    aligned = _check_points(a_out, x, mid, tag)
    shifted = _check_points(m_out, x, mid, tag + ' misaligned')
    bounded(tag + ': misaligned vs aligned launch', cc.rel_err(shifted.numpy(), aligned.numpy()), 2.0 ** -23)
    if mid:
        assert torch.equal(a_out['dists'].t, m_out['dists'].t)


@pytest.mark.parametrize('mid', [0, 1])
@pytest.mark.parametrize('n', cc.PTS_BWD_N)
def test_sample_points_adjoint_sizes(L, lib, n, mid):
    """What test_sample_points_adjoint (n = 192) leaves out: one sample, a wave one short of full, a wave and one sample."""
    B = 23
    x = cc.points_inputs(B, n)
    ref = cc.points_oracle(x, mid, torch.float64, adjoint=True)
    z, gp = _dev(x['z']), _dev(x['g_pts'])
    o = {'g_rays_o': Out(B, 3), 'g_rays_d': Out(B, 3)}
    L.check(lib.hn_sample_points_bwd(L.ptr(z), L.ptr(gp), B, n, mid, x['sample_dist'], L.ptr(o['g_rays_o'].t), L.ptr(o['g_rays_d'].t), L.stream_ptr()),
            'hn_sample_points_bwd')
    torch.cuda.synchronize()
    tag = 'hn_sample_points_bwd %d x %d mid=%d' % (B, n, mid)
    for k, v in o.items():
        assert_close(v.check('%s %s' % (tag, k)), ref[k], RT_PTS_BWD, '%s: %s' % (tag, k))
