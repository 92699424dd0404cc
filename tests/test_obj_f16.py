"""precision='f16' (HN_PREC_F16) for the OBJECT field: k_field2_obj_f16<0|1> run lin1, lin2, lin3, the hidden columns of lin4, lin5, lin6
and their W^T steps of the reverse sweep on one f16 MFMA per product; lin0, the skip columns over the encoded inputs, lin7, lin8, the
products in front of the encoding Jacobian and the colour network stay on the three-pass form, and so does everything that keeps a tape."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import product_modules, rel_err, bounded, record, cu, t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _obj_field(prec):
    from honerf_amd.nets import PackedField
    m = product_modules()
    return PackedField('obj', m['sdf_obj'], m['color_obj'], m['var_obj'], precision=prec)


def test_obj_f16_error_is_pinned(golden):
    """The object field's single-pass mode against the REFERENCE's fixtures, with the hand mode's bounds (test_gpu_parity.py::
    test_f16_throughput_mode_error_is_pinned): sdf 1e-3, gradient 2e-3, rgb 1e-3 on field_obj.npz; colour 2e-3, weight_sum / cdf /
    weight_max 1.5e-3 on the coarse-only render render_obj_32_0.npz (both arithmetics see the same depths).  sdf() and the sdf of a full
    evaluation are the same bits, and the errors sit more than 10x above the f16x3 kernels' -- on a build without k_field2_obj_f16 an
    object 'f16' field IS the f16x3 field and that assertion fails.
    Observed (MI355X): sdf 5.4e-4, gradient 4.1e-4, rgb 1.0e-4 (f16x3 on the same fixture: sdf 7.2e-7, gradient 7.6e-7); render (under
    no_grad, i.e. without a tape): colour 6.4e-4, weight_sum 6.3e-4, cdf 7.8e-4, weight_max 9.4e-4."""
    from honerf_amd.renderer import NeuSRenderer
    g = golden('field_obj')
    f, f3 = _obj_field('f16'), _obj_field('f16x3')
    pts, dirs = cu(g['pts']), cu(g['dirs'])
    sdf, grad, rgb = f.evaluate(pts, dirs, 1)
    e_sdf = bounded('obj f16 mode: sdf vs reference', rel_err(sdf.cpu().numpy().reshape(-1, 1), g['out'][:, :1]), 1e-3)
    e_grad = bounded('obj f16 mode: gradient vs reference', rel_err(grad.cpu().numpy(), g['grad']), 2e-3)
    bounded('obj f16 mode: rgb vs reference', rel_err(rgb.cpu().numpy(), g['rgb']), 1e-3)
    assert torch.equal(f.sdf(pts).reshape(-1), sdf.reshape(-1))                  # the sdf-only kernel takes the same passes
    s3, g3, _ = f3.evaluate(pts, dirs, 1)
    e3_sdf, e3_grad = rel_err(s3.cpu().numpy().reshape(-1, 1), g['out'][:, :1]), rel_err(g3.cpu().numpy(), g['grad'])
    record('obj f16x3 on the same fixture: sdf vs reference', e3_sdf, 1e-4)
    record('obj f16x3 on the same fixture: gradient vs reference', e3_grad, 1e-4)
    assert e_sdf > 10 * e3_sdf and e_grad > 10 * e3_grad, (e_sdf, e3_sdf, e_grad, e3_grad)   # it IS a different arithmetic
    gr = golden('render_obj_32_0')
    m = product_modules()
    ren = NeuSRenderer(m['sdf_obj'], m['var_obj'], m['color_obj'], 'obj', int(gr['n_samples']), 0, 0, 4, 1.0)
    ren.precision = 'f16'
    with torch.no_grad():        # (no tape: with grad mode on this renderer's render is differentiable in its parameters, i.e. f16x3)
        out = ren.render(cu(gr['rays_o']), cu(gr['rays_d']), float(gr['near']), float(gr['far']), None, None, None, gr.get('Ro'), gr.get('To'), 0,
                         t_rand=cu(gr['t_rand']))
    for k, bound in (('color_fine', 2e-3), ('weight_sum', 1.5e-3), ('cdf_fine', 1.5e-3), ('weight_max', 1.5e-3)):
        bounded('obj f16 mode: render_obj_32_0 %s vs reference' % k, rel_err(out[k].detach().cpu().numpy().reshape(gr[k].shape), gr[k]), bound)
    # the adjoint side of such a field is the fp32-equivalent one
    assert f.lib.hn_field_bwd_workspace_bytes(f.handle, 128) == f3.lib.hn_field_bwd_workspace_bytes(f3.handle, 128)


def _launch(f, pts, dirs, n, spr, full, out):
    """One launch over the first n points into sentinel-filled buffers of `out` (sdf [M], grad [M,3], rgb [M,3])."""
    from honerf_amd import lib as L
    lib = f.lib
    need = lib.hn_field_workspace_bytes(f.handle, n)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    if full:
        rc = lib.hn_field_eval(f.handle, L.ptr(pts), L.ptr(dirs), n, spr, None, None, 1, n, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), None,
                               L.ptr(ws), need, L.stream_ptr())
    else:
        rc = lib.hn_field_sdf(f.handle, L.ptr(pts), n, None, None, 1, n, L.ptr(out[0]), L.ptr(ws), need, L.stream_ptr())
    L.check(rc, 'hn_field_eval' if full else 'hn_field_sdf')
    torch.cuda.synchronize()


SENTINEL = -777.25


def _buffers(m):
    return [torch.full((m,), SENTINEL, device='cuda'), torch.full((m, 3), SENTINEL, device='cuda'), torch.full((m, 3), SENTINEL, device='cuda')]


def test_obj_f16_results_do_not_depend_on_grouping(golden):
    """A sample's result does not depend on its launch: n = 1 (one lane), 31 / 33 (a ragged 32-sample block), 128 / 133 (a ragged
    tile), 2 * 128 + 17 (more than one workgroup) against the same points inside one launch of 512, bit for bit, for the full evaluation
    and the sdf-only launch, with 1 and 7 samples per ray; nothing is written past n.  One launch long enough for the XCD-paced path
    (XCD_PACE_MIN_ROUNDS tiles per workgroup) against the same points in 8 chunks."""
    g = golden('field_obj')
    f = _obj_field('f16')
    lo, hi = g['pts'].min(0), g['pts'].max(0)
    gen = torch.Generator().manual_seed(16)
    M = 512
    pts = cu((t(lo) + (t(hi) - t(lo)) * torch.rand(M, 3, generator=gen)).float())
    dirs = cu(torch.nn.functional.normalize(torch.randn(M, 3, generator=gen), dim=-1))
    for spr in (1, 7):
        whole = {}
        for full in (True, False):
            whole[full] = _buffers(M)
            _launch(f, pts, dirs, M, spr, full, whole[full])
            assert all(bool(torch.isfinite(b).all()) and not bool((b == SENTINEL).any()) for b in whole[full][:3 if full else 1])
        assert torch.equal(whole[True][0], whole[False][0])
        for n in (1, 31, 33, 128, 133, 2 * 128 + 17):
            for full in (True, False):
                out = _buffers(M)
                _launch(f, pts, dirs, n, spr, full, out)
                for b, w in list(zip(out, whole[full]))[:3 if full else 1]:
                    assert torch.equal(b[:n], w[:n]), 'n = %d, spr = %d, full = %s' % (n, spr, full)
                for b in out:
                    assert bool((b[n:] == SENTINEL).all()), 'n = %d, spr = %d, full = %s: written past n' % (n, spr, full)
    # the XCD-paced path: at least XCD_PACE_MIN_ROUNDS tiles of 128 samples per workgroup, one workgroup per CU
    with open(os.path.join(ROOT, 'ho-nerf_amd', 'csrc', 'hn_mlp2.h')) as fh:
        rounds = int(re.search(r'constexpr int XCD_PACE_MIN_ROUNDS = (\d+);', fh.read()).group(1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = max(1 << 18, rounds * cus * 128)
    assert N % 8 == 0
    big = cu((t(lo) + (t(hi) - t(lo)) * torch.rand(N, 3, generator=gen)).float())
    bd = cu(torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1))
    one = _buffers(N)
    _launch(f, big, bd, N, 1, True, one)
    c = N // 8
    for i in range(8):
        part = _buffers(c)
        _launch(f, big[i * c:(i + 1) * c], bd[i * c:(i + 1) * c], c, 1, True, part)
        for b, w in zip(part, one):
            assert torch.equal(b, w[i * c:(i + 1) * c]), 'chunk %d of the paced launch' % i


def test_obj_f16_taped_render_is_the_f16x3_render(golden):
    """What keeps a tape is untouched: a two-field renderer at 'f16' called WITH autograd (render_dual.npz: 24 rays, 192 depths, four
    importance rounds) returns the 'f16x3' renderer's colour, sdf and gradients bit for bit, and the same gradients of Ro, To, bt_inv."""
    from honerf_amd.renderer import NeuSRenderer_fitting
    g = golden('render_dual')
    res = {}
    for prec in ('f16x3', 'f16'):
        m = product_modules()
        ren = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'],
                                   int(g['n_samples']), int(g['n_importance']), 0, 4, 1.0)
        ren.precision = prec
        leaves = {k: cu(g[k]).clone().requires_grad_(True) for k in ('rays_o', 'rays_d', 'bt_inv', 'Ro', 'To')}
        out = ren.render(leaves['rays_o'], leaves['rays_d'], float(g['near']), float(g['far']), leaves['bt_inv'], cu(g['T_pose']), None,
                         leaves['Ro'], leaves['To'], t_rand=cu(g['t_rand']))
        hand, obj = ren.fields()
        assert hand.precision == prec and obj.precision == prec
        loss = ((out['color_fine'] * cu(g['w_color'])).sum() + (out['weight_sum'] * cu(g['w_wsum'])).sum()
                + (out['sdf_hand'] * cu(g['w_sdf_hand'])).sum() + (out['sdf_obj'] * cu(g['w_sdf_obj'])).sum())
        loss.backward()
        res[prec] = ({k: out[k].detach().clone() for k in ('color_fine', 'sdf_hand', 'sdf_obj', 'gradient_hand', 'gradient_obj')},
                     {k: leaves[k].grad.detach().clone() for k in ('Ro', 'To', 'bt_inv')})
    for k, v in res['f16x3'][0].items():
        assert torch.isfinite(v).all() and torch.equal(res['f16'][0][k], v), k
    for k, v in res['f16x3'][1].items():
        assert torch.isfinite(v).all() and float(v.abs().max()) > 0 and torch.equal(res['f16'][1][k], v), 'g_' + k


# observed on an MI355X: worst grey-level difference and PSNR of the all-'f16' views against the 'f16x3' views (the parent's behaviour)
VIEWS_WORST_LEVELS = 2
VIEWS_PSNR_DB = 60.85        # (per view 60.85 / 62.08 dB; ssim 0.99990 / 0.99993)


def test_obj_f16_view_render():
    """harness.render_views of the 24 x 20, 2-view synthetic two-field scene of test_image_metrics.py with the renderer at 'f16' (both
    fields single-pass under torch.no_grad(): the untaped path) and at 'f16x3': uint8 [2, 24, 20, 3], bit-reproducible, chunk-consistent
    within one grey level, different from the f16x3 views -- and still different with only the OBJECT field single-pass, which a build
    without k_field2_obj_f16 cannot give.  The f16 views pass four importance rounds on single-pass sdf values; no reference bounds that,
    so the distance to the f16x3 views is the MEASURED one with the margin for +-1-level quantisation flips: worst grey-level difference
    <= 2x the observed 2 levels, PSNR >= the observed 60.85 dB (lower view; the other 62.08 dB, ssim 0.99990 / 0.99993) - 3 dB."""
    import bench
    from honerf_amd import harness, synth
    from honerf_amd.image_metrics import image_metrics
    from honerf_amd.nets import PackedField
    dev = torch.device('cuda')
    ren, nets, _, _, _ = bench.build_fit(dev, 40, 1, bench.FIT_RAYS, 'f16x3', halo=True)
    chain, j, _ = bench.build_fit_data(dev, 40, 1, halo=True)
    with torch.no_grad():
        pose = chain()
    bt_inv, T21 = pose['bt_inv'][0].detach().contiguous(), pose['T_pose_21'][0].detach().contiguous()
    Ro, To = pose['obj_r'][0].detach().contiguous(), pose['obj_t'][0].detach().contiguous()
    H, W, V = 24, 20, 2
    B = H * W
    cams = synth.ring_cameras(V, radius=1.0, target=tuple(float(c) for c in j[9]), seed=3)
    t_rand = torch.rand(V, B, 1, generator=torch.Generator().manual_seed(5)).to(dev)
    views = lambda n: harness.render_views(ren, cams, H, W, bench.NEAR, bench.FAR, bt_inv, T21, Ro, To, batch_size=n, t_rand=t_rand)
    assert (ren.precision or 'f16x3') == 'f16x3'
    ref = views(96)
    ren.precision = 'f16'
    got = views(96)
    hand, obj = ren.fields()
    assert hand.precision == 'f16' and obj.precision == 'f16'
    for x in (ref, got):
        assert x.is_cuda and x.dtype == torch.uint8 and tuple(x.shape) == (V, H, W, 3)
    assert int(got.max()) > 32, 'the synthetic views must show the scene'
    assert torch.equal(views(96), got)                                            # bit-reproducible
    d100 = (views(100).int() - got.int()).abs()
    record('f16 views: pixels that differ between 96-ray and 100-ray chunks', int((d100.amax(dim=3) > 0).sum()), V * B, kind='count')
    bounded('f16 views: grey levels between 96-ray and 100-ray chunks', int(d100.max()), 1, kind='abs')
    assert not torch.equal(got, ref), "the 'f16' views are the 'f16x3' views: no field is single-pass"
    # attribution: only the object field single-pass (the renderer's cached pair replaced; its version key stays valid)
    ren.precision = 'f16x3'
    hand3, _ = ren.fields()
    mods = (ren.sdf_network_obj, ren.color_network_obj, ren.deviation_network_obj)
    ren._fields = (hand3, PackedField('obj', mods[0], mods[1], mods[2], precision='f16'))
    mixed = views(96)
    ren._fields = None
    assert not torch.equal(mixed, ref), 'an object field at f16 renders the f16x3 views: it has no single-pass kernels'
    worst = int((got.int() - ref.int()).abs().max())
    met = image_metrics(got, ref)
    psnr = float(np.min(met['psnr']))
    record('f16 views vs f16x3 views: pixels that differ', int(((got.int() - ref.int()).abs().amax(dim=3) > 0).sum()), V * B, kind='count')
    record('f16 views vs f16x3 views: ssim (lower view)', float(np.min(met['ssim'])), 1.0, kind='value')
    print('obj_f16 view render: worst grey-level difference %d, psnr per view %s, ssim per view %s' % (worst, met['psnr'], met['ssim']))
    bounded('f16 views vs f16x3 views: worst grey-level difference', worst, 2 * VIEWS_WORST_LEVELS, kind='abs')
    record('f16 views vs f16x3 views: psnr [dB] (lower view), bound is a floor', psnr, VIEWS_PSNR_DB - 3.0, kind='value')
    assert psnr >= VIEWS_PSNR_DB - 3.0, 'psnr %.2f dB < %.2f dB' % (psnr, VIEWS_PSNR_DB - 3.0)
