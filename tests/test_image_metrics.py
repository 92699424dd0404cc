"""The device image metrics (hn_imgmetric.hip through honerf_amd.image_metrics) against the float64 restatement of
tests/test_image_metrics_cpu.py: the squared error to the integer, PSNR to 1e-12 relative, SSIM to 1e-9 absolute (both sides hold
exact integer window sums, only the fp64 rounding of S and of the mean differs), the S map to 1e-6 per pixel (fp32 storage), no
pixel left out; every input form and a repeated call to the bit; refusals; and producer to consumer: harness.render_views of the
two-field renderer, the files harness.write_image leaves in the reference's tree, and tools/image_eval.py on them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import bounded, record
from test_image_metrics_cpu import SIZES, image_pairs, np_psnr, np_sse, np_ssim, np_ssim_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


_REF = {}


def reference(H, W):
    """The scene and the restatement's values of it, computed once per size."""
    if (H, W) not in _REF:
        a, b = image_pairs(H, W)
        _REF[(H, W)] = dict(a=a, b=b, sse=np.array([np_sse(x, y) for x, y in zip(a, b)], dtype=np.int64),
                            psnr=np.array([np_psnr(x, y) for x, y in zip(a, b)]), ssim=np.array([np_ssim(x, y) for x, y in zip(a, b)]),
                            map=np.stack([np_ssim_map(x, y) for x, y in zip(a, b)]))
    return _REF[(H, W)]


@pytest.mark.parametrize('H,W', SIZES)
def test_matches_the_restatement(H, W):
    from honerf_amd import image_metrics as im
    ref = reference(H, W)
    a, b = ref['a'], ref['b']
    what = '%d x %d' % (H, W)
    s = im.sse(a, b)
    assert s.is_cuda and s.dtype == torch.int64 and tuple(s.shape) == (3,)
    assert np.array_equal(_np(s), ref['sse']), (what, _np(s), ref['sse'])
    p = im.psnr(a, b)
    assert p.is_cuda and p.dtype == torch.float64 and tuple(p.shape) == (3,)
    bounded(what + ' psnr (relative)', float(np.abs(_np(p) / ref['psnr'] - 1.0).max()), 1e-12)
    q = im.ssim(a, b)
    assert q.is_cuda and q.dtype == torch.float64 and tuple(q.shape) == (3,)
    bounded(what + ' ssim', float(np.abs(_np(q) - ref['ssim']).max()), 1e-9, kind='abs')
    m = im.ssim_map(a, b)
    assert m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (3, H - 6, W - 6, 3)
    bounded(what + ' ssim_map, every pixel', float(np.abs(_np(m).astype(np.float64) - ref['map']).max()), 1e-6, kind='abs')
    both = im.image_metrics(a, b)
    assert both['psnr'].dtype == np.float64 and both['psnr'].tobytes() == _np(p).tobytes() and both['ssim'].tobytes() == _np(q).tobytes()
    assert both['psnr_mean'] == float(_np(p).mean()) and both['ssim_mean'] == float(_np(q).mean())
    # identical images: exactly 1 and +inf
    assert _np(im.ssim(a, a)).tolist() == [1.0] * 3 and _np(im.psnr(b, b)).tolist() == [np.inf] * 3 and _np(im.sse(a, a)).tolist() == [0] * 3
    assert float(_np(im.ssim_map(b, b)).min()) == 1.0 == float(_np(im.ssim_map(b, b)).max())


def test_the_cases_span_low_and_high_ssim():
    vals = np.concatenate([reference(H, W)['ssim'] for H, W in SIZES])
    assert vals.min() < 0.5 and vals.max() > 0.8, (vals.min(), vals.max())


@pytest.mark.parametrize('H,W', [(37, 41), (8, 130)])
def test_input_forms_and_repeated_calls_give_the_same_bits(H, W):
    from honerf_amd import image_metrics as im
    ref = reference(H, W)
    a, b = ref['a'], ref['b']
    run = lambda x, y: tuple(_np(f(x, y)).tobytes() for f in (im.sse, im.psnr, im.ssim, im.ssim_map))
    first = run(a, b)
    assert run(a, b) == first                                                   # a repeated call
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert run(ta, tb) == first and run(ta.cuda(), tb.cuda()) == first and run(a, tb.cuda()) == first
    # image 1 of the batch alone: a device view that starts H W 3 bytes into the allocation (an odd address at 37 x 41), and [H, W, 3]
    alone = run(ta.cuda()[1:2], tb.cuda()[1:2])
    flat = run(a[1], b[1])
    for k, (x, y, z) in enumerate(zip(first, alone, flat)):
        per = len(x) // 3
        assert y == x[per:2 * per] and z == y, k
    assert im.sse(a[1], b[1]).dim() == 0 and im.psnr(a[1], b[1]).dim() == 0 and im.ssim(a[1], b[1]).dim() == 0
    assert tuple(im.ssim_map(a[1], b[1]).shape) == (H - 6, W - 6, 3)
    one = im.image_metrics(a[1], b[1])
    assert np.ndim(one['psnr']) == 0 and np.ndim(one['ssim']) == 0 and one['ssim_mean'] == float(one['ssim'])
    # non-contiguous input (a channel flip, as a BGR reader would hand over) is the image it shows
    assert _np(im.sse(a[..., ::-1], b[..., ::-1])).tolist() == ref['sse'].tolist()
    bounded('%d x %d channel-flipped ssim' % (H, W), float(np.abs(_np(im.ssim(a[..., ::-1], b[..., ::-1])) - ref['ssim']).max()), 1e-9, kind='abs')


def test_refusals_raise_and_never_fault():
    from honerf_amd import image_metrics as im, lib
    a, b = reference(37, 41)['a'], reference(37, 41)['b']
    for fn in (im.sse, im.psnr, im.ssim, im.ssim_map, im.image_metrics):
        first = '^pred:' if fn is im.image_metrics else '^a:'
        second = '^gt:' if fn is im.image_metrics else '^b:'
        with pytest.raises(ValueError, match=first):
            fn(a.astype(np.float32), b)                                         # float images
        with pytest.raises(ValueError, match=second):
            fn(a, torch.from_numpy(b).double())
        with pytest.raises(ValueError, match=first):
            fn(a[..., :2], b[..., :2])                                          # another channel count
        with pytest.raises(ValueError, match=first):
            fn(np.concatenate([a, a[..., :1]], -1), b)
        with pytest.raises(ValueError, match=first):
            fn(a[:0], b[:0])                                                    # empty
        with pytest.raises(ValueError, match=second):
            fn(a, b[:, :, :0])
        with pytest.raises(ValueError):
            fn(a, b[:2])                                                        # mismatched shapes
        with pytest.raises(ValueError):
            fn(a, b[:, :, :40])
        with pytest.raises(ValueError):
            fn(a[0], b)                                                         # [H, W, 3] against [F, H, W, 3]
        with pytest.raises(ValueError, match=first):
            fn(a[:, :6], b[:, :6])                                              # a side under 7
        with pytest.raises(ValueError, match=first):
            fn(a[:, :, :6], b[:, :, :6])
        with pytest.raises(ValueError, match=first):
            fn(a[0, 0], b[0, 0])                                                # 2-D
        with pytest.raises(ValueError, match=first):
            fn(a.tolist(), b)
    # the library itself: status codes with a message, before anything is launched
    L = lib.load()
    wsb = L.hn_im_workspace_bytes
    assert wsb(0, 37, 41) == 0 and wsb(3, 6, 41) == 0 and wsb(3, 37, 6) == 0 and wsb(-1, 37, 41) == 0
    assert wsb(1 << 12, 1 << 10, 1 << 10) == 0 and wsb(1, 1 << 16, 1 << 16) == 0         # 3 x 2^32 and 3 x 2^32 values
    assert wsb(3, 37, 41) >= 8 * 3 * 3 and wsb(64, 512, 334) >= 8 * 3 * 64 * 6 * 16
    x = torch.zeros(2, 8, 9, 3, dtype=torch.uint8, device='cuda')
    sse = torch.zeros(2, dtype=torch.int64, device='cuda')
    ch = torch.zeros(2, 3, dtype=torch.float64, device='cuda')
    sm = torch.zeros(2, 2, 3, 3, dtype=torch.float32, device='cuda')
    ws = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    P, S = lib.ptr, lib.stream_ptr()
    calls = [L.hn_im_sse(None, P(x), 2, 8, 9, P(sse), P(ws), 4096, S), L.hn_im_sse(P(x), None, 2, 8, 9, P(sse), P(ws), 4096, S),
             L.hn_im_sse(P(x), P(x), 2, 8, 9, None, P(ws), 4096, S), L.hn_im_sse(P(x), P(x), 2, 8, 9, P(sse), None, 4096, S),
             L.hn_im_sse(P(x), P(x), 2, 8, 9, P(sse), P(ws), 8, S),                     # a workspace that is too small
             L.hn_im_sse(P(x), P(x), 0, 8, 9, P(sse), P(ws), 4096, S), L.hn_im_sse(P(x), P(x), 2, 6, 9, P(sse), P(ws), 4096, S),
             L.hn_im_sse(P(x), P(x), 2, 8, 6, P(sse), P(ws), 4096, S), L.hn_im_sse(P(x), P(x), 1 << 12, 1 << 10, 1 << 10, P(sse), P(ws), 4096, S),
             L.hn_im_ssim(None, P(x), 2, 8, 9, P(ch), P(sm), P(ws), 4096, S), L.hn_im_ssim(P(x), None, 2, 8, 9, P(ch), P(sm), P(ws), 4096, S),
             L.hn_im_ssim(P(x), P(x), 2, 8, 9, None, P(sm), P(ws), 4096, S), L.hn_im_ssim(P(x), P(x), 2, 8, 9, P(ch), P(sm), None, 4096, S),
             L.hn_im_ssim(P(x), P(x), 2, 8, 9, P(ch), P(sm), P(ws), 8, S), L.hn_im_ssim(P(x), P(x), -2, 8, 9, P(ch), P(sm), P(ws), 4096, S),
             L.hn_im_ssim(P(x), P(x), 2, 8, 5, P(ch), P(sm), P(ws), 4096, S), L.hn_im_ssim(P(x), P(x), 2, 1 << 20, 1 << 20, P(ch), P(sm), P(ws), 4096, S)]
    assert calls == [-1] * len(calls), calls
    assert L.hn_last_error()
    torch.cuda.synchronize()
    assert int(sse.abs().sum()) == 0 and float(ch.abs().sum()) == 0.0 and float(sm.abs().sum()) == 0.0 and int(ws.sum()) == 0   # nothing written


def test_render_views_to_files_to_image_eval(tmp_path):
    """Producer to consumer: two held-out views of the synthetic two-field scene of tests/test_whole_step.py through
    harness.render_views, against direct renderer.render calls; the "ground truth" is the same render with the object moved by
    5 mm; both trees written as .ppm in the reference's layout with one training-view file that must be skipped; tools/image_eval.py
    on them against the restatement's means of the files."""
    import bench
    from honerf_amd import harness, synth
    dev = torch.device('cuda')
    ren, nets, _, _, _ = bench.build_fit(dev, 40, 1, bench.FIT_RAYS, 'f16x3', halo=True)
    chain, j, _ = bench.build_fit_data(dev, 40, 1, halo=True)
    with torch.no_grad():
        pose = chain()
    bt_inv, T21 = pose['bt_inv'][0].detach().contiguous(), pose['T_pose_21'][0].detach().contiguous()
    Ro, To = pose['obj_r'][0].detach().contiguous(), pose['obj_t'][0].detach().contiguous()
    H, W, V, step = 24, 20, 2, 96
    B = H * W
    # two chunk sizes: 96, five full chunks of the 480 rays, and 100, whose last chunk is a short one of 80
    assert B % step == 0 and B % 100 == 80
    cams = synth.ring_cameras(V, radius=1.0, target=tuple(float(c) for c in j[9]), seed=3)
    t_rand = torch.rand(V, B, 1, generator=torch.Generator().manual_seed(5)).to(dev)
    Ro_t = Ro.T.contiguous()
    rays = [harness.image_rays({k: a[v:v + 1] for k, a in cams.items()}, H, W, dev) for v in range(V)]
    with torch.no_grad():
        whole = [harness.to_image(ren.render(ro, rd, bench.NEAR, bench.FAR, bt_inv, T21, None, Ro_t, To, t_rand=t_rand[v])['color_fine'], H, W)
                 for v, (ro, rd) in enumerate(rays)]
    rendered = {}
    for n in (step, 100):
        got = harness.render_views(ren, cams, H, W, bench.NEAR, bench.FAR, bt_inv, T21, Ro, To, batch_size=n, t_rand=t_rand)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (V, H, W, 3)
        n_diff, worst = 0, 0
        for v, (ro, rd) in enumerate(rays):
            with torch.no_grad():
                chunks = [ren.render(ro[s:s + n], rd[s:s + n], bench.NEAR, bench.FAR, bt_inv, T21, None, Ro_t, To, t_rand=t_rand[v, s:s + n])
                          ['color_fine'] for s in range(0, B, n)]
            direct = np.concatenate([harness.to_image(c, 1, c.shape[0]).reshape(-1, 3) for c in chunks]).reshape(H, W, 3)
            assert _np(got[v]).tobytes() == direct.tobytes(), 'view %d, chunks of %d: render_views against to_image of the same chunks' % (v, n)
            d = np.abs(whole[v].astype(int) - direct.astype(int))
            n_diff += int((d.max(axis=2) > 0).sum())
            worst = max(worst, int(d.max()))
        record('pixels of %d that differ between %d-ray chunks and one %d-ray call' % (V * B, n, B), n_diff, V * B, kind='count')
        bounded('grey levels between %d-ray chunks and whole-image renders' % n, worst, 1, kind='abs')
        rendered[n] = got
    ours = rendered[step]
    again = harness.render_views(ren, cams, H, W, bench.NEAR, bench.FAR, bt_inv, T21, Ro, To, batch_size=step, t_rand=t_rand)
    assert torch.equal(again, ours)
    assert int(ours.max()) > 32, 'the synthetic views must show the scene'
    gt = harness.render_views(ren, cams, H, W, bench.NEAR, bench.FAR, bt_inv, T21, Ro, To + 0.005, batch_size=step, t_rand=t_rand)
    ours_h, gt_h = _np(ours), _np(gt)
    # the reference's tree: gt_path/<obj>/<frame>/MASK/<file>, ours_path/<fit>/<obj>/<frame>/render_<fit>/<file>
    gt_dir = tmp_path / 'final_render_img' / 'p1_box' / '000010' / 'MASK'
    our_dir = tmp_path / 'analys_res' / '12' / 'p1_box' / '000010' / 'render_12'
    gt_dir.mkdir(parents=True)
    our_dir.mkdir(parents=True)
    names = ['image_2132004%d.ppm' % v for v in range(V)]
    for v, name in enumerate(names):
        harness.write_image(str(gt_dir / name), gt_h[v])
        harness.write_image(str(our_dir / name), ours_h[v])
    harness.write_image(str(gt_dir / 'image_21320027.ppm'), gt_h[0])          # a training view: skipped, and it has no render
    files_o = [harness.read_image(str(our_dir / n)) for n in names]
    files_g = [harness.read_image(str(gt_dir / n)) for n in names]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(files_o, ours_h)) and all(x.tobytes() == y.tobytes() for x, y in zip(files_g, gt_h))
    psnr_mean = float(np.mean([np_psnr(o, g) for o, g in zip(files_o, files_g)]))
    ssim_mean = float(np.mean([np_ssim(o, g) for o, g in zip(files_o, files_g)]))
    record('producer to consumer: psnr_mean', psnr_mean, 60.0, kind='value')
    record('producer to consumer: ssim_mean', ssim_mean, 1.0, kind='value')
    assert np.isfinite(psnr_mean) and np.isfinite(ssim_mean) and psnr_mean < 60 and ssim_mean < 1, (psnr_mean, ssim_mean)
    torch.cuda.synchronize()
    out_json = tmp_path / 'per_file.json'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'image_eval.py'), str(tmp_path / 'final_render_img'), str(tmp_path / 'analys_res'),
                          '--fit-type', '12', '--json', str(out_json)], capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines == [str(V), '     psnr,     ssim', 'ours:  %.4f %.6f' % (psnr_mean, ssim_mean)], (run.stdout, psnr_mean, ssim_mean)
    import json
    with open(str(out_json)) as f:
        per_file = json.load(f)
    assert sorted(per_file) == ['p1_box+000010+' + n for n in names]
    for n, o, g in zip(names, files_o, files_g):
        assert abs(per_file['p1_box+000010+' + n]['ssim'] - np_ssim(o, g)) < 1e-9
    # a render that is missing for a held-out ground-truth file is an error naming the file
    os.remove(str(our_dir / names[1]))
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'image_eval.py'), str(tmp_path / 'final_render_img'), str(tmp_path / 'analys_res')],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode != 0 and names[1] in run.stderr, (run.returncode, run.stderr[-500:])
