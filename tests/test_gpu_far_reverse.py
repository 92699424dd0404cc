"""The all-far tile program's reverse sweep is a discarded pass ("The reverse sweep held").
Since the Jacobian pass of the all-far program multiplies zero fragments, nothing reads dz6 .. dz0: the program with the shared
epilogue and without table chunks now fetches two of the sweep's 56 chunks, runs the other 54 groups on one held k-step with the zero
fragment as B, runs none of the sweep's epilogues, and its forward layers keep neither a1 .. a7 nor the seed dz7 in the LDS image.
The sweep sits between lin8 and the Jacobian pass, so what it must leave behind is the weight stream's state (offset, buffer, the
chunk in flight): a wrong one shows in rgb at once, a forward epilogue that lost more than its store shows in sdf.  `hn_field_eval`
(sdf, gradient, rgb, feature rows) must return the SAME BITS as the general program (HONERF_FAR_TILES=0) and as the all-far program
that streams every chunk and keeps the real sweep (HONERF_FAR_STREAM=0), for both precisions; far points share one sdf and have a
gradient of exactly 0.  The method, the points, the weight sets and the helpers are those of tests/test_gpu_far_stream.py and
tests/test_gpu_far_hold.py: launches through the C ABI with a workspace filled with 0xFF bytes and into NaN-filled outputs."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_far_hold as fh
import test_gpu_far_stream as fs

pytestmark = pytest.mark.gpu

PRECISIONS = fs.PRECISIONS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fields = fh.fields   # one packed hand field per (weight set, precision), module-scoped: this module's own instance
check = fh.check     # the default against HONERF_FAR_TILES=0 and against HONERF_FAR_STREAM=0, far points' sdf and gradient


@pytest.mark.parametrize('weights', fh.WEIGHT_SETS, ids=lambda w: '%s%d' % (w[0], w[1]))
@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile(fields, monkeypatch, precision, weights):
    """128 far points: one tile through the held sweep on every weight set, those with weights near the top of the fp16 range and
    the one with spread pre-activations included."""
    pts, live = fs.build(torch.zeros(128, dtype=torch.bool), 510)
    check(fields(precision, *weights), pts, live, monkeypatch)


@pytest.mark.parametrize('live_pattern', [(False, False), (False, True)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_points(fields, monkeypatch, precision, live_pattern):
    """n = 2: two samples and 126 pad lanes, copies of the last one.  A live last sample sends the tile to the general program."""
    pts, live = fs.build(torch.tensor(live_pattern), 520)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """One tile of 100 points and 28 pad lanes with a far and with a live last sample."""
    live = torch.zeros(100, dtype=torch.bool)
    live[99] = last_live
    pts, live = fs.build(live, 530)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('pattern', ['far_far_far', 'far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_three_tiles_per_workgroup(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs).  The patterns hand the weight stream,
    the LDS image (whose slots a1 .. a7, HS_DZ7 and HS_DZ4 the all-far program no longer writes) and the parked registers between the
    all-far and the general program in both directions."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    f = fields(precision)
    ws = lambda n: f.lib.hn_field_workspace_bytes(f.handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r, kind in enumerate(pattern.split('_')):
        live[r * per_round:(r + 1) * per_round] = kind == 'live'
    pts, live = fs.build(live, 540)
    check(f, pts, live, monkeypatch)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_culled_launch(fields, monkeypatch, precision):
    """hn_field_set_culling on a mixed set -- an all-far tile, a tile with one live wave, a live tile, a padded far tail: a culled
    launch keeps the general program; its outputs equal the dense launch's in every mode."""
    live = torch.zeros(3 * 128 + 37, dtype=torch.bool)
    live[128 + 64:128 + 96] = True
    live[256:384] = True
    pts, live = fs.build(live, 550)
    field = fields(precision)
    field.set_culling(False)
    dense = check(field, pts, live, monkeypatch)
    field.set_culling(True)
    try:
        for mode in (fh.DEFAULT, fh.STREAM_OFF, fh.GENERAL):
            culled = fs.evaluate(field, pts, monkeypatch, mode)
            for name, a, b in zip(fs.NAMES, dense, culled):
                assert torch.equal(a, b), '%s: culled launch (mode %s) differs from the dense one' % (name, mode[0])
    finally:
        field.set_culling(False)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_live_first_render(monkeypatch, precision):
    """NeuSRenderer.render of 12 rays x 32 samples in live-first order at every size (HONERF_LIVE_FIRST=2): six rays pass joints of the
    hand at 5 mm, six miss it, so the ordered list ends in all-far tiles.  Every returned tensor but the scalar `gradient_error` (an
    atomic sum in arrival order) has the general program's bits, and those of HONERF_FAR_STREAM=0."""
    from honerf_amd.nets import SingleVarianceNetwork
    from honerf_amd.renderer import NeuSRenderer
    dev = torch.device('cuda')
    sdf, col = fh.make_nets('plain', 21)
    var = SingleVarianceNetwork(0.3).to(dev)
    ren = NeuSRenderer(sdf, var, col, 'hand', 32, 0, 0, 4, 1.0)
    ren.precision = precision
    miss = np.array([[0.5, 0.5, 0.9], [-0.5, 0.5, 0.9], [0.5, -0.5, 0.9], [-0.5, -0.5, 0.9], [0.6, 0.0, 0.9], [0.0, 0.6, 0.9]], dtype=np.float32)
    o, d = fs.rays_through(np.concatenate([fs.JOINTS[[0, 4, 8, 12, 16, 20]] + np.float32(0.005), miss]))
    t_rand = torch.rand(12, 1, generator=torch.Generator().manual_seed(2))
    monkeypatch.setenv('HONERF_LIVE_FIRST', '2')

    def render(mode):
        fs.set_mode(monkeypatch, mode)
        with torch.no_grad():
            out = ren.render(o.cuda(), d.cuda(), 0.4, 1.5, torch.from_numpy(fs.BT_INV).cuda(), torch.from_numpy(fs.T_POSE).cuda(), None, None, None, 0,
                             t_rand=t_rand.cuda())
        out = {k: v.clone() for k, v in out.items()}
        torch.cuda.synchronize()
        return out

    got = render(fh.DEFAULT)
    assert bool(torch.isfinite(got['color_fine']).all())
    for mode in (fh.GENERAL, fh.STREAM_OFF):
        ref = render(mode)
        assert ref.keys() == got.keys()
        for k in ref:
            if k == 'gradient_error':
                continue
            assert torch.equal(ref[k], got[k]), 'render: %s differs between the default and mode %s' % (k, mode[0])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_paced_mixed_launch(fields, monkeypatch, precision):
    """One launch of XCD_PACE_MIN_ROUNDS tiles per CU, from which size the kernel paces its workgroups per XCD (the threshold is read
    from the kernels' header).  A quarter of the rounds is live, and those rounds lie between far ones: in the order the points are
    given every workgroup changes program four times, and in live-first order a paced launch runs hundreds of all-far tiles in a row
    behind the live ones."""
    with open(os.path.join(ROOT, 'ho-nerf_amd', 'csrc', 'hn_mlp2.h')) as fh_:
        rounds = int(re.search(r'constexpr int XCD_PACE_MIN_ROUNDS = (\d+);', fh_.read()).group(1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    n_live = max(rounds // 4, 1)
    live_rounds = [1 + (rounds - 2) * i // n_live for i in range(n_live)]   # 8 rounds: rounds 1 and 4, far rounds on both sides
    assert len(set(live_rounds)) == n_live and 0 < min(live_rounds) and max(live_rounds) < rounds - 1
    live = torch.zeros(rounds * per_round, dtype=torch.bool)
    for r in live_rounds:
        live[r * per_round:(r + 1) * per_round] = True
    pts, live = fs.build(live, 560)
    check(fields(precision), pts, live, monkeypatch)
