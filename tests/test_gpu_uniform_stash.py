"""One stash column for the waves of the hand evaluation kernel whose 32 samples are all far (HONERF_UNIFORM_STASH).
Such a wave holds the same numbers in every sample column of everything it parks in its stash, so it stores the column of its lanes
j == 0 and every lane reads that one back.  Nothing else changes, so `hn_field_eval` (sdf, gradient, rgb, feature rows) must return
the SAME BITS with the switch off, with it on, and for a third arrangement of the same points in which no wave is uniform: there every
wave of 32 holds 31 points of the case and one live point of its own, and per-sample results do not depend on the lane, wave or tile
a sample sits in (tests/test_gpu_live_first_order.py).  "Far" points lie a metre from every joint (all 21 bone masks exactly 0),
"live" points 5 mm from joint 9 (a point ON a joint is NaN, as in the reference).  Each case first checks that premise on the
kernel's own outputs: every far point returns one and the same sdf and a gradient of exactly 0, live points do not."""
import numpy as np
import pytest
import torch

from honerf_amd import synth

pytestmark = pytest.mark.gpu

BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)


@pytest.fixture(scope='module')
def fields():
    """One packed hand field per precision, made on first use and shared by the cases."""
    from honerf_amd.nets import SDFNetwork, RenderingNetwork, PackedField
    made = {}

    def get(precision):
        if precision not in made:
            dev = torch.device('cuda')
            sdf, col = SDFNetwork().to(dev), RenderingNetwork(use_gradients=True).to(dev)
            sdf.reset_parameters(21)
            col.reset_parameters(22)
            made[precision] = PackedField('hand', sdf, col, 0.3, precision=precision)
        return made[precision]
    return get


def far_points(n, seed):
    """n distinct points a metre (and up to 5 cm more) from the hand: no bone of the hand is longer than 0.25 m."""
    g = torch.Generator().manual_seed(seed)
    c = torch.from_numpy(JOINTS.mean(0)) + torch.tensor([0.0, 0.0, 1.25])
    return (c + 0.05 * torch.rand(n, 3, generator=g)).float()


def live_points(n, seed):
    """n distinct points 5 mm from joint 9 (its cutoff is 3 cm)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return (torch.from_numpy(JOINTS[9]) + 0.005 * d).float()


def build(is_live, seed):
    """The case's points from its far / live pattern (bool [n])."""
    is_live = torch.as_tensor(is_live, dtype=torch.bool)
    pts = far_points(len(is_live), seed)
    pts[is_live] = live_points(int(is_live.sum()), seed + 1)
    return pts, is_live


def evaluate(field, pts, monkeypatch, switch):
    monkeypatch.setenv('HONERF_UNIFORM_STASH', switch)
    p = pts.cuda().contiguous()
    dirs = torch.nn.functional.normalize(p, dim=-1).contiguous()
    out = field.evaluate(p, dirs, 1, torch.from_numpy(BT_INV).cuda(), torch.from_numpy(T_POSE).cuda(), want_feat=True)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def with_a_live_point_per_wave(pts, seed):
    """31 points of the case + one live point per wave of 32 (the wave's last lane; the list's last wave is filled up with live
    points, so that clamped pad lanes are live too).  Returns the new list and where point i of the case went."""
    n = len(pts)
    n_waves = (n + 30) // 31
    out = live_points(32 * n_waves, seed)
    pos = torch.arange(n)
    pos = pos + pos // 31          # wave w holds the case's points 31 w .. 31 w + 30 in its lanes 0 .. 30
    out[pos] = pts
    return out, pos


def check(field, pts, is_live, monkeypatch, seed):
    off = evaluate(field, pts, monkeypatch, '0')
    on = evaluate(field, pts, monkeypatch, '1')
    pts3, pos = with_a_live_point_per_wave(pts, seed)
    third = [o[pos.cuda()] for o in evaluate(field, pts3, monkeypatch, '1')]
    # the premise, on the full-width path's outputs
    sdf, grad = off[0].reshape(-1).cpu(), off[1].cpu()
    far = ~is_live
    for o in off:
        assert bool(torch.isfinite(o).all())
    if bool(far.any()):
        assert bool((sdf[far] == sdf[far][0]).all()), 'far points do not share one sdf value'
        assert bool((grad[far] == 0.0).all()), 'far points have a non-zero gradient'
    if bool(is_live.any()):
        assert bool((grad[is_live] != 0.0).any(dim=-1).all()), 'a live point has a gradient of exactly 0'
        assert int(is_live.sum()) == 1 or len(torch.unique(sdf[is_live])) > 1, 'live points share one sdf value'
        if bool(far.any()):
            assert bool((sdf[is_live] != sdf[far][0]).all())
    # the same bits, sample by sample
    for name, a, b, c in zip(('sdf', 'grad', 'rgb', 'feat'), off, on, third):
        assert torch.equal(a, b), '%s: switch on differs from switch off' % name
        assert torch.equal(a, c), '%s: the arrangement without uniform waves differs' % name


PRECISIONS = ['f16x3', 'f16']


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_uniform_tile(fields, monkeypatch, precision):
    """128 far points: one tile, four uniform waves."""
    pts, live = build(torch.zeros(128, dtype=torch.bool), 10)
    check(fields(precision), pts, live, monkeypatch, 11)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_mixed_waves(fields, monkeypatch, precision):
    """256 points: wave 0 far, wave 1 far except its lane j = 0, wave 2 far except j = 31, wave 3 all live, waves 4 - 7 far."""
    live = torch.zeros(256, dtype=torch.bool)
    live[32] = True
    live[64 + 31] = True
    live[96:128] = True
    pts, live = build(live, 20)
    check(fields(precision), pts, live, monkeypatch, 21)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """229 points: the last wave holds 5 samples and 27 pad lanes, copies of the last one.  A far last sample leaves that wave uniform;
    a live one (with far samples in front of it) makes it non-uniform through the copies.  Wave 0 is live in both."""
    live = torch.zeros(229, dtype=torch.bool)
    live[:32] = True
    live[228] = last_live
    pts, live = build(live, 30)
    check(fields(precision), pts, live, monkeypatch, 31)


@pytest.mark.parametrize('pattern', ['far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_slot_reuse_across_tiles(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs) and its waves reuse their stash slots:
    compact stores followed by full-width loads of the same slots, and the other way round, never meet stale columns."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    # one workgroup per CU at the most, each with its own stash: the stash workspace stops growing at `cus` tiles.  Checked here so
    # that a change of the launch grid does not silently end the coverage of "three tiles per workgroup".
    ws = lambda n: fields('f16x3').lib.hn_field_workspace_bytes(fields('f16x3').handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r in range(3):
        live[r * per_round:(r + 1) * per_round] = (r % 2 == 1) == (pattern == 'far_live_far')
    pts, live = build(live, 40)
    check(fields(precision), pts, live, monkeypatch, 41)
