"""The packed stash image of the hand evaluation kernel's uniform waves (HONERF_UNIFORM_STASH).
A wave whose 32 samples are all far keeps one column of everything it parks in its stash.  HONERF_UNIFORM_STASH=2 leaves that column
where lanes 0 and 32 always stored it (16 useful bytes per 1 KiB block); unset or 1 packs it into whole 128-byte lines of the wave's
free slot: 32 bytes per block, a different address for every store and load of such a wave.  0 moves every wave at full width.  The
three forms park and read back the same numbers, so `hn_field_eval` (sdf, gradient, rgb, feature rows) must return the SAME BITS in
all three, for both precisions.
The launches go through the C ABI with a workspace of this file's own, filled with 0xFF bytes before every launch: whatever a launch
has not written is NaN (as fp32 and as f16), so a load from an address that the address map never stored to cannot pass by luck --
and neither can a packed image read back after a normal-layout tile, or the other way round, on the same workgroup.
"Far" points lie a metre from every joint (all 21 bone masks exactly 0), "live" points 5 mm from joint 9.  Each case first checks that
premise on the full-width outputs: every far point returns one and the same sdf and a gradient of exactly 0, live points do not.
What equal bits cannot show is that a launch with the switch unset or 1 really takes the packed addresses: a library that ignored the
difference between 1 and 2 would pass.  That the packed map is what the kernel is built with, and that it is injective and stays in the
wave's free slot, is the static_assert on USTASH_SITES in hn_field2_hand.hip; these cases show that the map, as built, returns every
value it parks."""
import pytest
import torch

from honerf_amd import synth

pytestmark = pytest.mark.gpu

BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)
MODES = ('0', '1', '2')
PRECISIONS = ['f16x3', 'f16']


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


def evaluate(field, pts, monkeypatch, mode):
    """hn_field_eval over `pts` with HONERF_UNIFORM_STASH=mode, on a workspace of 0xFF bytes and into NaN-filled outputs."""
    from honerf_amd import lib as L
    monkeypatch.setenv('HONERF_UNIFORM_STASH', mode)
    lib = field.lib
    p = pts.cuda().contiguous()
    dirs = torch.nn.functional.normalize(p, dim=-1).contiguous()
    bt, tp = torch.from_numpy(BT_INV).cuda().contiguous(), torch.from_numpy(T_POSE).cuda().contiguous()
    n = p.shape[0]
    out = [torch.full(s, float('nan'), device='cuda') for s in ((n,), (n, 3), (n, 3), (n, 256))]
    need = lib.hn_field_workspace_bytes(field.handle, n)
    ws = torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device='cuda')
    rc = lib.hn_field_eval(field.handle, L.ptr(p), L.ptr(dirs), n, 1, L.ptr(bt), L.ptr(tp), 1, n, L.ptr(out[0]), L.ptr(out[1]),
                           L.ptr(out[2]), L.ptr(out[3]), L.ptr(ws), need, L.stream_ptr())
    L.check(rc, 'hn_field_eval')
    torch.cuda.synchronize()
    return out


def check(field, pts, is_live, monkeypatch):
    full, packed, in_place = (evaluate(field, pts, monkeypatch, m) for m in MODES)
    # the premise, on the full-width path's outputs
    sdf, grad = full[0].cpu(), full[1].cpu()
    far = ~is_live
    for o in full:
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
    for name, a, b, c in zip(('sdf', 'grad', 'rgb', 'feat'), full, packed, in_place):
        assert torch.equal(a, b), '%s: the packed form (1) differs from full width (0)' % name
        assert torch.equal(a, c), '%s: the in-place one-column form (2) differs from full width (0)' % name
        assert torch.equal(b, c), '%s: the packed form (1) differs from the in-place form (2)' % name


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile(fields, monkeypatch, precision):
    """128 far points: one tile, four uniform waves."""
    pts, live = build(torch.zeros(128, dtype=torch.bool), 110)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_three_uniform_waves_and_a_live_one(fields, monkeypatch, precision):
    """One tile: waves 0, 1 and 3 far, wave 2 all live."""
    live = torch.zeros(128, dtype=torch.bool)
    live[64:96] = True
    pts, live = build(live, 120)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('lane', [0, 31])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_live_sample_takes_the_full_layout(fields, monkeypatch, precision, lane):
    """One tile of far points except one live sample in wave 1, in its lane 0 (the lane whose column a uniform wave keeps) or in its lane
    31: that wave is not uniform and every lane must get its own column back."""
    live = torch.zeros(128, dtype=torch.bool)
    live[32 + lane] = True
    pts, live = build(live, 130 + lane)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """229 points: the last wave holds 5 samples and 27 pad lanes, copies of the last one.  A far last sample leaves that wave uniform;
    a live one (with far samples in front of it) makes it non-uniform through the copies.  Wave 0 is live in both."""
    live = torch.zeros(229, dtype=torch.bool)
    live[:32] = True
    live[228] = last_live
    pts, live = build(live, 140)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('pattern', ['far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_layouts_alternate_on_one_workgroup(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs) on one stash, whose waves alternate
    between the packed image and the normal layout from tile to tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    # one workgroup per CU at the most, each with its own stash: the stash workspace stops growing at `cus` tiles.  Checked here so
    # that a change of the launch grid does not silently end the coverage of "three tiles per workgroup".
    ws = lambda n: fields('f16x3').lib.hn_field_workspace_bytes(fields('f16x3').handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r in range(3):
        live[r * per_round:(r + 1) * per_round] = (r % 2 == 1) == (pattern == 'far_live_far')
    pts, live = build(live, 150)
    check(fields(precision), pts, live, monkeypatch)
