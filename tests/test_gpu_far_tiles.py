"""The all-far tile program of the hand evaluation kernels (HONERF_FAR_TILES).
A sample tile whose four waves have no live bone is run by a second instance of the tile program, chosen per tile by the workgroup from
the kernel's own bone masks: no feature fragments, no leftover block, no Jacobian contraction, and the stash of such a tile in LDS
instead of the packed global image.  HONERF_FAR_TILES=0 sends every tile through the general program.  Both programs compute the same
numbers, so `hn_field_eval` (sdf, gradient, rgb, feature rows) must return the SAME BITS with the switch off and on, for both
precisions (both evaluation kernels carry the program).
The launches go through the C ABI with a workspace of this file's own, filled with 0xFF bytes, and into NaN-filled outputs: a value
that a launch never wrote, or read from a stash address that its program never stored to, cannot pass by luck.
"Far" points lie a metre from every joint (all 21 bone masks exactly 0), "live" points 5 mm from joint 9.  Each case first checks that
premise on the outputs of the general program: every far point returns one and the same sdf and a gradient of exactly 0, live points do
not.  Equal bits cannot show that a launch with the switch on really takes the all-far program for an all-far tile; that it does is
read from the profile (profiles/r08: the kernel's stash traffic)."""
import numpy as np
import pytest
import torch

from honerf_amd import synth

pytestmark = pytest.mark.gpu

BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)
PRECISIONS = ['f16x3', 'f16']
NAMES = ('sdf', 'grad', 'rgb', 'feat')


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
    yield get
    for f in made.values():
        f.set_culling(False)


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
    if bool(is_live.any()):
        pts[is_live] = live_points(int(is_live.sum()), seed + 1)
    return pts, is_live


def evaluate(field, pts, monkeypatch, switch):
    """hn_field_eval over `pts` with HONERF_FAR_TILES=switch (None: unset), on a workspace of 0xFF bytes and into NaN-filled outputs."""
    from honerf_amd import lib as L
    if switch is None:
        monkeypatch.delenv('HONERF_FAR_TILES', raising=False)
    else:
        monkeypatch.setenv('HONERF_FAR_TILES', switch)
    monkeypatch.delenv('HONERF_UNIFORM_STASH', raising=False)
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


def check_premise(general, is_live):
    sdf, grad = general[0].cpu(), general[1].cpu()
    far = ~is_live
    for o in general:
        assert bool(torch.isfinite(o).all())
    if bool(far.any()):
        assert bool((sdf[far] == sdf[far][0]).all()), 'far points do not share one sdf value'
        assert bool((grad[far] == 0.0).all()), 'far points have a non-zero gradient'
    if bool(is_live.any()):
        assert bool((grad[is_live] != 0.0).any(dim=-1).all()), 'a live point has a gradient of exactly 0'
        if bool(far.any()):
            assert bool((sdf[is_live] != sdf[far][0]).all())


def check(field, pts, is_live, monkeypatch):
    general = evaluate(field, pts, monkeypatch, '0')
    check_premise(general, is_live)
    for switch in (None, '1'):
        on = evaluate(field, pts, monkeypatch, switch)
        for name, a, b in zip(NAMES, general, on):
            assert torch.equal(a, b), '%s: HONERF_FAR_TILES=%s differs from the general program (0)' % (name, switch)
    return general


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile(fields, monkeypatch, precision):
    """128 far points: one tile that takes the all-far program, and nothing else in the launch."""
    pts, live = build(torch.zeros(128, dtype=torch.bool), 210)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('where', [(3, 31), (0, 0)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_live_sample_keeps_the_general_program(fields, monkeypatch, precision, where):
    """One tile of far points except one live sample, in lane 31 of wave 3 or in lane 0 of wave 0: three waves are uniform, but the
    workgroup must take the general program."""
    wave, lane = where
    live = torch.zeros(128, dtype=torch.bool)
    live[32 * wave + lane] = True
    pts, live = build(live, 220 + wave)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """229 points, the first tile live in wave 0: the last tile holds 101 samples and 27 pad lanes, copies of the last sample.  With a
    far last sample that tile is all-far; a live one, with far samples in front of it, pulls it into the general program through
    the copies."""
    live = torch.zeros(229, dtype=torch.bool)
    live[:32] = True
    live[228] = last_live
    pts, live = build(live, 240)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('live_pattern', [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_points(fields, monkeypatch, precision, live_pattern):
    """n = 2: one tile of two samples and 126 pad lanes."""
    pts, live = build(torch.tensor(live_pattern), 250)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('pattern', ['far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_programs_alternate_on_one_workgroup(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs) whose programs alternate -- the LDS
    image beside the global slots of the same waves, and the weight stream, its double buffer and the pacing carried from one program
    into the other."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    ws = lambda n: fields('f16x3').lib.hn_field_workspace_bytes(fields('f16x3').handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r in range(3):
        live[r * per_round:(r + 1) * per_round] = (r % 2 == 1) == (pattern == 'far_live_far')
    pts, live = build(live, 260)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_culled_launch_stays_out_of_the_far_program(fields, monkeypatch, precision):
    """hn_field_set_culling on a mixed set -- an all-far tile, a tile with one live wave, a live tile, a padded far tail: the culled
    launch skips weight chunks, which the all-far program never does, so it must keep the general program; its outputs equal the
    launch without culling, with the switch on and off."""
    live = torch.zeros(3 * 128 + 37, dtype=torch.bool)
    live[128 + 64:128 + 96] = True
    live[256:384] = True
    pts, live = build(live, 270)
    field = fields(precision)
    field.set_culling(False)
    dense = check(field, pts, live, monkeypatch)
    field.set_culling(True)
    try:
        for switch in ('0', None):
            culled = evaluate(field, pts, monkeypatch, switch)
            for name, a, b in zip(NAMES, dense, culled):
                assert torch.equal(a, b), '%s: culled launch with HONERF_FAR_TILES=%s differs from the dense one' % (name, switch)
    finally:
        field.set_culling(False)


FOCAL = 2.0


def rays_through(points):
    """Rays of a camera at the origin looking along +z (R = I, T = 0, focal 2) through the given world points."""
    p = torch.as_tensor(np.asarray(points), dtype=torch.float32)
    xy = FOCAL * p[:, :2] / p[:, 2:3]
    p1 = torch.cat([xy / FOCAL, torch.ones(len(p), 1)], dim=-1)
    d = torch.nn.functional.normalize(p1, dim=-1)
    return (p1 - d).contiguous(), d.contiguous()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_render_of_a_small_hand_frame(monkeypatch, precision):
    """NeuSRenderer.render of 12 rays x 32 samples in live-first order at every size (HONERF_LIVE_FIRST=2): six rays pass joints of the
    hand at 5 mm, six miss it, so the ordered list ends in all-far tiles.  Every returned tensor but the scalar `gradient_error` (an
    atomic sum in arrival order, which differs between two runs of one library: tests/test_gpu_live_first_order.py) has the same bits
    with the switch off and on."""
    from honerf_amd.nets import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
    from honerf_amd.renderer import NeuSRenderer
    dev = torch.device('cuda')
    sdf, col, var = SDFNetwork().to(dev), RenderingNetwork(use_gradients=True).to(dev), SingleVarianceNetwork(0.3).to(dev)
    sdf.reset_parameters(21)
    col.reset_parameters(22)
    ren = NeuSRenderer(sdf, var, col, 'hand', 32, 0, 0, 4, 1.0)
    ren.precision = precision
    miss = np.array([[0.5, 0.5, 0.9], [-0.5, 0.5, 0.9], [0.5, -0.5, 0.9], [-0.5, -0.5, 0.9], [0.6, 0.0, 0.9], [0.0, 0.6, 0.9]], dtype=np.float32)
    o, d = rays_through(np.concatenate([JOINTS[[0, 4, 8, 12, 16, 20]] + np.float32(0.005), miss]))
    t_rand = torch.rand(12, 1, generator=torch.Generator().manual_seed(1))
    monkeypatch.setenv('HONERF_LIVE_FIRST', '2')
    monkeypatch.delenv('HONERF_UNIFORM_STASH', raising=False)

    def render(switch):
        monkeypatch.setenv('HONERF_FAR_TILES', switch)
        with torch.no_grad():
            out = ren.render(o.cuda(), d.cuda(), 0.4, 1.5, torch.from_numpy(BT_INV).cuda(), torch.from_numpy(T_POSE).cuda(), None, None, None, 0,
                             t_rand=t_rand.cuda())
        out = {k: v.clone() for k, v in out.items()}
        torch.cuda.synchronize()
        return out

    off, on = render('0'), render('1')
    assert off.keys() == on.keys()
    assert bool(torch.isfinite(off['color_fine']).all())
    for k in off:
        if k == 'gradient_error':
            continue
        assert torch.equal(off[k], on[k]), 'render: %s differs between HONERF_FAR_TILES=0 and 1' % k
