"""The shared epilogue of the all-far tile program of the hand evaluation kernels (HONERF_FAR_EPILOGUE).
In an all-far tile every sample column of a wave holds the same numbers, so the element-wise epilogue of the SDF network's layers
(softplus forward, g sigma' in the reverse sweep, the fp16 hi / lo split behind both) is computed once per row of lanes and handed
round through two LDS lines of the wave instead of once per lane.  HONERF_FAR_EPILOGUE=0 keeps the per-lane epilogue in that program.
Both forms issue the same operations on the same values, so `hn_field_eval` (sdf, gradient, rgb, feature rows) must return the SAME
BITS with the switch off and on (unset and 1), for both precisions.
The method is that of tests/test_gpu_far_tiles.py: launches through the C ABI with a workspace of this file's own, filled with 0xFF
bytes, and into NaN-filled outputs.  "Far" points lie a metre from every joint (all 21 bone masks exactly 0), "live" points 5 mm from
joint 9.
All far samples share ONE network input, so a launch exercises 256 x 15 distinct epilogue values per weight set; the one-tile case
therefore runs on several weight sets, one of them with the SDF biases scaled until the pre-activations of lin1..lin7 cover negative
values, positive values, both sides of softplus's linear threshold (|z| > 0.2) and activations whose fp16 hi part is below 2^-14 --
checked on the CPU with the oracle's forward pass."""
import math

import numpy as np
import pytest
import torch

from honerf_amd import synth

pytestmark = pytest.mark.gpu

BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)
PRECISIONS = ['f16x3', 'f16']
NAMES = ('sdf', 'grad', 'rgb', 'feat')
BIAS_SCALE = 30.0   # synth draws the hidden layers' biases with sigma 0.01


def make_nets(seed, bias_scale=1.0):
    from honerf_amd.nets import SDFNetwork, RenderingNetwork
    dev = torch.device('cuda')
    sdf, col = SDFNetwork().to(dev), RenderingNetwork(use_gradients=True).to(dev)
    sdf.reset_parameters(seed)
    col.reset_parameters(seed + 1)
    if bias_scale != 1.0:
        with torch.no_grad():
            for l in range(8):
                getattr(sdf, 'lin%d' % l).bias.mul_(bias_scale)
    return sdf, col


@pytest.fixture(scope='module')
def fields():
    """One packed hand field per (weight seed, bias scale, precision), made on first use and shared by the cases."""
    from honerf_amd.nets import PackedField
    made = {}

    def get(precision, seed=21, bias_scale=1.0):
        key = (precision, seed, bias_scale)
        if key not in made:
            sdf, col = make_nets(seed, bias_scale)
            made[key] = PackedField('hand', sdf, col, 0.3, precision=precision)
        return made[key]
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
    is_live = torch.as_tensor(is_live, dtype=torch.bool)
    pts = far_points(len(is_live), seed)
    if bool(is_live.any()):
        pts[is_live] = live_points(int(is_live.sum()), seed + 1)
    return pts, is_live


def evaluate(field, pts, monkeypatch, switch):
    """hn_field_eval over `pts` with HONERF_FAR_EPILOGUE=switch (None: unset), on a workspace of 0xFF bytes and into NaN-filled outputs."""
    from honerf_amd import lib as L
    if switch is None:
        monkeypatch.delenv('HONERF_FAR_EPILOGUE', raising=False)
    else:
        monkeypatch.setenv('HONERF_FAR_EPILOGUE', switch)
    monkeypatch.delenv('HONERF_FAR_TILES', raising=False)
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


def check(field, pts, is_live, monkeypatch):
    per_lane = evaluate(field, pts, monkeypatch, '0')
    for o in per_lane:
        assert bool(torch.isfinite(o).all())
    far = ~is_live
    if bool(far.any()):
        sdf, grad = per_lane[0].cpu(), per_lane[1].cpu()
        assert bool((sdf[far] == sdf[far][0]).all()), 'far points do not share one sdf value'
        assert bool((grad[far] == 0.0).all()), 'far points have a non-zero gradient'
    for switch in (None, '1'):
        shared = evaluate(field, pts, monkeypatch, switch)
        for name, a, b in zip(NAMES, per_lane, shared):
            assert torch.equal(a, b), '%s: HONERF_FAR_EPILOGUE=%s differs from the per-lane epilogue (0)' % (name, switch)
    return per_lane


@pytest.mark.parametrize('seed', [21, 31, 41, 51])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile(fields, monkeypatch, precision, seed):
    """128 far points: one tile that takes the all-far program, on four weight sets."""
    pts, live = build(torch.zeros(128, dtype=torch.bool), 310)
    check(fields(precision, seed), pts, live, monkeypatch)


def far_preactivations(sdf_module):
    """(z_l, a_{l+1}) of lin0..lin7 at a far sample (all 1386 features exactly 0), float32 on the CPU, by the oracle's forward pass:
    oracle.nets.hand_sdf_forward's statements with the pre-activations kept."""
    from oracle import nets as onets
    mlp = onets.mlp_from_state_dict({k: v.detach().cpu() for k, v in sdf_module.state_dict().items()})
    pts = far_points(1, 310)
    feat, _, h = onets.hand_features(pts, torch.from_numpy(BT_INV), torch.from_numpy(T_POSE))
    assert bool((h == 0).all()) and bool((feat == 0).all())
    x, zs = feat, []
    for l, (W, b) in enumerate(mlp[:-1]):
        if l == onets.SKIP:
            x = torch.cat([x, feat], dim=1) / math.sqrt(2.0)
        z = torch.nn.functional.linear(x, W, b)
        x = onets.softplus100(z)
        zs.append((z[0], x[0]))
    return zs


@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile_with_spread_preactivations(fields, monkeypatch, precision):
    """The one-tile case on a weight set whose SDF biases are scaled by 30: every one of lin1..lin7 then has negative and positive
    pre-activations on both sides of |z| = 0.2 (softplus's threshold 20 / beta), and activations below 2^-14, whose fp16 hi part is a
    subnormal that the kernels' fp16 mode flushes."""
    sdf, _ = make_nets(61, BIAS_SCALE)
    zs = far_preactivations(sdf)
    assert len(zs) == 8
    for l, (z, a) in enumerate(zs):
        if l == 0:
            continue
        assert float(z.min()) < -0.2 and float(z.max()) > 0.2, 'lin%d: pre-activations span %g .. %g' % (l, float(z.min()), float(z.max()))
        assert bool(((z > -0.2) & (z < 0.0)).any()) and bool(((z > 0.0) & (z < 0.2)).any()), 'lin%d: nothing inside the threshold' % l
        assert bool(((a > 0.0) & (a < 2.0 ** -14)).any()), 'lin%d: no activation with an fp16 hi part below 2^-14' % l
    pts, live = build(torch.zeros(128, dtype=torch.bool), 310)
    check(fields(precision, 61, BIAS_SCALE), pts, live, monkeypatch)


@pytest.mark.parametrize('live_pattern', [(False, False), (False, True)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_points(fields, monkeypatch, precision, live_pattern):
    """n = 2: one tile of two samples and 126 pad lanes, copies of the last sample; waves 1..3 are made of copies alone.  With a live
    last sample the tile takes the general program."""
    pts, live = build(torch.tensor(live_pattern), 320)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """One tile of 100 points and 28 pad lanes, copies of the last sample.  Far: the tile is all-far.  Live, behind 99 far samples: the
    copies pull the tile into the general program, which must match all the same."""
    live = torch.zeros(100, dtype=torch.bool)
    live[99] = last_live
    pts, live = build(live, 330)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('pattern', ['far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_lines_are_reused_tile_after_tile(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs) whose programs alternate, the two LDS
    lines of the shared epilogue and the image beside them reused from tile to tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    f = fields(precision)
    ws = lambda n: f.lib.hn_field_workspace_bytes(f.handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r in range(3):
        live[r * per_round:(r + 1) * per_round] = (r % 2 == 1) == (pattern == 'far_live_far')
    pts, live = build(live, 340)
    check(f, pts, live, monkeypatch)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_culled_launch(fields, monkeypatch, precision):
    """hn_field_set_culling on a mixed set -- an all-far tile, a tile with one live wave, a live tile, a padded far tail: a culled
    launch keeps the general program; its outputs equal the dense launch's with the switch off and on."""
    live = torch.zeros(3 * 128 + 37, dtype=torch.bool)
    live[128 + 64:128 + 96] = True
    live[256:384] = True
    pts, live = build(live, 350)
    field = fields(precision)
    field.set_culling(False)
    dense = check(field, pts, live, monkeypatch)
    field.set_culling(True)
    try:
        for switch in ('0', None):
            culled = evaluate(field, pts, monkeypatch, switch)
            for name, a, b in zip(NAMES, dense, culled):
                assert torch.equal(a, b), '%s: culled launch with HONERF_FAR_EPILOGUE=%s differs from the dense one' % (name, switch)
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
    atomic sum in arrival order) has the same bits with the switch off and on."""
    from honerf_amd.nets import SingleVarianceNetwork
    from honerf_amd.renderer import NeuSRenderer
    dev = torch.device('cuda')
    sdf, col = make_nets(21)
    var = SingleVarianceNetwork(0.3).to(dev)
    ren = NeuSRenderer(sdf, var, col, 'hand', 32, 0, 0, 4, 1.0)
    ren.precision = precision
    miss = np.array([[0.5, 0.5, 0.9], [-0.5, 0.5, 0.9], [0.5, -0.5, 0.9], [-0.5, -0.5, 0.9], [0.6, 0.0, 0.9], [0.0, 0.6, 0.9]], dtype=np.float32)
    o, d = rays_through(np.concatenate([JOINTS[[0, 4, 8, 12, 16, 20]] + np.float32(0.005), miss]))
    t_rand = torch.rand(12, 1, generator=torch.Generator().manual_seed(1))
    monkeypatch.setenv('HONERF_LIVE_FIRST', '2')
    monkeypatch.delenv('HONERF_UNIFORM_STASH', raising=False)
    monkeypatch.delenv('HONERF_FAR_TILES', raising=False)

    def render(switch):
        monkeypatch.setenv('HONERF_FAR_EPILOGUE', switch)
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
        assert torch.equal(off[k], on[k]), 'render: %s differs between HONERF_FAR_EPILOGUE=0 and 1' % k
