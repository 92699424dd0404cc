"""The weight stream of the all-far tile program of the hand evaluation kernels (HONERF_FAR_STREAM).
In an all-far tile the 1386 features are exactly 0: the MFMAs of lin0, of the lin4 skip columns and of colour lin0's feature columns
add W * 0 to their accumulators, and the products of the Jacobian pass are discarded.  With the switch on (the default) the all-far
program runs those MFMAs on a weight chunk that is already resident in LDS and fetches none of the 206 chunks they used to read;
HONERF_FAR_STREAM=0 sends all-far tiles to the all-far program that streams every chunk, and HONERF_FAR_TILES=0 sends every tile to
the general program, which multiplies the real weights: the reference that matters.  `hn_field_eval` (sdf, gradient, rgb, feature
rows) must return the SAME BITS in all of them, for both precisions.
The method is that of tests/test_gpu_far_tiles.py: launches through the C ABI with a workspace of this file's own, filled with 0xFF
bytes, and into NaN-filled outputs.  "Far" points lie a metre from every joint (all 21 bone masks exactly 0), "live" points 5 mm from
joint 9.  One weight set holds values near the top of the fp16 range in every chunk that is no longer fetched for its own MFMAs (the
bones b >= 1 of W0, of W4's skip columns and of colour lin0's feature columns) and small ones in bone 0's and everywhere else."""
import numpy as np
import pytest
import torch

from honerf_amd import synth

pytestmark = pytest.mark.gpu

BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)
PRECISIONS = ['f16x3', 'f16']
NAMES = ('sdf', 'grad', 'rgb', 'feat')
BIAS_SCALE = 30.0    # the fifth weight set of tests/test_gpu_far_epilogue.py: SDF biases scaled until the pre-activations spread
BONE_FEAT = 66       # features per bone; 21 bones = the 1386 feature columns
N_FEAT = 21 * BONE_FEAT
# (name, HONERF_FAR_STREAM, HONERF_FAR_TILES); None: unset.  The last one is the reference.
MODES = (('unset', None, None), ('1', '1', None), ('0', '0', None), ('general', None, '0'))


def make_nets(seed, bias_scale=1.0, big_bones=False):
    from honerf_amd.nets import SDFNetwork, RenderingNetwork
    dev = torch.device('cuda')
    sdf, col = SDFNetwork().to(dev), RenderingNetwork(use_gradients=True).to(dev)
    sdf.reset_parameters(seed)
    col.reset_parameters(seed + 1)
    with torch.no_grad():
        if bias_scale != 1.0:
            for l in range(8):
                getattr(sdf, 'lin%d' % l).bias.mul_(bias_scale)
        if big_bones:
            # W = g v / |v| per row: the feature columns of the bones 1..20 get magnitudes of 30 000 .. 60 000 (fp16 ends at 65 504) with
            # random signs, and g = |v|, so that W is v to fp32 rounding; every other column keeps its drawn, small value
            g = torch.Generator().manual_seed(seed + 7)
            for lin, c0 in ((sdf.lin0, 0), (sdf.lin4, 256), (col.lin0, 0)):
                v = lin.weight_v
                assert v.shape[1] >= c0 + N_FEAT
                n = N_FEAT - BONE_FEAT
                big = (30000.0 + 30000.0 * torch.rand(v.shape[0], n, generator=g)) * (2.0 * torch.randint(0, 2, (v.shape[0], n), generator=g) - 1.0)
                v[:, c0 + BONE_FEAT:c0 + N_FEAT] = big.to(v.device)
                lin.weight_g.copy_(v.norm(dim=1, keepdim=True))
                w = lin.weight_g * v / v.norm(dim=1, keepdim=True)
                assert float(w[:, c0 + BONE_FEAT:c0 + N_FEAT].abs().min()) > 29000.0 and float(w.abs().max()) < 65000.0
                assert float(w[:, c0:c0 + BONE_FEAT].abs().max()) < 10.0
    return sdf, col


@pytest.fixture(scope='module')
def fields():
    """One packed hand field per (weight set, precision), made on first use and shared by the cases."""
    from honerf_amd.nets import PackedField
    made = {}

    def get(precision, seed=21, bias_scale=1.0, big_bones=False):
        key = (precision, seed, bias_scale, big_bones)
        if key not in made:
            sdf, col = make_nets(seed, bias_scale, big_bones)
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


def set_mode(monkeypatch, mode):
    _, stream, tiles = mode
    for var, val in (('HONERF_FAR_STREAM', stream), ('HONERF_FAR_TILES', tiles)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    monkeypatch.delenv('HONERF_FAR_EPILOGUE', raising=False)
    monkeypatch.delenv('HONERF_UNIFORM_STASH', raising=False)


def evaluate(field, pts, monkeypatch, mode):
    """hn_field_eval over `pts` under one of MODES, on a workspace of 0xFF bytes and into NaN-filled outputs."""
    from honerf_amd import lib as L
    set_mode(monkeypatch, mode)
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
    """Every mode against the general program (MODES[-1]); returns the general program's outputs."""
    ref = evaluate(field, pts, monkeypatch, MODES[-1])
    for o in ref:
        assert bool(torch.isfinite(o).all())
    far = ~is_live
    if bool(far.any()):
        sdf, grad = ref[0].cpu(), ref[1].cpu()
        assert bool((sdf[far] == sdf[far][0]).all()), 'far points do not share one sdf value'
        assert bool((grad[far] == 0.0).all()), 'far points have a non-zero gradient'
    for mode in MODES[:-1]:
        got = evaluate(field, pts, monkeypatch, mode)
        for name, a, b in zip(NAMES, ref, got):
            assert torch.equal(a, b), '%s: HONERF_FAR_STREAM %s differs from the general program (HONERF_FAR_TILES=0)' % (name, mode[0])
    return ref


WEIGHT_SETS = [(21, 1.0), (31, 1.0), (41, 1.0), (51, 1.0), (61, BIAS_SCALE)]


@pytest.mark.parametrize('weights', WEIGHT_SETS, ids=lambda w: 'seed%d' % w[0])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile(fields, monkeypatch, precision, weights):
    """128 far points: one tile that takes the all-far program, on the five weight sets of tests/test_gpu_far_epilogue.py."""
    pts, live = build(torch.zeros(128, dtype=torch.bool), 310)
    check(fields(precision, weights[0], weights[1]), pts, live, monkeypatch)


@pytest.mark.parametrize('n_tiles', [1, 3])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_weights_near_the_top_of_the_fp16_range_in_the_chunks_that_are_not_fetched(fields, monkeypatch, precision, n_tiles):
    """Far tiles on the weight set whose bones 1..20 hold |w| of 30 000 .. 60 000 in W0, in W4's skip columns and in colour lin0's
    feature columns: the general program multiplies those weights by the zero features, the all-far programs must give its bits."""
    pts, live = build(torch.zeros(128 * n_tiles - (28 if n_tiles > 1 else 0), dtype=torch.bool), 315)
    check(fields(precision, 71, 1.0, True), pts, live, monkeypatch)


@pytest.mark.parametrize('live_pattern', [(False, False), (False, True)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_points(fields, monkeypatch, precision, live_pattern):
    """n = 2: one tile of two samples and 126 pad lanes, copies of the last sample.  With a live last sample the tile takes the general
    program."""
    pts, live = build(torch.tensor(live_pattern), 320)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """One tile of 100 points and 28 pad lanes, copies of the last sample.  Far: the tile is all-far.  Live, behind 99 far samples: the
    copies pull the tile into the general program."""
    live = torch.zeros(100, dtype=torch.bool)
    live[99] = last_live
    pts, live = build(live, 330)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('pattern', ['far_far_far', 'far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_stream_state_is_handed_from_tile_to_tile(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs).  far / far / far: the resident chunk
    and the stream position carry from one all-far tile to the next; the mixed patterns hand the stream's state (offset, buffer, the
    chunk in flight) between the all-far and the general program in both directions."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    f = fields(precision)
    ws = lambda n: f.lib.hn_field_workspace_bytes(f.handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r, kind in enumerate(pattern.split('_')):
        live[r * per_round:(r + 1) * per_round] = kind == 'live'
    pts, live = build(live, 340)
    check(f, pts, live, monkeypatch)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_culled_launch(fields, monkeypatch, precision):
    """hn_field_set_culling on a mixed set -- an all-far tile, a tile with one live wave, a live tile, a padded far tail: a culled
    launch keeps the general program and the full stream of the bones it runs; its outputs equal the dense launch's in every mode."""
    live = torch.zeros(3 * 128 + 37, dtype=torch.bool)
    live[128 + 64:128 + 96] = True
    live[256:384] = True
    pts, live = build(live, 350)
    field = fields(precision)
    field.set_culling(False)
    dense = check(field, pts, live, monkeypatch)
    field.set_culling(True)
    try:
        for mode in MODES:
            culled = evaluate(field, pts, monkeypatch, mode)
            for name, a, b in zip(NAMES, dense, culled):
                assert torch.equal(a, b), '%s: culled launch (HONERF_FAR_STREAM %s) differs from the dense one' % (name, mode[0])
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
    atomic sum in arrival order) has the general program's bits in every mode."""
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

    def render(mode):
        set_mode(monkeypatch, mode)
        with torch.no_grad():
            out = ren.render(o.cuda(), d.cuda(), 0.4, 1.5, torch.from_numpy(BT_INV).cuda(), torch.from_numpy(T_POSE).cuda(), None, None, None, 0,
                             t_rand=t_rand.cuda())
        out = {k: v.clone() for k, v in out.items()}
        torch.cuda.synchronize()
        return out

    ref = render(MODES[-1])
    assert bool(torch.isfinite(ref['color_fine']).all())
    for mode in MODES[:-1]:
        got = render(mode)
        assert ref.keys() == got.keys()
        for k in ref:
            if k == 'gradient_error':
                continue
            assert torch.equal(ref[k], got[k]), 'render: %s differs between the general program and HONERF_FAR_STREAM %s' % (k, mode[0])
