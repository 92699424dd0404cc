"""The all-far tile program's discarded products keep their operands in registers ("held operands").
In an all-far tile the MFMAs over the feature space multiply the zero fragment (lin0, the lin4 skip columns, colour lin0's feature
columns) or their results are discarded (the Jacobian pass).  Since HONERF_FAR_STREAM they read one weight chunk that stays resident
in LDS; now the groups on the resident chunk read nothing at all: their A operand is ONE k-step of that chunk, loaded into registers
once per pass, and the Jacobian pass's B operand is the zero fragment as well.  A finite weight times +-0 is +-0 whichever weight it
is, so `hn_field_eval` (sdf, gradient, rgb, feature rows) must return the SAME BITS as the general program (HONERF_FAR_TILES=0), which
multiplies the real weights, and as the all-far program that streams every chunk (HONERF_FAR_STREAM=0), for both precisions.
The method, the points and the helpers are those of tests/test_gpu_far_stream.py: launches through the C ABI with a workspace filled
with 0xFF bytes and into NaN-filled outputs.  Beside that file's weight sets, one holds values near the top of the fp16 range exactly
where the held fragments come from: bone 0's feature columns (the resident chunk of a feature pass is bone 0's second chunk) and the
leftover block's columns (the resident chunk of the Jacobian pass is the leftover block's second), in W0, in W4's skip columns and in
colour lin0."""
import numpy as np
import pytest
import torch

import test_gpu_far_stream as fs

pytestmark = pytest.mark.gpu

PRECISIONS = fs.PRECISIONS
NAMES = fs.NAMES
# (name, HONERF_FAR_STREAM, HONERF_FAR_TILES); None: unset.  The first one is the default, the one under test.
DEFAULT, STREAM_OFF, GENERAL = ('unset', None, None), ('0', '0', None), ('general', None, '0')
LEFT_COLS = [fs.BONE_FEAT * b + c for b in range(21) for c in (22, 23)]   # (r_1 | r_2) h of every bone: the leftover block (hn_pack2.hip)
HELD_COLS = sorted(set(range(fs.BONE_FEAT)) | set(LEFT_COLS))


def make_nets(kind, seed, bias_scale=1.0):
    """kind 'plain' / 'big_bones': the sets of tests/test_gpu_far_stream.py.  'big_held': |w| of 30 000 .. 60 000 with random signs in
    bone 0's 66 feature columns and in the 42 leftover columns of W0, of W4's skip part and of colour lin0; every other column keeps its
    drawn, small value (W = g v / |v| per row with g = |v|, so that W is v to fp32 rounding)."""
    sdf, col = fs.make_nets(seed, bias_scale, kind == 'big_bones')
    if kind == 'big_held':
        g = torch.Generator().manual_seed(seed + 11)
        with torch.no_grad():
            for lin, c0 in ((sdf.lin0, 0), (sdf.lin4, 256), (col.lin0, 0)):
                v = lin.weight_v
                assert v.shape[1] >= c0 + fs.N_FEAT
                cols = torch.tensor([c0 + c for c in HELD_COLS], device=v.device)
                n = len(HELD_COLS)
                big = (30000.0 + 30000.0 * torch.rand(v.shape[0], n, generator=g)) * (2.0 * torch.randint(0, 2, (v.shape[0], n), generator=g) - 1.0)
                v[:, cols] = big.to(v.device)
                lin.weight_g.copy_(v.norm(dim=1, keepdim=True))
                w = lin.weight_g * v / v.norm(dim=1, keepdim=True)
                assert float(w[:, cols].abs().min()) > 29000.0 and float(w.abs().max()) < 65000.0
                rest = torch.ones(v.shape[1], dtype=torch.bool, device=v.device)
                rest[cols] = False
                assert float(w[:, rest].abs().max()) < 10.0
    return sdf, col


@pytest.fixture(scope='module')
def fields():
    """One packed hand field per (weight set, precision), made on first use and shared by the cases."""
    from honerf_amd.nets import PackedField
    made = {}

    def get(precision, kind='plain', seed=21, bias_scale=1.0):
        key = (precision, kind, seed, bias_scale)
        if key not in made:
            sdf, col = make_nets(kind, seed, bias_scale)
            made[key] = PackedField('hand', sdf, col, 0.3, precision=precision)
        return made[key]
    yield get
    for f in made.values():
        f.set_culling(False)


def check(field, pts, is_live, monkeypatch):
    """The default against the general program and against HONERF_FAR_STREAM=0; returns the default's outputs."""
    got = fs.evaluate(field, pts, monkeypatch, DEFAULT)
    for o in got:
        assert bool(torch.isfinite(o).all())
    far = ~is_live
    if bool(far.any()):
        sdf, grad = got[0].cpu(), got[1].cpu()
        assert bool((sdf[far] == sdf[far][0]).all()), 'far points do not share one sdf value'
        assert bool((grad[far] == 0.0).all()), 'far points have a non-zero gradient'
    for mode in (GENERAL, STREAM_OFF):
        ref = fs.evaluate(field, pts, monkeypatch, mode)
        for name, a, b in zip(NAMES, ref, got):
            assert torch.equal(a, b), '%s: the default differs from %s' % (name, 'the general program (HONERF_FAR_TILES=0)' if mode is GENERAL else 'HONERF_FAR_STREAM=0')
    return got


WEIGHT_SETS = [('plain', s, b) for s, b in fs.WEIGHT_SETS] + [('big_bones', 71, 1.0), ('big_held', 81, 1.0)]


@pytest.mark.parametrize('weights', WEIGHT_SETS, ids=lambda w: '%s%d' % (w[0], w[1]))
@pytest.mark.parametrize('precision', PRECISIONS)
def test_one_far_tile(fields, monkeypatch, precision, weights):
    """128 far points: one tile that takes the all-far program, on every weight set."""
    pts, live = fs.build(torch.zeros(128, dtype=torch.bool), 410)
    check(fields(precision, *weights), pts, live, monkeypatch)


@pytest.mark.parametrize('kind', ['big_bones', 'big_held'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_three_far_tiles_on_the_large_weights(fields, monkeypatch, precision, kind):
    """Two whole far tiles and a padded third on the two sets with weights near the top of the fp16 range: the general program
    multiplies them by the zero features, the all-far program multiplies ONE held k-step of them instead."""
    pts, live = fs.build(torch.zeros(3 * 128 - 28, dtype=torch.bool), 415)
    check(fields(precision, kind, 71 if kind == 'big_bones' else 81), pts, live, monkeypatch)


@pytest.mark.parametrize('live_pattern', [(False, False), (False, True)])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_points(fields, monkeypatch, precision, live_pattern):
    """n = 2: one tile of two samples and 126 pad lanes, copies of the last sample.  With a live last sample the tile takes the general
    program."""
    pts, live = fs.build(torch.tensor(live_pattern), 420)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('last_live', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_padded_tail(fields, monkeypatch, precision, last_live):
    """One tile of 100 points and 28 pad lanes, copies of the last sample.  Far: the tile is all-far.  Live, behind 99 far samples: the
    copies pull the tile into the general program."""
    live = torch.zeros(100, dtype=torch.bool)
    live[99] = last_live
    pts, live = fs.build(live, 430)
    check(fields(precision), pts, live, monkeypatch)


@pytest.mark.parametrize('pattern', ['far_far_far', 'far_live_far', 'live_far_live'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_three_tiles_per_workgroup(fields, monkeypatch, precision, pattern):
    """3 x CUs x 128 points: every workgroup runs three tiles (tile = workgroup + round x CUs).  far / far / far: the held fragments are
    loaded again in every pass of every tile from the chunk that pass made resident; the mixed patterns hand the stream's state between
    the all-far and the general program in both directions, with the passes' exit states unchanged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 128
    f = fields(precision)
    ws = lambda n: f.lib.hn_field_workspace_bytes(f.handle, n)
    assert ws(3 * per_round) == ws(per_round) > ws(per_round - 128), 'the launch grid is no longer min(tiles, CUs)'
    live = torch.zeros(3 * per_round, dtype=torch.bool)
    for r, kind in enumerate(pattern.split('_')):
        live[r * per_round:(r + 1) * per_round] = kind == 'live'
    pts, live = fs.build(live, 440)
    check(f, pts, live, monkeypatch)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_culled_launch(fields, monkeypatch, precision):
    """hn_field_set_culling on a mixed set -- an all-far tile, a tile with one live wave, a live tile, a padded far tail: a culled
    launch keeps the general program; its outputs equal the dense launch's in every mode."""
    live = torch.zeros(3 * 128 + 37, dtype=torch.bool)
    live[128 + 64:128 + 96] = True
    live[256:384] = True
    pts, live = fs.build(live, 450)
    field = fields(precision)
    field.set_culling(False)
    dense = check(field, pts, live, monkeypatch)
    field.set_culling(True)
    try:
        for mode in (DEFAULT, STREAM_OFF, GENERAL):
            culled = fs.evaluate(field, pts, monkeypatch, mode)
            for name, a, b in zip(NAMES, dense, culled):
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
    sdf, col = make_nets('plain', 21)
    var = SingleVarianceNetwork(0.3).to(dev)
    ren = NeuSRenderer(sdf, var, col, 'hand', 32, 0, 0, 4, 1.0)
    ren.precision = precision
    miss = np.array([[0.5, 0.5, 0.9], [-0.5, 0.5, 0.9], [0.5, -0.5, 0.9], [-0.5, -0.5, 0.9], [0.6, 0.0, 0.9], [0.0, 0.6, 0.9]], dtype=np.float32)
    o, d = fs.rays_through(np.concatenate([fs.JOINTS[[0, 4, 8, 12, 16, 20]] + np.float32(0.005), miss]))
    t_rand = torch.rand(12, 1, generator=torch.Generator().manual_seed(1))
    monkeypatch.setenv('HONERF_LIVE_FIRST', '2')

    def render(mode):
        fs.set_mode(monkeypatch, mode)
        with torch.no_grad():
            out = ren.render(o.cuda(), d.cuda(), 0.4, 1.5, torch.from_numpy(fs.BT_INV).cuda(), torch.from_numpy(fs.T_POSE).cuda(), None, None, None, 0,
                             t_rand=t_rand.cuda())
        out = {k: v.clone() for k, v in out.items()}
        torch.cuda.synchronize()
        return out

    got = render(DEFAULT)
    assert bool(torch.isfinite(got['color_fine']).all())
    for mode in (GENERAL, STREAM_OFF):
        ref = render(mode)
        assert ref.keys() == got.keys()
        for k in ref:
            if k == 'gradient_error':
                continue
            assert torch.equal(ref[k], got[k]), 'render: %s differs between the default and mode %s' % (k, mode[0])
