"""All-far tiles reuse the workgroup's far result ("The far result once per workgroup").
For a sample whose 21 bone masks are 0 the hand field is a function of the weights alone, so sdf, gradient, rgb and the 256 feature
rows are the same for every far sample of a launch.  A workgroup computes them in its FIRST all-far tile of a launch (the all-far
program with the full stream) and keeps them in LDS; every later all-far tile of that workgroup stores them again and runs its MFMAs
on held operands (the reuse program).  `hn_field_eval` (sdf, gradient, rgb, feature rows) must return the SAME BITS as the general
program (HONERF_FAR_TILES=0) and as HONERF_FAR_STREAM=0, which sends every all-far tile to the program that computes, for both
precisions.  The method, the points, the weight sets and the helpers are those of tests/test_gpu_far_stream.py and
tests/test_gpu_far_hold.py: launches through the C ABI with a workspace filled with 0xFF bytes and into NaN-filled outputs.
The existing far tests push far / far / far, far / live / far and a paced mixed launch through the reuse program; the cases here are
the ones where REUSE can go wrong.  Each is a launch of R x CUs x 128 points, so that every workgroup runs R tiles (tile = workgroup +
round x CUs); that the grid is still min(tiles, CUs) is asserted through hn_field_workspace_bytes -- otherwise a case could pass
without a single reused tile."""
import pytest
import torch

import test_gpu_far_hold as fh
import test_gpu_far_stream as fs

pytestmark = pytest.mark.gpu

PRECISIONS = fs.PRECISIONS
NAMES = fs.NAMES
fields = fh.fields   # one packed hand field per (weight set, precision), module-scoped: this module's own instance
check = fh.check     # the default against HONERF_FAR_TILES=0 and against HONERF_FAR_STREAM=0, far points' sdf and gradient
GUARD = 64           # rows behind row n of every output that no launch may write


def per_round():
    return torch.cuda.get_device_properties(0).multi_processor_count * 128


def assert_grid(f, rounds):
    """Every workgroup of a launch of `rounds` x CUs x 128 points runs `rounds` tiles."""
    ws = lambda n: f.lib.hn_field_workspace_bytes(f.handle, n)
    assert ws(rounds * per_round()) == ws(per_round()) > ws(per_round() - 128), 'the launch grid is no longer min(tiles, CUs)'


def rounds_of(pattern, seed):
    """One round of CUs x 128 points per word of `pattern` ('far_live_far'); -> (pts, is_live)"""
    kinds = pattern.split('_')
    live = torch.zeros(len(kinds) * per_round(), dtype=torch.bool)
    for r, kind in enumerate(kinds):
        live[r * per_round():(r + 1) * per_round()] = kind == 'live'
    return fs.build(live, seed)


def launch(field, pts, monkeypatch, mode, want_feat=True, ws=None):
    """fs.evaluate with a guard band of GUARD NaN rows behind row n of every output, the feature rows on request, and optionally on
    a workspace of the caller's that is NOT filled again.  -> the outputs with their guard rows ([n + GUARD, ...]; feat None if not
    requested)"""
    from honerf_amd import lib as L
    fs.set_mode(monkeypatch, mode)
    lib = field.lib
    p = pts.cuda().contiguous()
    dirs = torch.nn.functional.normalize(p, dim=-1).contiguous()
    bt, tp = torch.from_numpy(fs.BT_INV).cuda().contiguous(), torch.from_numpy(fs.T_POSE).cuda().contiguous()
    n = p.shape[0]
    out = [torch.full((n + GUARD,) + s, float('nan'), device='cuda') for s in ((), (3,), (3,), (256,))]
    if not want_feat:
        out[3] = None
    need = lib.hn_field_workspace_bytes(field.handle, n)
    if ws is None:
        ws = torch.full((max(need, 16),), 0xFF, dtype=torch.uint8, device='cuda')
    assert ws.numel() >= need
    rc = lib.hn_field_eval(field.handle, L.ptr(p), L.ptr(dirs), n, 1, L.ptr(bt), L.ptr(tp), 1, n, L.ptr(out[0]), L.ptr(out[1]),
                           L.ptr(out[2]), L.ptr(out[3]), L.ptr(ws), need, L.stream_ptr())
    L.check(rc, 'hn_field_eval')
    torch.cuda.synchronize()
    return out


def assert_same(ref, got, n, what):
    """Rows 0 .. n - 1 of `got` (with guard rows) are `ref`'s (without), and its guard rows are still NaN."""
    for name, a, b in zip(NAMES, ref, got):
        if b is None:
            continue
        assert torch.equal(a[:n], b[:n]), '%s: %s' % (name, what)
        assert bool(torch.isnan(b[n:]).all()), '%s: rows behind row n were written (%s)' % (name, what)


@pytest.mark.parametrize('weights', fh.WEIGHT_SETS, ids=lambda w: '%s%d' % (w[0], w[1]))
@pytest.mark.parametrize('precision', PRECISIONS)
def test_far_far_on_every_weight_set(fields, monkeypatch, precision, weights):
    """R = 2, all far: the second tile of every workgroup comes from the saved result.  The sets with weights near the top of the fp16
    range are where the held fragment comes from (bone 0's chunks of lin0)."""
    f = fields(precision, *weights)
    assert_grid(f, 2)
    pts, live = rounds_of('far_far', 610)
    check(f, pts, live, monkeypatch)


MIXED = ['live_far_far', 'far_far_live_far', 'live_live_far']


@pytest.fixture(scope='module')
def mixed_general(fields):
    """The general program's outputs for the MIXED patterns, computed once per (precision, pattern) and shared by the cases below."""
    made = {}

    def get(precision, pattern, monkeypatch):
        key = (precision, pattern)
        if key not in made:
            pts, live = rounds_of(pattern, 620)
            made[key] = (pts, live, fs.evaluate(fields(precision), pts, monkeypatch, fh.GENERAL))
        return made[key]
    return get


@pytest.mark.parametrize('pattern', MIXED)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_the_saved_result_survives_general_tiles(fields, mixed_general, monkeypatch, precision, pattern):
    """live / far / far, far / far / live / far and live / live / far: the saved result survives a general tile, and a workgroup whose
    first all-far tile is not its first tile computes it then."""
    f = fields(precision)
    assert_grid(f, len(pattern.split('_')))
    pts, live, ref = mixed_general(precision, pattern, monkeypatch)
    far = ~live
    assert bool((ref[0].cpu()[far] == ref[0].cpu()[far][0]).all()) and bool((ref[1].cpu()[far] == 0.0).all())
    for mode in (fh.DEFAULT, fh.STREAM_OFF):
        assert_same(ref, launch(f, pts, monkeypatch, mode), len(pts), 'mode %s differs from the general program' % mode[0])


@pytest.mark.parametrize('pattern', MIXED)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_culled_and_general_launches_never_reuse(fields, mixed_general, monkeypatch, precision, pattern):
    """A culled launch and a HONERF_FAR_TILES=0 launch of the same points keep the general program: their outputs are unchanged."""
    f = fields(precision)
    pts, live, ref = mixed_general(precision, pattern, monkeypatch)
    assert_same(ref, launch(f, pts, monkeypatch, fh.GENERAL), len(pts), 'HONERF_FAR_TILES=0 is not reproducible')
    f.set_culling(True)
    try:
        for mode in (fh.DEFAULT, fh.STREAM_OFF, fh.GENERAL):
            assert_same(ref, launch(f, pts, monkeypatch, mode), len(pts), 'culled launch (mode %s) differs from the dense one' % mode[0])
    finally:
        f.set_culling(False)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_last_tile_is_a_padded_reuse_tile(fields, monkeypatch, precision):
    """n = 2 x CUs x 128 - 28, all far: the last tile is a reuse tile with 28 pad lanes; nothing is stored behind row n."""
    f = fields(precision)
    assert_grid(f, 2)
    pts, live = fs.build(torch.zeros(2 * per_round() - 28, dtype=torch.bool), 630)
    ref = fs.evaluate(f, pts, monkeypatch, fh.GENERAL)
    assert bool((ref[0] == ref[0][0]).all()) and bool((ref[1] == 0.0).all())
    for mode in (fh.DEFAULT, fh.STREAM_OFF):
        assert_same(ref, launch(f, pts, monkeypatch, mode), len(pts), 'mode %s differs from the general program' % mode[0])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_partial_tile_computes_the_result(fields, monkeypatch, precision):
    """n = CUs x 128 + 100 with the first CUs x 128 points live: the one partial tile is the first all-far tile of its workgroup and
    computes the result, with 28 pad lanes; nothing is stored behind row n."""
    f = fields(precision)
    assert_grid(f, 2)
    live = torch.zeros(per_round() + 100, dtype=torch.bool)
    live[:per_round()] = True
    pts, live = fs.build(live, 640)
    ref = fs.evaluate(f, pts, monkeypatch, fh.GENERAL)
    for mode in (fh.DEFAULT, fh.STREAM_OFF):
        assert_same(ref, launch(f, pts, monkeypatch, mode), len(pts), 'mode %s differs from the general program' % mode[0])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_nothing_survives_a_launch(fields, monkeypatch, precision):
    """Two fields of different weight sets launched alternately (A, B, A) on ONE workspace buffer that is not filled again between the
    launches: each launch equals its own general-program result, and the far sdf of A differs from that of B."""
    fa, fb = fields(precision, 'plain', 21), fields(precision, 'plain', 31)
    assert_grid(fa, 3)
    pts, live = rounds_of('far_far_far', 650)
    n = len(pts)
    refs = [fs.evaluate(f, pts, monkeypatch, fh.GENERAL) for f in (fa, fb)]
    assert float(refs[0][0][0]) != float(refs[1][0][0]), 'the two weight sets give the same far sdf: pick another pair'
    need = max(f.lib.hn_field_workspace_bytes(f.handle, n) for f in (fa, fb))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device='cuda')
    for f, ref, name in ((fa, refs[0], 'A'), (fb, refs[1], 'B'), (fa, refs[0], 'A again')):
        assert_same(ref, launch(f, pts, monkeypatch, fh.DEFAULT, ws=ws), n, 'launch %s differs from its own general-program result' % name)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_feature_rows_on_request(fields, monkeypatch, precision):
    """One far / far launch with the feature rows requested and one with NULL in their place: sdf, gradient and rgb are the same."""
    f = fields(precision)
    assert_grid(f, 2)
    pts, live = rounds_of('far_far', 660)
    n = len(pts)
    ref = fs.evaluate(f, pts, monkeypatch, fh.GENERAL)
    with_rows = launch(f, pts, monkeypatch, fh.DEFAULT)
    without = launch(f, pts, monkeypatch, fh.DEFAULT, want_feat=False)
    assert_same(ref, with_rows, n, 'the default with feature rows differs from the general program')
    assert_same(ref, without, n, 'the default without feature rows differs from the general program')
    for name, a, b in zip(NAMES[:3], with_rows, without):
        assert torch.equal(a[:n], b[:n]), '%s depends on whether the feature rows are requested' % name
