"""GPU tests of the mesh components kernels: hn_meshcc.hip through honerf_amd.mesh_components and the C ABI, against the numpy
restatement of tests/meshcc_cases.py (tests/test_meshcc_cpu.py: that restatement is a breadth-first search's labelling).  Labels,
component indices, counts, bounds, closedness and everything the compaction returns are integers or bit copies and must be EQUAL; area
and volume are held to the summation bound |got - fsum| <= (n_faces + 8) * 2^-52 * sum |term|: the standard bound of a sum of n_faces
terms in any order, plus a few roundings per term; nothing in it is measured."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshcc_cases as cc
from helpers import bounded, product_modules, t as tt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL_KEYS = ('label', 'vertex_label', 'face_label', 'vertex_component', 'face_component')
EPS = 2.0 ** -52


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


@pytest.fixture(scope='module')
def mcomp():
    from honerf_amd import mesh_components
    return mesh_components


@pytest.fixture(scope='module')
def L():
    from honerf_amd import lib
    return lib


def check_labels(got, ref, tag):
    assert got['n'] == ref['n'], (tag, got['n'], ref['n'])
    for k in LABEL_KEYS:
        g = _np(got[k])
        assert g.dtype == np.int32 and got[k].is_cuda, (tag, k, g.dtype)
        assert np.array_equal(g, ref[k]), '%s: %s differs at %d places' % (tag, k, (g != ref[k]).sum() if g.shape == ref[k].shape else -1)


def check_measures(got, ref, tag):
    for k in ('faces', 'vertices'):
        assert _np(got[k]).dtype == np.int64 and np.array_equal(_np(got[k]), ref[k]), (tag, k)
    assert _np(got['bounds']).dtype == ref['bounds'].dtype and np.array_equal(_np(got['bounds']), ref['bounds']), tag + ': bounds'
    assert _np(got['closed']).dtype == np.bool_ and np.array_equal(_np(got['closed']), ref['closed']), tag + ': closed'
    for k in ('area', 'volume'):
        g = _np(got[k])
        assert g.dtype == np.float64
        for c in range(len(g)):
            allowed = (ref['faces'][c] + 8) * EPS * ref[k + '_abs'][c]
            err = abs(float(g[c]) - float(ref[k][c]))
            if len(g) <= 4 or c == int(np.argmax(ref['faces'])):
                bounded('%s: %s of component %d against fsum, as a fraction of the summation bound' % (tag, k, c), err / allowed if allowed else err, 1.0,
                        kind='fraction of bound')
            assert err <= allowed, '%s: %s of component %d: |%r - %r| = %.3e > %.3e' % (tag, k, c, g[c], ref[k][c], err, allowed)


# ---- 1. labels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cc.NAMES)
def test_labels_are_the_restatements(mcomp, name):
    v, t = cc.mesh(name)
    got = mcomp.components((v, t))
    ref = cc.comps(name)
    check_labels(got, ref, 'meshcc ' + name)
    used = np.zeros(len(v), bool)
    used[t.reshape(-1)] = True
    assert np.array_equal(_np(got['vertex_label']) == -1, ~used) and np.array_equal(_np(got['vertex_component']) == -1, ~used)
    if name in ('blobs24', 'soup_gaps'):                        # int32 triangles, tensors on the device
        again = mcomp.components((torch.from_numpy(v).cuda(), torch.from_numpy(t.astype(np.int32)).cuda()))
        check_labels(again, ref, 'meshcc %s (int32 triangles)' % name)


def _raw_label(L, tris, n_verts, **over):
    """hn_meshcc_label on canary-filled outputs; `over` replaces arguments: t (the triangles' pointer), V, T, ws, bytes, or an output's name."""
    lib = L.load()
    V, T = over.get('V', n_verts), over.get('T', tris.shape[0])
    i32 = dict(dtype=torch.int32, device='cuda')
    nv, nt = max(n_verts, 1), max(tris.shape[0], 1)
    out = dict(vertex_label=torch.full((nv,), -7, **i32), face_label=torch.full((nt,), -7, **i32), vertex_component=torch.full((nv,), -7, **i32),
               face_component=torch.full((nt,), -7, **i32), label=torch.full((nv,), -7, **i32), total=torch.full((1,), -7, dtype=torch.int64, device='cuda'))
    ws = torch.empty(max(int(lib.hn_meshcc_workspace_bytes(n_verts, tris.shape[0])), 256), dtype=torch.uint8, device='cuda')
    a = dict(t=L.ptr(tris), V=V, T=T, ws=L.ptr(ws), bytes=ws.numel(), **{k: L.ptr(x) for k, x in out.items()})
    a.update(over)
    rc = lib.hn_meshcc_label(a['t'], a['V'], a['T'], a['vertex_label'], a['face_label'], a['vertex_component'], a['face_component'], a['label'],
                             a['total'], a['ws'], a['bytes'], L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def test_out_of_range_triangle_through_the_abi(mcomp, L):
    v, t = cc.mesh('soup257')
    bad = np.concatenate([t[:100], [[t[3, 0], t[8, 1], len(v)]], t[100:], [[-1, t[4, 0], t[6, 0]]]])
    ref = cc.np_components(bad, len(v))
    assert (ref['face_label'][[100, -1]] == -1).all() and ref['n'] == 257
    rc, out = _raw_label(L, torch.from_numpy(bad).cuda(), len(v))
    assert rc == 0
    assert int(out['total'].item()) == ref['n']
    for k in LABEL_KEYS[1:]:
        assert np.array_equal(_np(out[k]), ref[k]), k
    assert np.array_equal(_np(out['label'])[:ref['n']], ref['label'])
    with pytest.raises(ValueError, match='triangle indices outside'):
        mcomp.components((v, bad))


# ---- 2. order independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['noise', 'strip', 'fan_high'])
def test_labels_do_not_depend_on_order_or_schedule(mcomp, name):
    v, t = cc.mesh(name)
    vd, td = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    first = mcomp.components((vd, td))
    perm = torch.randperm(len(t), generator=torch.Generator().manual_seed(7)).cuda()
    shuffled = mcomp.components((vd, td[perm]))
    assert torch.equal(shuffled['vertex_label'], first['vertex_label']) and torch.equal(shuffled['vertex_component'], first['vertex_component'])
    assert torch.equal(shuffled['face_label'], first['face_label'][perm]) and torch.equal(shuffled['face_component'], first['face_component'][perm])
    for shift in (1, 2):
        rolled = mcomp.components((vd, torch.roll(td, shift, 1).contiguous()))
        assert all(torch.equal(rolled[k], first[k]) for k in LABEL_KEYS), (name, shift)
    second = mcomp.components((vd, td))
    assert all(torch.equal(second[k], first[k]) for k in LABEL_KEYS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = mcomp.components((vd, td))
        meas_side = mcomp.measure((vd, td), on_side)
    side.synchronize()
    assert on_side['n'] == first['n'] and all(torch.equal(on_side[k], first[k]) for k in LABEL_KEYS)
    meas = mcomp.measure((vd, td), first)
    assert all(torch.equal(meas_side[k], meas[k]) for k in meas)


# ---- 3. measures ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in cc.NAMES if not n.startswith('empty')])
def test_measures(mcomp, name):
    v, t = cc.mesh(name)
    got = mcomp.measure((v, t))
    ref = cc.measures(name)
    check_measures(got, ref, 'meshcc ' + name)
    again = mcomp.measure((v, t), mcomp.components((v, t)))
    assert all(torch.equal(again[k], got[k]) for k in got), 'a second call'
    other = np.float64 if v.dtype == np.float32 else np.float32
    if other == np.float64 or np.array_equal(v.astype(np.float32).astype(np.float64), v):
        cast = mcomp.measure((v.astype(other), t))
        assert cast['bounds'].dtype == (torch.float64 if other == np.float64 else torch.float32)
        for k in ('faces', 'vertices', 'area', 'volume', 'closed'):
            assert torch.equal(cast[k], got[k]), 'fp32 against fp64 vertices of the same values: ' + k
        assert torch.equal(cast['bounds'].double(), got['bounds'].double())


def test_closed_is_is_closed_per_component(mcomp):
    from honerf_amd.interaction import is_closed
    for name in ('blobs24', 'noise', 'pinch', 'soup_extras'):
        v, t = cc.mesh(name)
        comps = mcomp.components((v, t))
        closed = _np(mcomp.measure((v, t), comps)['closed'])
        fc = _np(comps['face_component'])
        assert closed.tolist() == [is_closed(t[fc == c]) for c in range(comps['n'])], name


# ---- 4. compaction -------------------------------------------------------------------------------------------------------------------------
def _criteria(name):
    C = cc.comps(name)['n']
    mask = np.zeros(C, bool)
    mask[[0, C // 2, C - 1]] = True
    return [dict(largest=1), dict(largest=2), dict(min_faces=2), dict(closed_only=True), dict(min_area_fraction=0.01), dict(mask=mask)]


def check_keep(mcomp, v, t, crit, tag):
    ref_c = cc.np_components(t, len(v))
    ref_m = cc.np_measure(v, t, ref_c)
    sel = cc.np_select(ref_m, **crit)
    kv, kt, vmap, fmap, kept = cc.np_keep(v, t, sel, ref_c)
    gv, gt, info = mcomp.keep((v, t), **crit)
    assert gv.is_cuda and gt.is_cuda and _np(gv).dtype == v.dtype and gt.dtype == torch.int64 and tuple(gv.shape) == kv.shape and tuple(gt.shape) == kt.shape
    assert np.array_equal(_np(info['kept']), kept), (tag, _np(info['kept']), kept)
    assert _np(gv).tobytes() == kv.tobytes(), tag + ': vertices'
    assert np.array_equal(_np(gt), kt), tag + ': triangles'
    assert _np(info['vertex_map']).dtype == np.int32 and np.array_equal(_np(info['vertex_map']), vmap), tag + ': vertex_map'
    assert _np(info['face_map']).dtype == np.int32 and np.array_equal(_np(info['face_map']), fmap), tag + ': face_map'
    assert _np(gv).tobytes() == v[_np(info['vertex_map']) >= 0].tobytes(), tag + ': a bit copy of the kept rows, in order'
    for k in ('faces', 'vertices', 'closed'):
        assert np.array_equal(_np(info[k]), ref_m[k][kept]), (tag, k)
    after = mcomp.components((gv, gt))
    assert after['n'] == len(kept) and bool((after['vertex_label'] >= 0).all()), tag
    return gv, gt, info


@pytest.mark.parametrize('name', ['blobs24', 'noise', 'soup_extras'])
def test_keep_is_the_restatements(mcomp, name):
    v, t = cc.mesh(name)
    for crit in _criteria(name):
        check_keep(mcomp, v, t, crit, 'meshcc %s keep(%s)' % (name, ', '.join(crit)))
    C = cc.comps(name)['n']
    gv, gt, info = check_keep(mcomp, v, t, dict(mask=np.ones(C, bool)), 'meshcc %s keep(all)' % name)
    used = np.zeros(len(v), bool)
    used[t.reshape(-1)] = True
    assert _np(gv).tobytes() == v[used].tobytes() and gt.shape[0] == len(t)
    gv, gt, info = check_keep(mcomp, v.astype(np.float64), t, dict(mask=np.zeros(C, bool)), 'meshcc %s keep(none)' % name)
    assert tuple(gv.shape) == (0, 3) and gv.dtype == torch.float64 and tuple(gt.shape) == (0, 3) and info['kept'].numel() == 0
    assert bool((info['vertex_map'] == -1).all()) and bool((info['face_map'] == -1).all())


def test_largest_and_comps_argument(mcomp):
    v, t = cc.mesh('noise')
    comps = mcomp.components((v, t))
    a = mcomp.keep((v, t), comps, largest=1)
    b = mcomp.largest((v, t))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].shape[0] == 19716
    both = mcomp.keep((v, t), comps, largest=3, min_faces=40)               # AND: of the three largest, those with 40 faces
    assert _np(both[2]['faces']).tolist() == [19716, 48]


# ---- 5. refusals and empties ---------------------------------------------------------------------------------------------------------------
def test_python_refusals(mcomp):
    v, t = cc.mesh('blobs24')
    with pytest.raises(ValueError, match='CUDA tensor'):
        mcomp.components((torch.from_numpy(v), t))
    with pytest.raises(ValueError, match='dtype'):
        mcomp.components((v.astype(np.float16), t))
    with pytest.raises(ValueError, match='dtype'):
        mcomp.components((v, t.astype(np.float32)))
    with pytest.raises(ValueError, match='shape'):
        mcomp.components((v[:, :2], t))
    with pytest.raises(ValueError, match='shape'):
        mcomp.measure((v, t.reshape(-1)))
    with pytest.raises(ValueError, match='no criterion'):
        mcomp.keep((v, t))
    with pytest.raises(ValueError, match='mask'):
        mcomp.keep((v, t), mask=np.ones(4, bool))
    with pytest.raises(ValueError, match='largest'):
        mcomp.keep((v, t), largest=0)
    with pytest.raises(ValueError, match='comps'):
        mcomp.measure((v, t), mcomp.components(cc.mesh('sphere20')))


def test_abi_refusals_launch_nothing(L):
    lib = L.load()
    v, t = cc.mesh('blobs24')
    td = torch.from_numpy(t).cuda()
    V = len(v)
    outs = []
    for over, word in (({'t': None}, 'NULL'), ({'vertex_label': None}, 'NULL'), ({'total': None}, 'NULL'), ({'ws': None}, 'NULL'), ({'V': -1}, 'n_verts'),
                       ({'T': -1}, 'n_tris'), ({'T': 2 ** 31 - 256}, 'n_tris'), ({'V': 2 ** 31 - 256}, 'n_verts'), ({'bytes': 255}, 'workspace')):
        rc, out = _raw_label(L, td, V, **over)
        assert rc == -1, over
        assert word in lib.hn_last_error().decode(), (over, lib.hn_last_error())
        outs.append(out)
    rc, out = _raw_label(L, td, V, T=0)
    assert rc == 0
    rc, out2 = _raw_label(L, td, V, T=0, t=None, ws=None, bytes=0)
    assert rc == 0
    for o in outs + [out, out2]:
        assert all(bool((x == -7).all()) for x in o.values()), 'a refused / empty call wrote an output'
    # measure and the compaction: NULL, negative count, short workspace
    comps = cc.comps('blobs24')
    vd = torch.from_numpy(v).cuda()
    vc, fc = torch.from_numpy(comps['vertex_component']).cuda(), torch.from_numpy(comps['face_component']).cuda()
    order = torch.sort(fc, stable=True).indices.contiguous()
    C, T = comps['n'], len(t)
    o64 = lambda *s: torch.full(s, -7, dtype=torch.int64, device='cuda')
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device='cuda')
    faces, nv, area, vol, bounds = o64(C), o64(C), f64(C), f64(C), torch.full((C, 6), -7.0, device='cuda')
    ws = torch.empty(int(lib.hn_meshcc_measure_workspace_bytes(T, C)), dtype=torch.uint8, device='cuda')
    p = L.ptr

    def meas(**a):
        return lib.hn_meshcc_measure(a.get('v', p(vd)), 0, a.get('V', V), p(td), a.get('T', T), p(vc), p(fc), a.get('order', p(order)), a.get('C', C),
                                     p(faces), p(nv), a.get('area', p(area)), p(vol), p(bounds), a.get('ws', p(ws)), a.get('bytes', ws.numel()),
                                     L.stream_ptr())
    for over, word in (({'v': None}, 'NULL'), ({'order': None}, 'NULL'), ({'area': None}, 'NULL'), ({'ws': None}, 'NULL'), ({'T': -1}, 'n_tris'),
                       ({'C': -1}, 'n_comp'), ({'V': -2}, 'n_verts'), ({'bytes': ws.numel() - 1}, 'workspace'), ({'C': 2 ** 31 - 256}, 'n_comp')):
        assert meas(**over) == -1, over
        assert word in lib.hn_last_error().decode(), (over, lib.hn_last_error())
    assert meas(T=0) == 0 and meas(C=0) == 0
    keep = torch.ones(C, dtype=torch.uint8, device='cuda')
    totals = o64(2)
    cws = torch.empty(int(lib.hn_meshcc_workspace_bytes(V, T)), dtype=torch.uint8, device='cuda')

    def count(**a):
        return lib.hn_meshcc_compact_count(p(vc), a.get('V', V), a.get('fc', p(fc)), a.get('T', T), a.get('keep', p(keep)), C, a.get('totals', p(totals)),
                                           a.get('ws', p(cws)), a.get('bytes', cws.numel()), L.stream_ptr())
    for over, word in (({'fc': None}, 'NULL'), ({'keep': None}, 'NULL'), ({'totals': None}, 'NULL'), ({'ws': None}, 'NULL'), ({'V': -1}, 'n_verts'),
                       ({'T': -1}, 'n_tris'), ({'bytes': cws.numel() - 1}, 'workspace')):
        assert count(**over) == -1, over
        assert word in lib.hn_last_error().decode(), (over, lib.hn_last_error())
    vout, tout = torch.full((V, 3), -7.0, device='cuda'), o64(T, 3)
    vmap, fmap = torch.full((V,), -7, dtype=torch.int32, device='cuda'), torch.full((T,), -7, dtype=torch.int32, device='cuda')

    def emit(**a):
        return lib.hn_meshcc_compact_emit(a.get('v', p(vd)), 0, V, p(td), a.get('T', T), p(vc), p(fc), p(keep), C, a.get('ws', p(cws)),
                                          a.get('bytes', cws.numel()), a.get('Vo', V), T, a.get('vout', p(vout)), p(tout), p(vmap), a.get('fmap', p(fmap)),
                                          L.stream_ptr())
    for over, word in (({'v': None}, 'NULL'), ({'vout': None}, 'NULL'), ({'fmap': None}, 'NULL'), ({'ws': None}, 'NULL'), ({'T': -1}, 'n_tris'),
                       ({'Vo': V + 1}, 'n_verts_out'), ({'Vo': -1}, 'n_verts_out'), ({'bytes': cws.numel() - 1}, 'workspace')):
        assert emit(**over) == -1, over
        assert word in lib.hn_last_error().decode(), (over, lib.hn_last_error())
    torch.cuda.synchronize()
    for x in (faces, nv, area, vol, bounds, totals, vout, tout, vmap, fmap):
        assert bool((x == -7).all()), 'a refused / empty call wrote an output'


def test_empty_and_single(mcomp):
    for name in ('empty', 'empty_v0'):
        v, t = cc.mesh(name)
        c = mcomp.components((v, t))
        assert c['n'] == 0 and c['label'].shape == (0,) and bool((c['vertex_label'] == -1).all()) and c['vertex_component'].shape == (len(v),)
        assert c['face_label'].shape == (0,) and c['face_component'].dtype == torch.int32
        m = mcomp.measure((v, t))
        assert all(m[k].shape[0] == 0 for k in m) and m['bounds'].shape == (0, 6)
        gv, gt, info = mcomp.keep((v, t), largest=1)
        assert tuple(gv.shape) == (0, 3) and gv.dtype == torch.float32 and tuple(gt.shape) == (0, 3) and gt.dtype == torch.int64
        assert info['kept'].numel() == 0 and info['vertex_map'].shape == (len(v),) and info['face_map'].shape == (0,)
        with pytest.raises(ValueError, match='no criterion'):
            mcomp.keep((v, t))
    v, t = cc.mesh('single')
    c = mcomp.components((v, t))
    assert c['n'] == 1 and c['label'].tolist() == [0] and c['vertex_label'].tolist() == [0, -1, 0, 0] and c['face_component'].tolist() == [0]
    gv, gt, info = mcomp.keep((v, t), largest=1)
    assert _np(gv).tobytes() == v[[0, 2, 3]].tobytes() and gt.tolist() == [[2, 0, 1]] and info['vertex_map'].tolist() == [0, -1, 1, 2]


# ---- 6. what it is for -----------------------------------------------------------------------------------------------------------------------
def test_a_hand_floater_inside_the_object(mcomp):
    from honerf_amd import interaction
    hand, obj, big = cc.floater_in_object()
    assert interaction.penetration_depth(hand, obj) > 0
    before = interaction.interaction_metrics(hand, obj)
    assert before['n_hand_verts_inside'] > 0
    clean = mcomp.largest(hand)
    assert _np(clean[0]).tobytes() == big[0].tobytes() and np.array_equal(_np(clean[1]), big[1])      # the big component, bit for bit
    assert interaction.penetration_depth(clean, obj) == 0.0
    assert interaction.interaction_metrics(clean, obj)['n_hand_verts_inside'] == 0
    o = mcomp.largest(obj)
    assert _np(o[0]).tobytes() == obj[0].tobytes() and np.array_equal(_np(o[1]), obj[1])              # the object is untouched


def test_synthetic_hand_and_object(mcomp):
    from honerf_amd import synth
    from honerf_amd.interaction import hand_object_meshes
    from honerf_amd.meshcast import MeshCaster
    from honerf_amd.renderer import NeuSRenderer_fitting
    m = product_modules()
    dual = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)
    bt, tp, j = synth.synth_hand_pose(3)
    c = j[9]
    R, tr = synth.synth_obj_pose(2, center=tuple(c))
    meshes = hand_object_meshes(dual, tt(j.min(0) - 0.08), tt(j.max(0) + 0.08), tt(c - 0.35), tt(c + 0.35), 24, bt, tp, tt(R).T.contiguous(), tt(tr))
    kept = []
    for kind, (vd, td) in zip(('hand', 'obj'), meshes):
        v, t = _np(vd), _np(td)
        assert len(t) > 0
        comps = mcomp.components((vd, td))
        ref_c = cc.np_components(t, len(v))
        check_labels(comps, ref_c, 'synthetic ' + kind)
        check_measures(mcomp.measure((vd, td), comps), cc.np_measure(v, t, ref_c), 'synthetic ' + kind)
        print('synthetic %s at 24^3: %d faces in %d components' % (kind, len(t), comps['n']))
        kept.append(check_keep(mcomp, v, t, dict(largest=1), 'synthetic %s keep(largest=1)' % kind)[:2])
    caster = MeshCaster(kept)
    assert caster.n_tris == kept[0][1].shape[0] + kept[1][1].shape[0]


def test_mesh_clean_tool(tmp_path, mcomp):
    from honerf_amd import harness
    hand, obj, big = cc.floater_in_object()
    src, dst = tmp_path / 'src', tmp_path / 'dst'
    for fit, sub in (('1', 'mesh_1'), ('12', 'mesh_12')):
        p = src / fit / 'p1_box' / 'seq0' / sub
        p.mkdir(parents=True)
        harness.write_ply(str(p / '0_hand.ply'), hand[0], hand[1])
        harness.write_ply(str(p / '0_obj.ply'), obj[0], obj[1])
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'mesh_clean.py'), str(src), str(dst), '--largest', '1'], capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rel = os.path.join('1', 'p1_box', 'seq0', 'mesh_1')
    hv, ht = harness.read_ply(str(dst / rel / '0_hand.ply'))
    assert hv.tobytes() == big[0].astype(np.float32).tobytes() and np.array_equal(ht, big[1])
    ov, ot = harness.read_ply(str(dst / rel / '0_obj.ply'))
    assert ov.tobytes() == obj[0].astype(np.float32).tobytes() and np.array_equal(ot, obj[1])
    report = json.load(open(str(dst / 'mesh_clean.json')))
    assert len(report['files']) == 4
    row = report['files'][os.path.join(rel, '0_hand.ply')]
    ref = cc.np_measure(*harness.read_ply(str(src / rel / '0_hand.ply')))
    assert row['components']['faces'] == ref['faces'].tolist() and row['components']['closed'] == [True, True] and row['kept'] == [0]
    assert row['faces'] == len(hand[1]) and row['kept_faces'] == len(big[1]) and row['components']['label'] == [0, len(big[0])]
    assert report['files'][os.path.join(rel, '0_obj.ply')]['kept'] == [0]
    ev = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'interaction_eval.py'), str(dst), '--classes', 'box', '--max-frame', '2'],
                        capture_output=True, text=True, timeout=600, env=env)
    assert ev.returncode == 0, ev.stderr[-2000:]
    assert 'object class box has 1 frames' in ev.stdout and 'fit1_dep_sum: 0.00' in ev.stdout, ev.stdout
