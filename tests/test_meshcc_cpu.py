"""CPU checks of the mesh components contract (no GPU): the numpy restatement of tests/meshcc_cases.py agrees with a breadth-first
search on every case, labels are the smallest index of their component, the component tables of the cases are what the cases were
chosen for, the three blobs measure as their spheres within the mesher's own discretisation error, the C ABI carries the six exports,
and tools/mesh_clean.py parses its arguments without a device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import meshcc_cases as cc
from test_mesh_cpu import area_volume, np_marching_cubes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'hn_meshcc_workspace_bytes': 2, 'hn_meshcc_measure_workspace_bytes': 2, 'hn_meshcc_label': 12, 'hn_meshcc_measure': 17,
           'hn_meshcc_compact_count': 10, 'hn_meshcc_compact_emit': 18}


@pytest.mark.parametrize('name', cc.NAMES)
def test_restatement_agrees_with_a_breadth_first_search(name):
    v, t = cc.mesh(name)
    c = cc.comps(name)
    assert np.array_equal(c['vertex_label'], cc.bfs_labels(t, len(v))), name
    for k in ('label', 'vertex_label', 'vertex_component', 'face_label', 'face_component'):
        assert c[k].dtype == np.int32, (name, k)
    # the label is the smallest index of the component; -1 sits exactly on the unreferenced vertices
    used = np.zeros(len(v), bool)
    used[t.reshape(-1)] = True
    assert np.array_equal(c['vertex_label'] >= 0, used), name
    for i, lab in enumerate(c['label'].tolist()):
        members = np.nonzero(c['vertex_component'] == i)[0]
        assert members.min() == lab and (c['vertex_label'][members] == lab).all(), (name, i)
    assert (np.diff(c['label']) > 0).all() and c['n'] == len(c['label'])
    if len(t):
        assert np.array_equal(c['face_label'], c['vertex_label'][t[:, 0]]) and np.array_equal(c['face_label'], c['vertex_label'][t[:, 2]])


def test_an_out_of_range_triangle_joins_nothing():
    v, t = cc.mesh('soup257')
    bad = np.concatenate([t, [[t[3, 0], t[8, 1], len(v)], [-1, t[4, 0], t[6, 0]]]])
    a, b = cc.np_components(t, len(v)), cc.np_components(bad, len(v))
    assert np.array_equal(a['vertex_label'], b['vertex_label']) and a['n'] == b['n']
    assert np.array_equal(b['face_label'][:-2], a['face_label']) and (b['face_label'][-2:] == -1).all() and (b['face_component'][-2:] == -1).all()


def test_component_tables():
    m = cc.measures('blobs24')
    v, t = cc.mesh('blobs24')
    assert (len(v), len(t), cc.comps('blobs24')['n']) == (640, 1268, 3)
    assert sorted(m['faces'].tolist(), reverse=True) == [796, 428, 44] and m['closed'].all()
    v, t = cc.mesh('noise')
    m = cc.measures('noise')
    assert (len(v), len(t), len(m['faces'])) == (10563, 20365, 85)
    assert m['faces'].max() == 19716 and np.sort(m['faces'])[-2] == 48 and m['faces'].min() == 1 and (~m['closed']).sum() == 41 and not m['closed'][0]
    for name in ('sphere20', 'torus24', 'strip', 'fan_high', 'fan_low', 'pinch', 'single'):
        assert cc.comps(name)['n'] == 1, name
    assert cc.measures('sphere20')['closed'].all() and cc.measures('torus24')['closed'].all()
    assert not cc.measures('strip')['closed'].any() and not cc.measures('fan_high')['closed'].any() and not cc.measures('single')['closed'].any()
    assert cc.comps('fan_high')['label'].tolist() == [0] and cc.comps('strip')['label'].tolist() == [0]
    for n in (255, 256, 257):
        c = cc.comps('soup%d' % n)
        assert c['n'] == n and np.array_equal(c['label'], 3 * np.arange(n))
    g = cc.comps('soup_gaps')
    assert g['n'] == 257 and (g['vertex_label'] == -1).sum() == 5
    e = cc.comps('soup_extras')
    assert e['n'] == 256 and len(cc.mesh('soup_extras')[1]) == 259          # the degenerate face joins two triangles, the duplicate none
    assert cc.comps('empty')['n'] == 0 and (cc.comps('empty')['vertex_label'] == -1).all() and cc.comps('empty_v0')['n'] == 0
    f = cc.measures('floater')
    assert len(f['faces']) == 2 and f['closed'].all() and f['faces'][0] > 4 * f['faces'][1]


def test_pinch_is_one_component_and_two_closed_fans():
    v, t = cc.mesh('pinch')
    assert cc.comps('pinch')['n'] == 1
    assert cc.np_is_closed(t[:4]) and cc.np_is_closed(t[4:]) and cc.np_is_closed(t)     # no shared edge: every edge still has its reverse


def test_torus_volume_and_genus():
    v, t = cc.mesh('torus24')
    m = cc.measures('torus24')
    h = 1.0 / 23
    exact = 2 * np.pi ** 2 * 0.3 * 0.1 ** 2
    assert m['closed'][0] and abs(m['volume'][0] * h ** 3 / exact - 1) < 0.1
    E = len(np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0))
    assert len(v) - E + len(t) == 0                                         # genus 1


def test_blobs_measure_as_their_spheres_within_the_meshers_error():
    """Each blob's component against 4 pi r^2 and 4/3 pi r^3.  The allowed error is the mesher's own: what test_mesh_cpu.area_volume
    gives for the marching-cubes mesh of that sphere ALONE on the same grid (away from the others min() changes nothing near its
    surface), against the same formulas -- measured per blob, not a constant."""
    v, t = cc.mesh('blobs24')
    w = cc.blob_world(v)
    c = cc.comps('blobs24')
    m = cc.np_measure(w, t, c)
    assert (m['volume'] > 0).all()
    centres = np.stack([w[c['vertex_component'] == i].mean(0) for i in range(3)])
    for cx, cy, cz, r in cc.BLOBS:
        i = int(np.argmin(np.linalg.norm(centres - np.array([cx, cy, cz]), axis=1)))
        sv, st = np_marching_cubes(cc.blob_volume(((cx, cy, cz, r),)))
        area1, vol1 = area_volume(cc.blob_world(sv), st)
        fa, fv = 4 * np.pi * r * r, 4 / 3 * np.pi * r ** 3
        assert m['faces'][i] == len(st)
        assert abs(m['area'][i] - fa) <= abs(area1 - fa) + 1e-12 * fa, (r, m['area'][i], area1, fa)
        assert abs(m['volume'][i] - fv) <= abs(vol1 - fv) + 1e-12 * fv, (r, m['volume'][i], vol1, fv)


def test_keep_restatement_is_stable():
    v, t = cc.mesh('noise')
    c, m = cc.comps('noise'), cc.measures('noise')
    sel = cc.np_select(m, largest=2)
    assert sel.sum() == 2 and sel[np.argmax(m['faces'])]
    kv, kt, vmap, fmap, kept = cc.np_keep(v, t, sel, c)
    assert np.array_equal(kv, v[vmap >= 0]) and (np.diff(vmap[vmap >= 0]) == 1).all() and (np.diff(fmap[fmap >= 0]) == 1).all()
    assert np.array_equal(kv[kt], v[t[fmap >= 0]]) and cc.np_components(kt, len(kv))['n'] == 2
    assert (cc.np_components(kt, len(kv))['vertex_label'] >= 0).all()
    ties = cc.np_select(cc.measures('soup257'), largest=3)
    assert np.nonzero(ties)[0].tolist() == [0, 1, 2]                      # equal face counts: the smaller labels


def test_header_and_library_carry_the_components():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'honerf.h')).read(), flags=re.S)
    decl = dict(re.findall(r'\b(hn_meshcc[a-z0-9_]*)\s*\(([^)]*)\)', src))
    assert set(decl) == set(EXPORTS), set(decl)
    from honerf_amd import lib
    assert re.search(r'#define\s+HN_VERSION\s+121\b', src) and lib.HN_VERSION == 121
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for n, args in decl.items():
        assert hasattr(cdll, n), n
        assert n in lib.SIGNATURES, n
        assert len(lib.SIGNATURES[n][1]) == len(args.split(',')) == EXPORTS[n], n
    L = lib.load()
    assert L.hn_version() == 121
    assert L.hn_meshcc_workspace_bytes(0, 0) > 0 and L.hn_meshcc_measure_workspace_bytes(0, 0) > 0
    assert L.hn_meshcc_workspace_bytes(1000, 2000) >= 3 * 4 * 1000
    assert L.hn_meshcc_workspace_bytes(-1, 5) == 0 and b'n_verts' in L.hn_last_error()
    assert L.hn_meshcc_workspace_bytes(5, 2 ** 31 - 256) == 0 and b'n_tris' in L.hn_last_error()
    assert L.hn_meshcc_workspace_bytes(2 ** 31 - 257, 2 ** 31 - 257) > 12 * (2 ** 31 - 257)
    assert L.hn_meshcc_measure_workspace_bytes(5, -1) == 0 and b'n_comp' in L.hn_last_error()
    assert L.hn_meshcc_measure_workspace_bytes(256 * 100, 7) >= 64 * 107


def test_mesh_clean_help_parses_without_a_device():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'mesh_clean.py'), '--help'], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='-1'))
    assert out.returncode == 0, out.stderr[-2000:]
    for word in ('--largest', '--min-faces', '--min-area-fraction', '--closed-only'):
        assert word in out.stdout, word
