"""CPU checks of the mesh ray caster's contract (no GPU): the cases of tests/meshcast_cases.py are sound, the fp32 restatement of the
intersection rule is the float64 reference on every settled ray, rays through the mesh's own vertices and edges do not leak, the hit
distances are the analytic sphere's, the C ABI carries the three exports, and harness.label_iou's rules.

|t32 - t64| of the fp32 restatement on settled rays, worst over all cases with the final rule: 1.91e-6 (the grazing view of the 24^3
torus; head-on views 2.3e-7 - 3.7e-7).  T_BOUND is four times that; the margin is for the grazing rays of other seeds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import meshcast_cases as mc
from helpers import bounded, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_WORST_OBSERVED = 1.91e-6
T_BOUND = 4 * T_WORST_OBSERVED
UNSETTLED_CAP = 0.02


def test_meshes_are_the_issues():
    for name, n in mc.N_TRIS.items():
        v, t = mc.mesh(name)
        assert len(t) == n, (name, len(t))
        assert v.dtype == np.float32 and float(np.abs(v).max()) <= 0.5
    assert len(mc.mesh('sphere48')[1]) > 3 * 2048, 'the largest mesh must span more than three groups of 32 blocks of 64 triangles'


@pytest.mark.parametrize('name', mc.CAPPED)
def test_at_most_two_percent_of_a_case_is_unsettled(name):
    s = mc.reference(name)['settled']
    bounded('meshcast %s: unsettled fraction of the reference' % name, float((~s).mean()), UNSETTLED_CAP, kind='fraction')


@pytest.mark.parametrize('name', mc.CAPPED + ('n1', 'n65'))
def test_fp32_restatement_is_the_reference_on_settled_rays(name):
    r, q = mc.reference(name), mc.restatement(name)
    s = r['settled']
    assert np.array_equal(q['hit'][s], r['hit'][s]), name
    assert np.array_equal(q['face'][s], r['face'][s]), name
    both = s & r['hit']
    dt = float(np.abs(q['t'].astype(np.float64) - r['t'])[both].max()) if both.any() else 0.0
    bounded('meshcast %s: |t32 - t64| on settled rays' % name, dt, T_BOUND, kind='abs')
    if both.any():
        record('meshcast %s: |bary32 - bary64| on settled rays' % name, float(np.abs(q['bary'].astype(np.float64) - r['bary'])[both].max()), 0, kind='value')
        assert float(np.abs(q['normal'].astype(np.float64) - r['normal'])[both].max()) < 1e-5


def test_cases_reach_what_they_are_for():
    r = {n: mc.reference(n) for n in ('axis', 'inside', 'second', 'nothing', 'bad', 'two/0', 'two/1', 'sphere32/0')}
    c = mc.case('axis')
    assert ((c['d'] == 0).sum(1) == 2).all() and r['axis']['hit'].sum() >= 60 and (~r['axis']['hit']).sum() >= 6
    # (c) from inside: every ray hits, and every hit is a back face (the outward normal points along the ray)
    assert r['inside']['hit'].all()
    assert ((r['inside']['normal'] * mc.case('inside')['d'].astype(np.float64)).sum(1) > 0).all()
    # (d) near behind the first surface: the second surface answers, farther than the first and a back face; far in front: nothing
    first, second = r['sphere32/0'], r['second']
    both = first['hit'] & second['hit']
    assert both.sum() >= 100 and (second['t'][both] > first['t'][both] + 0.05).all()
    assert ((second['normal'] * mc.case('second')['d'].astype(np.float64)).sum(1)[both] > 0).all()
    assert not r['nothing']['hit'].any()
    # (e) the three unsound triangles are never hit, though they lie in front of the sphere; the sphere's faces answer as without them
    n_sound = len(mc.mesh('sphere16')[1])
    assert (r['bad']['face'] < n_sound).all()
    assert not mc.sound_triangles(*mc.with_bad_triangles(*mc.mesh('sphere16')))[n_sound:].any()
    plain = mc.reference('sphere16/0')
    assert np.array_equal(r['bad']['face'], plain['face']) and np.array_equal(r['bad']['t'], plain['t'])
    # (f) both meshes are seen, and the sphere in front of (part of) the torus
    for n in ('two/0', 'two/1'):
        m = mc.mesh_of(r[n]['face'], mc.case(n)['offsets'])
        assert (m == 0).sum() >= 40 and (m == 1).sum() >= 20 and (m == -1).sum() >= 40, (n, np.bincount(m + 1))


@pytest.mark.parametrize('f', [np.float64, np.float32])
def test_rays_through_vertices_and_edges_do_not_leak(f):
    """Set (a): a ray from an outside point through a vertex or an edge midpoint of the 16^3 sphere passes within a rounding error of
    where triangles meet.  Every such ray hits, in both precisions, except possibly where the surface FOLDS as seen from that point (the
    faces around the target face the ray both ways: meshcast_cases.horizon_targets): there the projected faces overlap instead of
    surrounding the target, and a ray an ulp outside the mesh's outline misses every closed mesh under every rule.  The 16^3 sphere
    has 75 such targets among 1 434 from this point (49 of their rays miss in float64, 44 in fp32); all 1 359 others must hit."""
    c = mc.case('through')
    r = mc.rule(c['verts'], c['tris'], c['o'], c['d'], c['near'], c['far'], f)
    fold = mc.horizon_targets(c['verts'], c['tris'])
    assert len(c['o']) == len(c['verts']) + len(mc.edges_of(c['tris'])) == len(fold)
    assert fold.sum() <= 0.06 * len(fold), fold.sum()
    leaks = ~r['hit'] & ~fold
    assert not leaks.any(), '%d rays leak between triangles: %s' % (leaks.sum(), np.nonzero(leaks)[0][:10])
    # a ray that hits, hits no later than its target (the front surface, or the target itself on the far side), a cell's slack for folds
    tgt_t = np.linalg.norm(np.concatenate([c['verts'], 0.5 * (c['verts'][mc.edges_of(c['tris'])].sum(1))]).astype(np.float64)
                           - np.asarray(mc.OUTSIDE)[None, :], axis=1)
    assert (r['t'][r['hit']] <= tgt_t[r['hit']] + mc.cell('sphere16')).all()
    record('meshcast through: rays that miss at a fold (%s)' % np.dtype(f).name, float((~r['hit']).sum()), float(fold.sum()), kind='count')


def _sphere_t(o, d, far_root):
    o, d = o.astype(np.float64), d.astype(np.float64)
    b = (o * d).sum(1)
    disc = b * b - ((o * o).sum(1) - mc.SPHERE_R ** 2)
    root = np.sqrt(np.maximum(disc, 0.0))
    return np.where(disc > 0, -b + root if far_root else -b - root, np.nan)


@pytest.mark.parametrize('name', [n for n in mc.GRID_CASES if n.startswith('sphere')] + ['inside'])
def test_settled_sphere_hits_are_within_a_cell_of_the_analytic_sphere(name):
    c, r = mc.case(name), mc.reference(name)
    ts = _sphere_t(c['o'], c['d'], far_root=name == 'inside')
    use = r['settled'] & r['hit'] & np.isfinite(ts)
    assert use.sum() >= 150
    h = mc.cell('sphere16' if name == 'inside' else name.split('/')[0])
    bounded('meshcast %s: |t - analytic sphere| in grid cells' % name, float(np.abs(r['t'] - ts)[use].max() / h), 1.0, kind='cells')


def test_header_and_library_carry_the_caster():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'honerf.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(hn_meshcast[a-z0-9_]*)\s*\(', src))
    assert names == {'hn_meshcast_workspace_bytes', 'hn_meshcast_prepare', 'hn_meshcast'}, names
    from honerf_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(cdll, n), n
        assert n in lib.SIGNATURES, n
    L = lib.load()
    assert L.hn_meshcast_workspace_bytes(0) > 0
    one, two = L.hn_meshcast_workspace_bytes(64), L.hn_meshcast_workspace_bytes(65)
    assert one >= 64 * 48 + 2 * 32 and two >= one + 64 * 48
    assert L.hn_meshcast_workspace_bytes(-1) == 0 and L.hn_meshcast_workspace_bytes(2 ** 31 - 64) == 0
    assert L.hn_meshcast_workspace_bytes(2 ** 31 - 65) > 48 * (2 ** 31 - 65)
    assert b'n_tris' in L.hn_last_error()


def test_label_iou_rules():
    from honerf_amd import harness
    a = np.zeros((3, 4, 5), np.uint8)
    b = np.zeros((3, 4, 5), np.uint8)
    a[0, :2] = 1                      # view 0: 10 pixels against 15, 10 shared
    b[0, :3] = 1
    a[1, 0, :2] = 2                   # view 1: label 1 nowhere, label 2 disjoint
    b[1, 3, :2] = 2
    a[2], b[2] = 1, 1                 # view 2: identical
    for mk in (lambda x: x, torch.from_numpy):
        got = harness.label_iou(mk(a), mk(b), 1)
        assert got.dtype == torch.float64 and tuple(got.shape) == (3,)
        assert got.tolist() == [10 / 15, 1.0, 1.0]
        assert harness.label_iou(mk(a), mk(b), 2).tolist() == [1.0, 0.0, 1.0]
    assert harness.label_iou(a[0], b[0], 1).tolist() == [10 / 15]
    with pytest.raises(ValueError, match='label_iou'):
        harness.label_iou(a, b[:2], 1)
