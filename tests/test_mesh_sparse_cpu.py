"""CPU checks of the narrow-band mesher (hn_mcubes_sparse.hip, honerf_amd.mesh.marching_cubes_sparse): the numpy restatement of
tests/mesh_sparse_cases.py against the dense restatement of tests/test_mesh_cpu.py on every case the GPU tests run, what the
classification promises for exact distance fields, growth on a field steeper than assumed, the size of the band, and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_sparse_cases as C
from test_mesh_cpu import np_marching_cubes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.cases()


@pytest.fixture(scope='module')
def dense():
    return {k: np_marching_cubes(vol, thr) for k, (vol, thr, _) in CASES.items()}


@pytest.mark.parametrize('b', C.BLOCKS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_band_mesh_is_the_dense_mesh(name, b, dense):
    vol, thr, reach = CASES[name]
    v, t, info = C.np_marching_cubes_sparse(vol, thr, b, reach[b])
    rv, rt = dense[name]
    assert len(rv) > 0 and info['leaks_left'] == 0
    assert v.dtype == np.float32 and v.tobytes() == rv.tobytes(), name
    assert np.array_equal(t, rt), name
    assert info['active_initial'] <= info['active'] <= info['blocks']
    if name.startswith('noise'):
        assert info['active'] == info['blocks']             # every block carries a piece of the surface


@pytest.mark.parametrize('b', C.BLOCKS)
@pytest.mark.parametrize('name', [k for k in sorted(CASES) if k.split()[0] in ('sphere', 'torus', 'two')])
def test_exact_distance_fields_need_no_growth(name, b):
    """|grad| = 1 and reach = half a block diagonal: the classification alone holds every block with a crossing edge."""
    vol, thr, reach = CASES[name]
    active, info = C.band(vol, thr, b, reach[b])
    assert info['grow_rounds'] == 0 and info['leaks_left'] == 0 and info['active'] == info['active_initial']
    inside = vol < np.float32(thr)
    nb = C.n_blocks(vol.shape, b)
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        g = np.stack(np.nonzero(inside[tuple(lo)] != inside[tuple(hi)]), -1)
        c = np.minimum(g // b, np.array(nb)[None, :] - 1)
        assert active[c[:, 0], c[:, 1], c[:, 2]].all(), (name, a)


def test_small_sphere_is_smaller_than_a_block():
    vol = C.two_spheres_volume(64)
    small = vol[44:62, 4:20, 36:52] < 0
    assert 0 < small.sum() < 4 ** 3 and not (vol[44, 4:20, 36:52] < 0).any()


def test_steep_field_needs_growth():
    """5 (|p| - r) meshed with the reach of lipschitz = 1: the classification misses blocks that carry triangles, growth finds
    them, and without growth the leak search reports them."""
    b = C.STEEP['block']
    vol = C.steep_volume(C.STEEP['res'], C.STEEP['r'])
    reach = C.unit_reach(vol.shape, b)
    rv, rt = np_marching_cubes(vol, 0.0)
    first, _ = C.band(vol, 0.0, b, reach, grow=False)
    cells = np.stack(np.unravel_index(C.mesh_keys(vol, 0.0)[1] // 8, vol.shape), -1) // b
    assert not first[cells[:, 0], cells[:, 1], cells[:, 2]].all()                  # a block with triangles is not in the first band
    v, t, info = C.np_marching_cubes_sparse(vol, 0.0, b, reach)
    assert info['grow_rounds'] >= 1 and info['leaks_left'] == 0 and info['active'] > info['active_initial']
    assert v.tobytes() == rv.tobytes() and np.array_equal(t, rt)
    v0, t0, info0 = C.np_marching_cubes_sparse(vol, 0.0, b, reach, grow=False)
    assert info0['leaks_left'] > 0 and info0['grow_rounds'] == 0 and info0['active'] == info0['active_initial']
    assert len(t0) < len(rt)
    v1, t1, info1 = C.np_marching_cubes_sparse(vol, 0.0, b, reach, max_grow=0)
    assert info1['leaks_left'] == info0['leaks_left'] and len(t1) == len(t0)


def test_band_size_bound_at_512():
    """Sphere r = 0.3 in the unit box at 512^3, b = 8, lipschitz = 1, classification only, on the 65^3 lattice of the analytic
    function.  The band lies within (6.9 + 13.9) voxels of a surface of radius 153 voxels: about 9 % of the points, times (9 / 8)^3
    for the aprons.  The cap of a quarter of the grid catches a band that silently degenerates to everything."""
    res, b = 512, 8
    ax = np.linspace(-0.5, 0.5, res, dtype=np.float32)
    lx = ax[C.lattice_axes((res,) * 3, b)[0]]
    assert len(lx) == 65
    x, y, z = np.meshgrid(lx, lx, lx, indexing='ij')
    lat = (np.sqrt(x * x + y * y + z * z) - np.float32(0.3)).astype(np.float32)
    active = C.classify(lat, 0.0, C.unit_reach((res,) * 3, b))
    assert active.shape == (64, 64, 64)
    assert 0 < int(active.sum()) * (b + 1) ** 3 <= 0.25 * res ** 3


def test_header_and_library_carry_the_sparse_mesher():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'honerf.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(hn_mcs_[a-z0-9_]*)\s*\(', src))
    assert names == {'hn_mcs_workspace_bytes', 'hn_mcs_lattice', 'hn_mcs_classify', 'hn_mcs_compact', 'hn_mcs_brick_points',
                     'hn_mcs_leaks', 'hn_mcs_count', 'hn_mcs_emit'}, names
    from honerf_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(cdll, n), n
        assert n in lib.SIGNATURES, n
    L = lib.load()
    assert L.hn_mcs_workspace_bytes(64, 64, 64, 8, 0) > 0
    assert L.hn_mcs_workspace_bytes(64, 64, 64, 8, 512) > 512 * 729 * 5
    assert L.hn_mcs_workspace_bytes(64, 64, 64, 8, 513) == 0        # more bricks than blocks
    assert L.hn_mcs_workspace_bytes(64, 64, 64, 5, 0) == 0          # block edges of 4 and 8 only
    assert L.hn_mcs_workspace_bytes(1, 64, 64, 8, 0) == 0
    assert L.hn_mcs_workspace_bytes(2049, 64, 64, 8, 0) == 0
    assert L.hn_mcs_workspace_bytes(1024, 1024, 1024, 8, 0) > 0     # beyond the dense mesher's limit
    assert L.hn_mcubes_workspace_bytes(1024, 1024, 1024) == 0


def test_the_two_meshers_share_one_case_table():
    csrc = os.path.join(ROOT, 'ho-nerf_amd', 'csrc')
    for f in ('hn_mcubes.hip', 'hn_mcubes_sparse.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "hn_mc_tables.h"' in text and 'c_tri_table[256]' not in text, f
    assert 'c_tri_table[256][16]' in open(os.path.join(csrc, 'hn_mc_tables.h')).read()
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert 'hn_mcubes_sparse.hip' in mk and 'FLAGS_hn_mcubes_sparse := -ffp-contract=off' in mk


def test_mesher_argument_is_checked_without_a_device():
    import inspect
    from honerf_amd.mesh import marching_cubes_sparse
    from honerf_amd.renderer import NeuSRenderer, NeuSRenderer_fitting
    p = inspect.signature(marching_cubes_sparse).parameters
    assert [k for k in p][:3] == ['values_at', 'dims', 'threshold'] and p['reach'].default is inspect.Parameter.empty
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('block', 'reach', 'grow', 'max_grow', 'chunk'))
    for cls in (NeuSRenderer, NeuSRenderer_fitting):
        q = inspect.signature(cls.extract_geometry).parameters
        assert (q['mesher'].default, q['block'].default, q['lipschitz'].default, q['grow'].default, q['return_info'].default) \
            == (None, 8, 1.0, True, False)
        assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('mesher', 'block', 'lipschitz', 'grow', 'return_info'))
