"""GPU tests of the mesh ray caster: hn_meshcast.hip through honerf_amd.meshcast.MeshCaster and the C ABI, against the FP32 RESTATEMENT of
the intersection rule (tests/meshcast_cases.py: the cases, the rule in numpy; tests/test_meshcast_cpu.py: that restatement is the
float64 reference on every settled ray) on ALL rays, settled or not: hit, face and mesh equal, t, bary and normal within 4 ulp -- the
bound tests/test_mesh.py holds the mesher's vertices to.  0 ulp is expected: both sides make the same correctly rounded operations.
Then: cull off gives cull on's bits; ray order, chunking and a second call change nothing; NULL outputs are not written; the
refusals; empty inputs; identity and Morton order give the same bits; harness.render_mesh_buffers; the synthetic scene end to end."""

import numpy as np
import pytest
import torch

import meshcast_cases as mc
from helpers import bounded, product_modules, t as tt

pytestmark = pytest.mark.gpu
ULP = 4
KEYS = ('t', 'face', 'bary', 'normal')
_CASTERS = {}


@pytest.fixture(scope='module')
def L():
    from honerf_amd import lib
    return lib


@pytest.fixture(scope='module')
def lib(L):
    return L.load()


def caster(name, order='morton'):
    from honerf_amd.meshcast import MeshCaster
    if (name, order) not in _CASTERS:
        c = mc.case(name)
        _CASTERS[name, order] = MeshCaster(c['meshes'] if 'meshes' in c else (c['verts'], c['tris']), order=order)
    return _CASTERS[name, order]


def cast(name, order='morton', **kw):
    c = mc.case(name)
    out = caster(name, order).cast(c['o'], c['d'], c['near'], c['far'], **kw)
    torch.cuda.synchronize()
    return out


def compare(got, q, tag, offsets):
    """A cast's dict of device tensors against a restatement's dict of arrays."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g['t'].dtype == np.float32 and g['face'].dtype == np.int32 and g['mesh'].dtype == np.int32 and g['hit'].dtype == bool
    assert np.array_equal(g['hit'], q['hit']), '%s: hit differs on %d rays' % (tag, (g['hit'] != q['hit']).sum())
    assert np.array_equal(g['face'], q['face']), '%s: face differs on %d rays' % (tag, (g['face'] != q['face']).sum())
    assert np.array_equal(g['mesh'], mc.mesh_of(q['face'], offsets)), tag + ': mesh'
    for k in ('t', 'bary', 'normal'):
        assert g[k].shape == q[k].shape and np.isfinite(g[k]).all(), (tag, k)
        bounded('%s: %s against the fp32 restatement (ulp)' % (tag, k), float(mc.ulps(g[k], q[k]).max()) if g[k].size else 0.0, ULP, kind='ulp')
    miss = ~q['hit']
    assert (g['t'][miss] == 0).all() and (g['bary'][miss] == 0).all() and (g['normal'][miss] == 0).all() and (g['mesh'][miss] == -1).all()


def same_bits(a, b, tag):
    for k in a:
        assert torch.equal(a[k], b[k]), '%s: %s differs' % (tag, k)


# ---- the kernel against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mc.ALL_CASES)
def test_kernel_is_the_fp32_restatement(name):
    c = mc.case(name)
    got = cast(name)
    compare(got, mc.restatement(name), 'meshcast ' + name, c.get('offsets', [0, len(c['tris'])]))
    same_bits(got, cast(name, cull=False), 'meshcast %s: cull off against cull on' % name)


@pytest.mark.parametrize('name', ['sphere48/1', 'bad', 'two/0', 'through'])
def test_identity_and_morton_order_give_the_same_bits(name):
    a, b = caster(name, 'morton'), caster(name, 'identity')
    assert torch.equal(b.order.cpu(), torch.arange(b.n_tris, dtype=torch.int32))
    assert torch.equal(torch.sort(a.order).values.cpu(), torch.arange(a.n_tris, dtype=torch.int32)) and not torch.equal(a.order, b.order)
    same_bits(cast(name, 'morton'), cast(name, 'identity'), 'meshcast %s: identity against Morton order' % name)
    same_bits(cast(name, 'identity'), cast(name, 'identity', cull=False), 'meshcast %s identity order: cull off against cull on' % name)


def test_ray_order_chunks_and_a_second_call_change_nothing():
    c = mc.case('torus24/1')
    k = caster('torus24/1')
    o, d = torch.from_numpy(c['o']).cuda(), torch.from_numpy(c['d']).cuda()
    first = k.cast(o, d, c['near'], c['far'])
    same_bits(first, k.cast(o, d, c['near'], c['far']), 'a second call')
    perm = torch.randperm(len(o), generator=torch.Generator().manual_seed(2)).cuda()
    shuffled = k.cast(o[perm], d[perm], c['near'], c['far'])
    same_bits({n: v[perm] for n, v in first.items()}, shuffled, 'shuffled rays')
    parts = [k.cast(o[a:b], d[a:b], c['near'], c['far']) for a, b in ((0, 1), (1, 66), (66, 480))]
    same_bits(first, {n: torch.cat([p[n] for p in parts]) for n in first}, 'three chunks (1, 65 and 414 rays)')


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
class Out:
    """The four outputs, each inside a canary-filled tensor with 64 canaries in front and behind."""
    GUARD = 64
    SPEC = {'t': (1, torch.float32, 7.5), 'face': (1, torch.int32, 12345), 'bary': (2, torch.float32, 7.5), 'normal': (3, torch.float32, 7.5)}

    def __init__(self, n):
        self.flat, self.view, self.n = {}, {}, n
        for k, (w, dt, canary) in self.SPEC.items():
            self.flat[k] = torch.full((2 * self.GUARD + n * w,), canary, dtype=dt, device='cuda')
            self.view[k] = self.flat[k][self.GUARD:self.GUARD + n * w]

    def untouched(self, k):
        return bool((self.flat[k] == self.SPEC[k][2]).all())

    def guards_intact(self, k):
        g, c = self.GUARD, self.SPEC[k][2]
        return bool((self.flat[k][:g] == c).all()) and bool((self.flat[k][-g:] == c).all())

    def get(self, k):
        w = self.SPEC[k][0]
        return self.view[k].view(self.n, w) if w > 1 else self.view[k]


def _raw(L, lib, k, o, d, near, far, out, want=KEYS, cull=1, **over):
    a = {'ws': L.ptr(k._ws), 'ws_bytes': k._ws.numel(), 'T': k.n_tris, 'po': L.ptr(o), 'pd': L.ptr(d), 'N': o.shape[0]}
    a.update(over)
    p = {n: (L.ptr(out.view[n]) if n in want else None) for n in KEYS}
    return lib.hn_meshcast(a['ws'], a['ws_bytes'], a['T'], a['po'], a['pd'], a['N'], near, far, cull, p['t'], p['face'], p['bary'], p['normal'],
                           L.stream_ptr())


def test_null_outputs_are_not_written(L, lib):
    c = mc.case('sphere16/1')
    k = caster('sphere16/1')
    o, d = torch.from_numpy(c['o']).cuda(), torch.from_numpy(c['d']).cuda()
    full = k.cast(o, d, c['near'], c['far'])
    for want in [tuple(n for n in KEYS if n != drop) for drop in KEYS] + [(n,) for n in KEYS] + [()]:
        out = Out(len(o))
        assert _raw(L, lib, k, o, d, c['near'], c['far'], out, want) == 0
        torch.cuda.synchronize()
        for n in KEYS:
            if n in want:
                assert out.guards_intact(n) and torch.equal(out.get(n), full[n]), (want, n)
            else:
                assert out.untouched(n), '%s was passed as NULL and written (outputs %s)' % (n, want)


def test_refusals_and_empty_calls(L, lib):
    c = mc.case('sphere16/0')
    k = caster('sphere16/0')
    o, d = torch.from_numpy(c['o']).cuda(), torch.from_numpy(c['d']).cuda()
    out = Out(len(o))
    run = lambda **over: _raw(L, lib, k, o, d, c['near'], c['far'], out, **over)
    for over, word in (({'ws': None}, 'NULL'), ({'po': None}, 'NULL'), ({'pd': None}, 'NULL'), ({'N': -1}, 'n_rays'), ({'T': -1}, 'n_tris'),
                       ({'T': 2 ** 31 - 64}, 'n_tris'), ({'N': 2 ** 31 - 256}, 'n_rays'), ({'ws_bytes': k._ws.numel() - 1}, 'workspace'),
                       ({'T': k.n_tris + 64}, 'workspace')):
        assert run(**over) == -1, over
        assert word in lib.hn_last_error().decode(), (over, lib.hn_last_error())
    assert run(N=0) == 0 and run(T=0) == 0 and run(N=0, po=None, pd=None) == 0 and run(T=0, ws=None, ws_bytes=0) == 0
    # prepare
    v, tr = torch.from_numpy(c['verts']).cuda(), torch.from_numpy(c['tris']).cuda()
    order = torch.arange(len(tr), dtype=torch.int32, device='cuda')
    ws = torch.full((int(lib.hn_meshcast_workspace_bytes(len(tr))),), 0x5a, dtype=torch.uint8, device='cuda')
    prep = lambda **a: lib.hn_meshcast_prepare(a.get('v', L.ptr(v)), a.get('nv', len(v)), a.get('t', L.ptr(tr)), a.get('nt', len(tr)),
                                               a.get('order', L.ptr(order)), a.get('ws', L.ptr(ws)), a.get('bytes', ws.numel()), L.stream_ptr())
    for over, word in (({'v': None}, 'NULL'), ({'t': None}, 'NULL'), ({'order': None}, 'NULL'), ({'ws': None}, 'NULL'), ({'nv': -1}, 'n_verts'),
                       ({'nt': -1}, 'n_tris'), ({'nt': 2 ** 31 - 64}, 'n_tris'), ({'bytes': ws.numel() - 1}, 'workspace')):
        assert prep(**over) == -1, over
        assert word in lib.hn_last_error().decode(), (over, lib.hn_last_error())
    assert prep(nt=0) == 0 and prep(nt=0, v=None, t=None, order=None, ws=None, bytes=0) == 0
    torch.cuda.synchronize()
    assert bool((ws == 0x5a).all()), 'a refused / empty prepare wrote its workspace'
    for n in KEYS:
        assert out.untouched(n), 'a refused / empty call wrote ' + n


def test_python_refusals_and_empty_inputs():
    from honerf_amd.meshcast import MeshCaster
    v, tr = mc.mesh('sphere16')
    bad = tr.copy()
    bad[5, 1] = len(v)
    with pytest.raises(ValueError, match='triangle indices outside'):
        MeshCaster((v, bad))
    bad[5, 1] = -1
    with pytest.raises(ValueError, match='triangle indices outside'):
        MeshCaster([(v, tr), (v, bad)])
    with pytest.raises(ValueError, match='requires grad'):
        MeshCaster((torch.from_numpy(v).cuda().requires_grad_(True), tr))
    with pytest.raises(ValueError, match='CUDA tensor'):
        MeshCaster((torch.from_numpy(v), tr))
    with pytest.raises(ValueError, match='order'):
        MeshCaster((v, tr), order='bvh')
    k = caster('sphere16/0')
    c = mc.case('sphere16/0')
    with pytest.raises(ValueError, match='requires grad'):
        k.cast(torch.from_numpy(c['o']).cuda().requires_grad_(True), c['d'], 0.1, 3.0)
    with pytest.raises(ValueError, match='rays_o'):
        k.cast(c['o'][:5], c['d'], 0.1, 3.0)
    none = k.cast(c['o'][:0], c['d'][:0], 0.1, 3.0)
    assert all(none[n].shape[0] == 0 for n in none) and none['bary'].shape == (0, 2) and none['normal'].shape == (0, 3)
    empty = MeshCaster([(v, tr[:0]), (v[:0], tr[:0])])
    assert empty.n_tris == 0 and empty.face_offsets == [0, 0, 0]
    got = empty.cast(c['o'], c['d'], 0.1, 3.0)
    assert not bool(got['hit'].any()) and bool((got['face'] == -1).all()) and bool((got['mesh'] == -1).all()) and bool((got['t'] == 0).all())
    zero_d = k.cast(c['o'][:7], np.zeros((7, 3), np.float32), 0.1, 3.0)          # a ray with d = 0 never hits
    assert not bool(zero_d['hit'].any()) and bool((zero_d['t'] == 0).all())


# ---- the harness -------------------------------------------------------------------------------------------------------------------
def test_render_mesh_buffers_against_the_restatement():
    """A 24 x 20 view of the two-mesh case: depth and face as the kernel's t and face, label = 1 + mesh, and the normal's grey levels
    within one of the float64 encoding of the restatement's normal."""
    from honerf_amd import harness, synth
    H, W, near, far = 20, 24, 0.1, 3.0
    cams = synth.ring_cameras(2, radius=1.3, seed=5)
    c = mc.case('two/0')
    k = caster('two/0')
    got = harness.render_mesh_buffers(k, cams, H, W, near, far)
    assert set(got) == {'depth', 'normal', 'label', 'face'} and all(v.is_cuda for v in got.values())
    assert got['depth'].dtype == torch.float32 and tuple(got['depth'].shape) == (2, H, W)
    assert got['normal'].dtype == torch.uint8 and tuple(got['normal'].shape) == (2, H, W, 3)
    assert got['label'].dtype == torch.uint8 and tuple(got['label'].shape) == (2, H, W)
    assert got['face'].dtype == torch.int32 and tuple(got['face'].shape) == (2, H, W)
    same_bits(got, harness.render_mesh_buffers(c['meshes'], cams, H, W, near, far), 'a list of meshes against the prepared caster')
    seen = set()
    for v in range(2):
        ro, rd = harness.image_rays({n: np.asarray(a)[v:v + 1] for n, a in cams.items()}, H, W, torch.device('cuda'))
        q = mc.rule(c['verts'], c['tris'], ro.cpu().numpy(), rd.cpu().numpy(), near, far, np.float32)
        assert np.array_equal(got['face'][v].reshape(-1).cpu().numpy(), q['face']), 'view %d: face' % v
        bounded('render_mesh_buffers view %d: depth (ulp)' % v, float(mc.ulps(got['depth'][v].reshape(-1).cpu().numpy(), q['t']).max()), ULP, kind='ulp')
        label = mc.mesh_of(q['face'], c['offsets']) + 1
        assert np.array_equal(got['label'][v].reshape(-1).cpu().numpy(), label.astype(np.uint8)), 'view %d: label' % v
        seen |= set(label.tolist())
        n = q['normal'].astype(np.float64) @ np.asarray(cams['R'][v], dtype=np.float64)
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)
        level = np.floor(np.clip((n * 0.5 + 0.5) * 255.0, 0, 255)) * q['hit'][:, None]
        diff = np.abs(got['normal'][v].reshape(-1, 3).cpu().numpy().astype(np.float64) - level)
        bounded('render_mesh_buffers view %d: normal (grey levels)' % v, float(diff.max()), 1.0, kind='levels')
        assert (got['normal'][v].reshape(-1, 3).cpu().numpy()[~q['hit']] == 0).all()
    assert seen == {0, 1, 2}, seen


def test_synthetic_hand_and_object_end_to_end():
    """hand_object_meshes at 32^3 through render_mesh_buffers, 24 x 20, one camera: both labels occur, and every labelled pixel has a
    depth in [near, far], a face of its mesh and a normal."""
    from honerf_amd import harness, synth
    from honerf_amd.interaction import hand_object_meshes
    from honerf_amd.meshcast import MeshCaster
    from honerf_amd.renderer import NeuSRenderer_fitting
    m = product_modules()
    dual = NeuSRenderer_fitting(m['sdf_hand'], m['var_hand'], m['color_hand'], m['sdf_obj'], m['var_obj'], m['color_obj'], 64, 64, 0, 4, 1.0)
    bt, tp, j = synth.synth_hand_pose(3)
    c = j[9] + np.array([0.35, 0.0, 0.0], np.float32)      # (posed at joint 9 itself the object, 0.4 m across, swallows the hand)
    R, tr = synth.synth_obj_pose(2, center=tuple(c))
    hand, obj = hand_object_meshes(dual, tt(j.min(0) - 0.08), tt(j.max(0) + 0.08), tt(c - 0.35), tt(c + 0.35), 32, bt, tp, tt(R).T.contiguous(), tt(tr))
    assert hand[1].shape[0] > 0 and obj[1].shape[0] > 0
    H, W, near, far = 20, 24, 0.05, 2.5
    cams = synth.ring_cameras(1, radius=0.9, target=tuple(float(x) for x in 0.5 * (c + j[9])), seed=3)
    k = MeshCaster([hand, obj])
    got = harness.render_mesh_buffers(k, cams, H, W, near, far)
    label, depth, face = got['label'][0], got['depth'][0], got['face'][0]
    counts = [int((label == i).sum()) for i in range(3)]
    print('mesh view of the synthetic scene: %d background, %d hand, %d object pixels' % tuple(counts))
    assert counts[1] > 0 and counts[2] > 0, counts
    lit = label > 0
    assert bool(((depth[lit] >= near) & (depth[lit] <= far)).all()) and bool((depth[~lit] == 0).all())
    assert bool((face[label == 1] < k.face_offsets[1]).all()) and bool((face[label == 2] >= k.face_offsets[1]).all()) and bool((face[~lit] == -1).all())
    assert bool((got['normal'][0][lit].sum(-1) > 0).all()) and bool((got['normal'][0][~lit] == 0).all())
    field_like = harness.label_iou(got['label'], got['label'], 1)
    assert field_like.is_cuda and field_like.tolist() == [1.0]
