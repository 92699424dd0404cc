"""Hand-object interaction metrics on the device (hn_interact.hip): analys_results/analys_interaction.py without trimesh.

The reference scores a fitted frame by two numbers on the meshes get_res.py exports (`get_int_vol`, analys_interaction.py:21-42):
  int_vol  the object mesh voxelized at a 5 mm pitch (`Trimesh.voxelized`), its voxel points inside the hand mesh
           (`Trimesh.contains`) counted, times pitch^3, x 1e6: cm^3;
  pen_dep  the largest distance from a hand vertex inside the object mesh to the object's surface (`trimesh.proximity.closest_point`),
           x 1000: mm; 0 when no hand vertex is inside.
DESIGN.md 3.14 restates what trimesh computes for those calls, and that restatement is the contract:
  voxelize_surface  every triangle split 4-way at its edge midpoints until no edge is longer than pitch / 2 (at most 10 rounds),
                    every leaf vertex snapped to rint(v / pitch), duplicates dropped.  A HOLLOW SHELL: the surface's voxels, no
                    interior, so int_vol measures the object's surface layer inside the hand, not the shared volume (the
                    reference's quirk, kept; `intersection_volume(..., solid=True)` is the volume estimate);
  contains          |generalized winding number| > 1/2, and outside the mesh's bounds without evaluation;
  closest_distance  the exact unsigned distance to the nearest triangle.

Meshes are (vertices [V, 3], triangles [T, 3]) and points [P, 3]: numpy arrays or CUDA tensors (a CPU tensor is refused), float32
or float64.  They are moved to the current CUDA device and results stay there, except scalars.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib

KEY_BIAS = 1 << 20
_KEY_MASK = (1 << 21) - 1


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _tensor(x, what, dtypes=(torch.float32, torch.float64)):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x)).to(_device())
    if not isinstance(x, torch.Tensor):
        raise ValueError('%s: expected a numpy array or a torch tensor, got %s' % (what, type(x).__name__))
    if not x.is_cuda:
        raise ValueError('%s: a %s tensor; pass a CUDA tensor or a numpy array' % (what, x.device.type))
    if x.dtype not in dtypes:
        raise ValueError('%s: dtype %s, expected one of %s' % (what, x.dtype, ', '.join(str(d) for d in dtypes)))
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError('%s: shape %s, expected [N, 3]' % (what, tuple(x.shape)))
    return x.detach().to(_device())


class _Mesh:
    """A checked mesh on the device: vertices [V, 3] (its own float dtype), triangles int64 [T, 3].  The fp32 vertices, the fp32 and
    fp64 rows of 9 coordinates per triangle and the fp32 bounds are built once, on first use."""

    def __init__(self, v, t):
        self.v, self.t = v, t
        self._cache = {}

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    @property
    def v32(self):
        return self._get('v32', lambda: self.v.to(torch.float32).contiguous())

    def rows(self, dtype):
        src = self.v32 if dtype == torch.float32 else self.v.to(dtype)
        return self._get(('rows', dtype), lambda: src[self.t].reshape(-1, 9).contiguous())

    @property
    def bbox(self):
        return self._get('bbox', lambda: torch.cat([self.v32.amin(0), self.v32.amax(0)]).contiguous())


def _meshes(*named):
    """(mesh, name) pairs -> checked _Mesh objects.  The index ranges of all of them are read back together (one host sync)."""
    out, lims = [], []
    for mesh, what in named:
        if not isinstance(mesh, (tuple, list)) or len(mesh) != 2:
            raise ValueError('%s: expected (vertices [V, 3], triangles [T, 3])' % what)
        v = _tensor(mesh[0], what + ' vertices')
        t = _tensor(mesh[1], what + ' triangles', (torch.int32, torch.int64)).long().contiguous()
        out.append(_Mesh(v, t))
        if t.numel():
            lims.append((what, v.shape[0], torch.stack([t.min(), t.max()])))
    if lims:
        vals = torch.stack([x[2] for x in lims]).tolist()
        for (what, nv, _), (lo, hi) in zip(lims, vals):
            if lo < 0 or hi >= nv:
                raise ValueError('%s: triangle indices outside [0, %d)' % (what, nv))
    return out


def _points(points, what):
    return _tensor(points, what + ' points').to(torch.float32).contiguous()


def _check(rc, what):
    if rc == -1:                     # HN_EINVAL: a refused argument, with the library's message
        msg = _lib.load().hn_last_error()
        raise ValueError('%s: %s' % (what, msg.decode() if msg else 'invalid argument'))
    _lib.check(rc, what)


# ---- public queries: each checks its arguments once and hands checked tensors to the private passes below -------------------------
def voxelize_surface(mesh, pitch):
    """Trimesh.voxelized(pitch).points -> float64 [N, 3] on the device, sorted by key (x, then y, then z).  Raises ValueError when
    a triangle would need more than 10 rounds of splitting (edge / pitch about 1000 and more) or lies 2^20 pitches from the origin."""
    m, = _meshes((mesh, 'mesh'))
    return _voxelize(m, _pitch(pitch))


def contains(mesh, points):
    """Trimesh.contains(points) as |generalized winding number| > 1/2 -> bool [P] on the device."""
    m, = _meshes((mesh, 'contains mesh'))
    return _winding(m, _points(points, 'contains'))[0]


def winding_number(mesh, points):
    """The generalized winding number itself -> float32 [P] on the device (0 outside the mesh's bounds)."""
    m, = _meshes((mesh, 'winding_number mesh'))
    return _winding(m, _points(points, 'winding_number'), want_w=True)[1]


def closest_distance(mesh, points, culled=False):
    """trimesh.proximity.closest_point's distance: the unsigned distance to the nearest triangle -> float32 [P] on the device
    (inf for a mesh without triangles).  culled=True asks `mesh_distance.MeshIndex` (the same arithmetic per pair behind two levels of
    bounding boxes) instead of the brute force: the same bits."""
    m, = _meshes((mesh, 'closest_distance mesh'))
    return _distance(m, _points(points, 'closest_distance'), culled)


def solid_lattice(obj_mesh, hand_mesh, pitch):
    """The lattice points k * pitch (float64 [N, 3], device) in the overlap of the two meshes' bounds: what solid=True counts."""
    obj, hand = _meshes((obj_mesh, 'obj_mesh'), (hand_mesh, 'hand_mesh'))
    return _solid_lattice(obj, hand, _pitch(pitch))


def intersection_volume(obj_mesh, hand_mesh, pitch=0.005, solid=False):
    """intersect_vox (analys_interaction.py:14-19) -> m^3.  solid=False: the reference's number, the object's surface voxels inside
    the hand times pitch^3 (a hollow shell: not a volume).  solid=True: the lattice points k * pitch inside BOTH meshes times
    pitch^3, a true estimate of the shared volume that converges as the pitch shrinks; NOT the reference's number."""
    obj, hand = _meshes((obj_mesh, 'obj_mesh'), (hand_mesh, 'hand_mesh'))
    pitch = _pitch(pitch)
    if solid:
        pts = _solid_lattice(obj, hand, pitch)
        in_hand = _winding(hand, pts.to(torch.float32).contiguous())[0]
        n = int(_winding(obj, pts[in_hand].to(torch.float32).contiguous())[0].sum())
    else:
        n = int(_winding(hand, _voxelize(obj, pitch).to(torch.float32).contiguous())[0].sum())
    return n * pitch ** 3


def penetration_depth(hand_mesh, obj_mesh, culled=False):
    """get_pen_depth (analys_interaction.py:44-55) -> m: the largest distance from a hand vertex inside the object mesh to the
    object's surface; 0.0 when no hand vertex is inside.  culled: as in closest_distance."""
    hand, obj = _meshes((hand_mesh, 'hand_mesh'), (obj_mesh, 'obj_mesh'))
    return float(_penetration(hand, obj, culled)[0])


def is_closed(triangles):
    """Edge-manifold and consistently oriented: every directed edge (a, b) is used by exactly one face and its reverse (b, a) by
    exactly one other.  A mesh cut by the box of its grid is open.  triangles [T, 3] (numpy or torch, any device)."""
    t = torch.as_tensor(triangles).long().reshape(-1, 3)
    return bool(_closed(t, int(t.max()) + 1 if t.numel() else 0))


def interaction_metrics(hand_mesh, obj_mesh, pitch=0.005, culled=False):
    """get_int_vol (analys_interaction.py:21-42) on device meshes -> dict: int_vol (cm^3) and pen_dep (mm), the keys and units of the
    reference's pickle; n_obj_voxels, n_obj_voxels_inside, n_hand_verts_inside; hand_closed / obj_closed (is_closed: the metrics are
    computed on an open mesh too, but containment there is not a closed surface's).  Host syncs: the index check of both meshes,
    the key total and torch.unique of the voxelizer, the selection of the inner hand vertices, and the final read-back.  culled: the
    penetration depth's distances as in closest_distance (the same bits)."""
    hand, obj = _meshes((hand_mesh, 'hand_mesh'), (obj_mesh, 'obj_mesh'))
    pitch = _pitch(pitch)
    vox = _voxelize(obj, pitch)
    n_in = _winding(hand, vox.to(torch.float32).contiguous())[0].sum()
    pen, n_hand = _penetration(hand, obj, culled)
    closed = torch.stack([_closed(hand.t, hand.v.shape[0]), _closed(obj.t, obj.v.shape[0])])
    n_in, n_hand, pen, hc, oc = torch.stack([n_in.double(), n_hand.double(), pen.double(), closed[0].double(), closed[1].double()]).tolist()
    n_in, n_hand = int(n_in), int(n_hand)
    return dict(int_vol=n_in * pitch ** 3 * 1e6, pen_dep=pen * 1000.0, n_obj_voxels=vox.shape[0], n_obj_voxels_inside=n_in,
                n_hand_verts_inside=n_hand, hand_closed=hc == 1.0, obj_closed=oc == 1.0)


# ---- private passes on checked meshes ------------------------------------------------------------------------------------------
def _pitch(pitch):
    pitch = float(pitch)
    if not pitch > 0.0 or not np.isfinite(pitch):
        raise ValueError('pitch must be positive and finite, got %r' % pitch)
    return pitch


def _voxelize(m, pitch):
    dev = m.v.device
    T = m.t.shape[0]
    if T == 0:
        return torch.zeros(0, 3, dtype=torch.float64, device=dev)
    L = _lib.load()
    rows = m.rows(torch.float64)
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(L.hn_voxelize_workspace_bytes(T)), 256), dtype=torch.uint8, device=dev)
        n = ctypes.c_longlong(0)
        _check(L.hn_voxelize_count(_lib.ptr(rows), T, pitch, ctypes.byref(n), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'voxelize_surface')
        keys = torch.empty(int(n.value), dtype=torch.int64, device=dev)
        _check(L.hn_voxelize_emit(_lib.ptr(rows), T, pitch, _lib.ptr(ws), ws.numel(), keys.numel(), _lib.ptr(keys), _lib.stream_ptr()),
               'voxelize_surface')
    k = torch.unique(keys)           # sorted, duplicates dropped (plumbing: the keys are plain int64)
    ijk = torch.stack([(k >> 42) & _KEY_MASK, (k >> 21) & _KEY_MASK, k & _KEY_MASK], 1) - KEY_BIAS
    return ijk.to(torch.float64) * pitch


def _winding(m, p, want_w=False):
    """p: fp32 [P, 3] contiguous on the device -> (inside bool [P], w fp32 [P] or None)."""
    P, T = p.shape[0], m.t.shape[0]
    dev = p.device
    if P == 0 or T == 0:
        return torch.zeros(P, dtype=torch.bool, device=dev), torch.zeros(P, dtype=torch.float32, device=dev) if want_w else None
    L = _lib.load()
    rows = m.rows(torch.float32)
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(L.hn_interact_workspace_bytes(P, T)), 256), dtype=torch.uint8, device=dev)
        inside = torch.empty(P, dtype=torch.uint8, device=dev)
        w = torch.empty(P, dtype=torch.float32, device=dev) if want_w else None
        _check(L.hn_winding_contains(_lib.ptr(p), P, _lib.ptr(rows), T, _lib.ptr(m.bbox), _lib.ptr(inside), _lib.ptr(w), _lib.ptr(ws),
                                     ws.numel(), _lib.stream_ptr()), 'contains')
    return inside.bool(), w


def _distance(m, p, culled=False):
    P, T = p.shape[0], m.t.shape[0]
    dev = p.device
    if P == 0 or T == 0:
        return torch.full((P,), float('inf'), dtype=torch.float32, device=dev)
    if culled:
        from .mesh_distance import MeshIndex
        return MeshIndex(m).closest(p, want=('dist',))['dist']
    L = _lib.load()
    rows = m.rows(torch.float32)
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(L.hn_interact_workspace_bytes(P, T)), 256), dtype=torch.uint8, device=dev)
        d = torch.empty(P, dtype=torch.float32, device=dev)
        _check(L.hn_closest_distance(_lib.ptr(p), P, _lib.ptr(rows), T, _lib.ptr(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               'closest_distance')
    return d


def _penetration(hand, obj, culled=False):
    """-> (largest distance of an inner hand vertex, count of inner hand vertices), both device scalars (one host sync: the
    selection of the inner vertices)."""
    inside = _winding(obj, hand.v32)[0]
    inner = hand.v32[inside]
    if inner.shape[0] == 0:
        z = torch.zeros((), dtype=torch.float32, device=hand.v.device)
        return z, z
    return _distance(obj, inner, culled).max(), inside.sum()


def _closed(t, n_verts):
    """is_closed as a device bool scalar, without a host sync: the directed edge codes sorted, no code twice, every reverse found."""
    if t.shape[0] == 0:
        return torch.zeros((), dtype=torch.bool, device=t.device)
    d = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    code = d[:, 0] * n_verts + d[:, 1]
    rev = d[:, 1] * n_verts + d[:, 0]
    s = torch.sort(code).values
    once = ~(s[1:] == s[:-1]).any()
    pos = torch.searchsorted(s, rev).clamp(max=s.shape[0] - 1)
    return once & (s[pos] == rev).all()


def _solid_lattice(obj, hand, pitch):
    dev = obj.v.device
    if obj.v.shape[0] == 0 or hand.v.shape[0] == 0:
        return torch.zeros(0, 3, dtype=torch.float64, device=dev)
    lo = torch.maximum(obj.v.double().amin(0), hand.v.double().amin(0))
    hi = torch.minimum(obj.v.double().amax(0), hand.v.double().amax(0))
    klo, khi = torch.stack([torch.ceil(lo / pitch), torch.floor(hi / pitch)]).long().tolist()
    if any(b < a for a, b in zip(klo, khi)):
        return torch.zeros(0, 3, dtype=torch.float64, device=dev)
    ax = [torch.arange(a, b + 1, dtype=torch.float64, device=dev) * pitch for a, b in zip(klo, khi)]
    g = torch.meshgrid(*ax, indexing='ij')
    return torch.stack([x.reshape(-1) for x in g], 1)


def hand_object_meshes(renderer, bmin_hand, bmax_hand, bmin_obj, bmax_obj, resolution, bt_inv, T_pose_21, Ro, To, threshold=0.0):
    """The hand and object meshes of a NeuSRenderer_fitting (get_res.py:219-234) on the device, in world coordinates:
    ((hand vertices float64 [V, 3], hand triangles int64 [T, 3]), (object vertices, object triangles)).  The same volume, mesher and
    index-to-world mapping as extract_geometry(..., mesher='native'), without the copy to the host."""
    from .mesh import marching_cubes
    from .renderer import _grid_points
    out = []
    for kind, bmin, bmax in (('hand', bmin_hand, bmax_hand), ('obj', bmin_obj, bmax_obj)):
        _, lo, hi = _grid_points(bmin, bmax, 2, torch.device('cpu'))
        vol = renderer._volume(bmin, bmax, resolution, bt_inv, T_pose_21, Ro, To, kind)
        v, t = marching_cubes(vol, threshold)
        # renderer._to_world: vertices / (res - 1) * (bmax - bmin) + bmin, the box difference in float32 as the numpy expression has it
        span = torch.from_numpy(hi - lo).to(device=v.device, dtype=torch.float64)
        base = torch.from_numpy(lo).to(device=v.device, dtype=torch.float64)
        out.append((v.double() / (resolution - 1.0) * span[None, :] + base[None, :], t))
    return tuple(out)


def pci(prev_ids, next_ids):
    """analys_pci.get_iou_map's value for two inner-point id sets (get_inner_point_id): |intersection| / (|union| + 1e-7), on the
    host."""
    a = np.unique(np.asarray(prev_ids).reshape(-1))
    b = np.unique(np.asarray(next_ids).reshape(-1))
    return np.intersect1d(a, b).shape[0] / (np.union1d(a, b).shape[0] + 1e-7)

