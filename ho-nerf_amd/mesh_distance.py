"""Mesh-to-mesh surface distance on the device (hn_meshdist.hip): the closest point on a mesh, a surface sampler, and the metrics that
score one surface against another -- Chamfer distance, accuracy / completeness, precision / recall / F-score at thresholds, Hausdorff
distance and normal consistency.

DESIGN.md 3.27 is the contract; tests/mesh_distance_cases.py restates it in numpy.  The closest-point query is exact (Ericson's
point-triangle distance in fp32, the arithmetic of `interaction.closest_distance` bit for bit) and culled by the ray caster's two-level
boxes; the winner is the smallest (squared distance, face) pair, so the result depends neither on the order of the triangles nor on
what was culled.  There are no gradients: an input that requires grad is a ValueError.

Meshes are (vertices [V, 3], triangles [T, 3]) and points [P, 3]: numpy arrays or CUDA tensors (a CPU tensor is refused), checked the
way `interaction` checks its meshes (one read-back of the index ranges).  Results stay on the device, except the metrics' scalars.
"""
import math

import torch

from . import lib as _lib
from .interaction import _check, _device, _Mesh, _meshes, _tensor
from .meshcast import morton_order


def _no_grad(x, what):
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise ValueError('%s requires grad: the mesh distance queries have no backward pass (detach it)' % what)


def _mesh(mesh, what):
    if isinstance(mesh, _Mesh):
        return mesh
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        _no_grad(mesh[0], what + ' vertices')
    return _meshes((mesh, what))[0]


def _morton_points(p):
    """p fp32 [P, 3] -> int64 [P]: the points sorted by the 30-bit Morton code of their position in their own bounds (stable).
    Plumbing (torch.sort); a point that is not finite sorts first."""
    c = torch.nan_to_num(p, nan=0.0, posinf=0.0, neginf=0.0)
    lo = c.amin(0)
    span = (c.amax(0) - lo).clamp_min(1e-30)
    q = ((c - lo) / span * 1023.0).clamp(0, 1023).long()
    q = (q | (q << 16)) & 0x30000FF
    q = (q | (q << 8)) & 0x300F00F
    q = (q | (q << 4)) & 0x30C30C3
    q = (q | (q << 2)) & 0x9249249
    code = (q[:, 0] << 2) | (q[:, 1] << 1) | q[:, 2]
    return torch.sort(code, stable=True).indices


def _face_areas(m):
    """-> (area fp64 [T], unit normal fp32 [T, 3]) of a checked mesh (hn_mesh_face_areas)."""
    T, dev = m.t.shape[0], m.v.device
    area = torch.zeros(T, dtype=torch.float64, device=dev)
    normal = torch.zeros(T, 3, dtype=torch.float32, device=dev)
    if T:
        with torch.cuda.device(dev):
            _check(_lib.load().hn_mesh_face_areas(_lib.ptr(m.v32), m.v32.shape[0], _lib.ptr(m.t), T, _lib.ptr(area), _lib.ptr(normal),
                                                  _lib.stream_ptr()), 'face areas')
    return area, normal


class MeshIndex:
    """A mesh prepared for closest-point queries: the triangles in `order`, a box per 64 of them, a box per 32 boxes, prepared once.
    `order`: 'morton' (triangles sorted by the Morton code of their centroid: compact boxes whatever order the file had), 'identity'
    (the caller's order) or an int32 permutation of the triangles; the results are the same bits whichever it is."""

    def __init__(self, mesh, order='morton'):
        if isinstance(order, str) and order not in ('morton', 'identity'):
            raise ValueError("MeshIndex: order must be 'morton', 'identity' or a permutation, got %r" % (order,))
        m = self._mesh = _mesh(mesh, 'MeshIndex mesh')
        dev = _device()
        self.vertices = m.v32                                          # fp32 [V, 3]
        self.triangles = m.t                                           # int64 [T, 3]
        self.n_tris = T = m.t.shape[0]
        L = _lib.load()
        nbytes = int(L.hn_meshdist_workspace_bytes(T))
        if nbytes == 0:
            raise ValueError('MeshIndex: %d triangles, at most 2^31 - 66 are indexed' % T)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._normals = None
        if isinstance(order, str):
            if T and order == 'morton':
                order = morton_order(m.rows(torch.float32))
            else:
                order = torch.arange(T, dtype=torch.int32, device=dev)
        else:
            order = torch.as_tensor(order)
            if order.dim() != 1 or order.shape[0] != T or order.dtype not in (torch.int32, torch.int64):
                raise ValueError('MeshIndex: order must be an integer permutation of the %d triangles' % T)
            order = order.to(device=dev, dtype=torch.int32).contiguous()
        self.order = order
        if T:
            with torch.cuda.device(dev):
                _check(L.hn_meshdist_prepare(_lib.ptr(self.vertices), self.vertices.shape[0], _lib.ptr(self.triangles), T, _lib.ptr(self.order),
                                             _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr()), 'MeshIndex')

    @property
    def face_normals(self):
        """fp32 [T, 3]: the unit normal of every face (0 for a face without area)."""
        if self._normals is None:
            self._normals = _face_areas(self._mesh)[1]
        return self._normals

    def closest(self, points, cull=True, sort=True, want=('dist', 'face', 'point', 'bary')):
        """points [P, 3] -> a dict of device tensors: dist fp32 [P] (inf for a mesh without triangles), face int32 [P] (the caller's
        index; the smallest among triangles at the same fp32 squared distance; -1), point fp32 [P, 3] (the closest point; 0), bary fp32
        [P, 2] (the weights of the triangle's second and third vertex; 0).  cull=False walks every block of triangles; sort=True hands
        the points to the kernel in Morton order (a workgroup's points then share blocks) and scatters the results back: the same
        bits either way.  `want`: the outputs to compute."""
        _no_grad(points, 'closest: points')
        p = _tensor(points, 'closest: points').to(torch.float32).contiguous()
        P, dev = p.shape[0], p.device
        launch = P > 0 and self.n_tris > 0
        new = torch.empty if launch else torch.zeros
        shapes = {'dist': ((P,), torch.float32), 'face': ((P,), torch.int32), 'point': ((P, 3), torch.float32), 'bary': ((P, 2), torch.float32)}
        out = {k: new(shapes[k][0], dtype=shapes[k][1], device=dev) for k in shapes if k in want}
        if not launch:
            if 'dist' in out:
                out['dist'].fill_(float('inf'))
            if 'face' in out:
                out['face'].fill_(-1)
            return out
        perm = _morton_points(p) if sort and P > 256 else None         # (one workgroup: nothing to gather)
        q = p[perm].contiguous() if perm is not None else p
        with torch.cuda.device(dev):
            _check(_lib.load().hn_meshdist_closest(_lib.ptr(self._ws), self._ws.numel(), self.n_tris, _lib.ptr(q), P, 1 if cull else 0,
                                                   _lib.ptr(out.get('dist')), _lib.ptr(out.get('face')), _lib.ptr(out.get('point')),
                                                   _lib.ptr(out.get('bary')), _lib.stream_ptr()), 'closest')
        if perm is not None:
            for k, v in out.items():
                back = torch.empty_like(v)
                back[perm] = v
                out[k] = back
        return out


def vertex_distance(points, mesh):
    """The distance from every point to the mesh -> fp32 [P] on the device: the one-direction query for callers with their own points."""
    return MeshIndex(mesh).closest(points, want=('dist',))['dist']


def _sample(m, n, seed, what):
    n, seed = int(n), int(seed)
    if n < 0 or n >= 2 ** 31 - 65:
        raise ValueError('%s: n = %d outside [0, 2^31 - 65)' % (what, n))
    if not 0 <= seed < 2 ** 32:
        raise ValueError('%s: seed = %d outside [0, 2^32)' % (what, seed))
    area, _ = _face_areas(m)
    cum = torch.cumsum(area, 0)                                        # fp64, inclusive (plumbing; the same bits on every run)
    total = float(cum[-1]) if cum.numel() else 0.0
    if not (total > 0.0 and math.isfinite(total)):
        raise ValueError('%s: the mesh has a total area of %r: nothing to sample' % (what, total))
    dev = m.v.device
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    nrm = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if n:
        with torch.cuda.device(dev):
            _check(_lib.load().hn_mesh_sample(_lib.ptr(m.v32), m.v32.shape[0], _lib.ptr(m.t), m.t.shape[0], _lib.ptr(cum), n, seed, _lib.ptr(pts),
                                              _lib.ptr(face), _lib.ptr(nrm), _lib.stream_ptr()), what)
    return pts, face, nrm, total


def sample_surface(mesh, n, seed=0):
    """n points on the mesh's surface, uniform by area and stratified, deterministic in (mesh, n, seed) -> (points fp32 [n, 3], face
    int32 [n], normal fp32 [n, 3], the face's unit normal) on the device.  DESIGN.md 3.27 has the formula.  ValueError for a mesh of
    zero total area."""
    return _sample(_mesh(mesh, 'sample_surface mesh'), n, seed, 'sample_surface')[:3]


def _direction(samples, normals, index):
    """One direction of the comparison -> (distances fp64 [n], mean |n_sample . n_closest face| as a device scalar)."""
    r = index.closest(samples, want=('dist', 'face'))
    fn = index.face_normals[r['face'].long().clamp_min(0)]
    dots = (normals.double() * fn.double()).sum(1).abs()
    return r['dist'].double(), dots.mean()


def surface_metrics(pred, gt, n=100_000, taus=(0.005, 0.010), seed=0, samples=None, align=None, icp_iters=30):
    """pred and gt meshes scored against each other -> a dict of Python floats, in the meshes' units.  acc: the distances from n
    samples of pred (seed) to gt; comp: from n samples of gt (seed + 1) to pred.
      chamfer_l1 = (mean acc + mean comp) / 2, chamfer_l2 = mean acc^2 + mean comp^2, hausdorff = max of both maxima,
      accuracy = mean acc, completeness = mean comp, precision@tau = share of acc <= tau, recall@tau = share of comp <= tau,
      fscore@tau = 2 p r / (p + r) (0 when p + r = 0), normal_consistency = the mean of both directions' mean |n_sample . n_face|,
      n, pred_area, gt_area.
    Every sum is an fp64 reduction of the device, the same bits on every run.  `samples`: a dict that receives the device's own
    samples (pred_points, pred_normals, gt_points, gt_normals), for callers that check the metrics.

    align='icp' (rigid) or 'icp+scale' (similarity): the pred mesh is first moved onto gt by `alignment.icp` of its n samples against
    the gt mesh (`icp_iters` iterations), so that a global pose offset stops dominating a shape score.  The pred SAMPLES are
    transformed, not redrawn, their normals rotated; comp is measured against the moved pred mesh.  The dict gains `transform` (R
    [3, 3], s, t as nested lists and floats, float64) and `icp_rms` (the ICP's RMS trace, a list); pred_area stays the unmoved mesh's.
    None: nothing is aligned."""
    if align not in (None, 'icp', 'icp+scale'):
        raise ValueError("surface_metrics: align must be None, 'icp' or 'icp+scale', got %r" % (align,))
    mp, mg = _mesh(pred, 'surface_metrics pred'), _mesh(gt, 'surface_metrics gt')
    n = int(n)
    if n < 1:
        raise ValueError('surface_metrics: n = %d, at least one sample per mesh is needed' % n)
    taus = [float(t) for t in taus]
    pp, _, pn, pa = _sample(mp, n, seed, 'surface_metrics pred')
    gp, _, gn, ga = _sample(mg, n, (int(seed) + 1) % 2 ** 32, 'surface_metrics gt')
    if samples is not None:
        samples.update(pred_points=pp, pred_normals=pn, gt_points=gp, gt_normals=gn)
    index_g = MeshIndex(mg)
    moved = None
    if align is not None:
        from . import alignment
        moved = alignment.icp(pp, index_g, iters=icp_iters, scale=align == 'icp+scale')
        R, s, t = moved['R'][None].contiguous(), moved['s'][None].contiguous(), moved['t'][None].contiguous()
        pp = moved['aligned']
        pn = (pn.double() @ R[0].T).float().contiguous()              # (unit normals: a rotation of 3-vectors, plumbing)
        mp = _Mesh(alignment._apply(mp.v32[None].contiguous(), R, s, t)[0], mp.t)
        if samples is not None:
            samples.update(pred_points=pp, pred_normals=pn)
    acc, nc_a = _direction(pp, pn, index_g)
    comp, nc_c = _direction(gp, gn, MeshIndex(mp))
    vals = [acc.mean(), comp.mean(), (acc * acc).mean(), (comp * comp).mean(), acc.max(), comp.max(), nc_a, nc_c]
    for t in taus:
        vals += [(acc <= t).sum().double(), (comp <= t).sum().double()]   # (counts: exact in fp64, divided on the host)
    vals = torch.stack(vals).tolist()                                  # the one read-back
    ma, mc, ma2, mc2, xa, xc, nca, ncc = vals[:8]
    out = dict(chamfer_l1=(ma + mc) / 2.0, chamfer_l2=ma2 + mc2, hausdorff=max(xa, xc), accuracy=ma, completeness=mc,
               normal_consistency=(nca + ncc) / 2.0, n=n, pred_area=pa, gt_area=ga)
    for k, t in enumerate(taus):
        p, r = vals[8 + 2 * k] / n, vals[9 + 2 * k] / n
        out['precision@%g' % t], out['recall@%g' % t] = p, r
        out['fscore@%g' % t] = 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0
    if moved is not None:
        tr = torch.cat([moved['R'].reshape(-1), moved['s'].reshape(-1), moved['t'].reshape(-1)]).tolist()
        out['transform'] = dict(R=[tr[0:3], tr[3:6], tr[6:9]], s=tr[9], t=tr[10:13])
        out['icp_rms'] = [float(x) for x in moved['rms']]
    return out
