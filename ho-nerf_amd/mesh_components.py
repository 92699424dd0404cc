"""Connected components of a triangle mesh on the device (hn_meshcc.hip): split, measure, drop floaters.

A marching-cubes mesh of a learned SDF is rarely one surface: it comes with floaters, with shells cut open by the box and with interior
bubbles, and every consumer here (`interaction`, `meshcast`) takes the mesh as it is.  This is the step trimesh users reach for
(`Trimesh.split`, `.area`, `.volume`, `.is_watertight` per body), on the tensors `mesh.marching_cubes` leaves on the device.

The rule (tests/meshcc_cases.py restates it in numpy).  Two triangles belong to the same component when they share a
vertex INDEX, transitively: vertex connectivity.  trimesh's `split` joins faces over shared edges; the two differ only at pinch vertices
(two fans meeting in one vertex and no edge are one component here).  A component's label is the smallest vertex index its triangles
use; components are numbered 0 .. C-1 in ascending label order (the component index).  A vertex no triangle uses has label and
component -1.  Duplicate vertices are not welded: two shells that touch in space but share no index are two components.

Meshes are (vertices [V, 3], triangles [T, 3]): numpy arrays or CUDA tensors (a CPU tensor is refused), fp32 or fp64 vertices, int32 or
int64 triangles, checked the way `interaction` checks its meshes (out-of-range indices raise ValueError; one host sync).  Results stay
on the device and are the same bits on every run; everything runs on the current stream.
"""
import torch

from . import lib as _lib
from .interaction import _check, _device, _meshes

MEASURES = ('faces', 'vertices', 'area', 'volume', 'bounds', 'closed')


def _checked(mesh, what):
    m, = _meshes((mesh, what))
    m.v = m.v.contiguous()
    return m


def _ws(nbytes, what, dev):
    if nbytes == 0:
        raise ValueError('%s: the mesh is too large (counts must stay below 2^31 - 256)' % what)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _components(m):
    dev = m.v.device
    V, T = m.v.shape[0], m.t.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    if T == 0:                       # no launch
        return dict(n=0, label=torch.zeros(0, **i32), vertex_label=torch.full((V,), -1, **i32), face_label=torch.zeros(0, **i32),
                    vertex_component=torch.full((V,), -1, **i32), face_component=torch.zeros(0, **i32))
    L = _lib.load()
    with torch.cuda.device(dev):
        ws = _ws(L.hn_meshcc_workspace_bytes(V, T), 'components', dev)
        out = {k: torch.empty(V if k.startswith('vertex') else T, **i32) for k in ('vertex_label', 'face_label', 'vertex_component', 'face_component')}
        label = torch.empty(V, **i32)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        _check(L.hn_meshcc_label(_lib.ptr(m.t), V, T, _lib.ptr(out['vertex_label']), _lib.ptr(out['face_label']), _lib.ptr(out['vertex_component']),
                                 _lib.ptr(out['face_component']), _lib.ptr(label), _lib.ptr(total), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               'components')
        C = int(total.item())        # the one read-back (8 bytes), as marching_cubes reads its totals
    out['n'] = C
    out['label'] = label[:C].clone()
    return out


def _comps_of(m, comps):
    if comps is None:
        return _components(m)
    V, T = m.v.shape[0], m.t.shape[0]
    try:
        ok = (int(comps['n']) == comps['label'].shape[0] and tuple(comps['vertex_component'].shape) == (V,)
              and tuple(comps['face_component'].shape) == (T,) and comps['vertex_component'].dtype == torch.int32
              and comps['face_component'].dtype == torch.int32 and comps['face_component'].is_cuda)
    except (KeyError, TypeError, AttributeError):
        ok = False
    if not ok:
        raise ValueError('comps: expected what components() returned for this mesh (%d vertices, %d triangles)' % (V, T))
    return comps


def _closed_per_component(t, face_component, n_verts, C):
    """interaction.is_closed's rule per component, bool [C], without a host sync: a directed edge is bad when another face uses the
    same one or no face uses its reverse; a component is closed when none of its edges is bad.  (Components share no vertex, so an
    edge's code is looked up among its own component's.)"""
    d = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    comp = face_component.long().repeat(3)
    code = d[:, 0] * n_verts + d[:, 1]
    rev = d[:, 1] * n_verts + d[:, 0]
    s, idx = torch.sort(code)
    same = s[1:] == s[:-1]
    twice = torch.zeros_like(s, dtype=torch.bool)
    twice[1:] |= same
    twice[:-1] |= same
    pos = torch.searchsorted(s, rev).clamp(max=s.shape[0] - 1)
    bad = s[pos] != rev
    bad[idx] |= twice
    n_bad = torch.zeros(C, dtype=torch.int64, device=t.device).index_add_(0, comp, bad.long())
    return n_bad == 0


def _measure(m, comps):
    dev = m.v.device
    V, T, C = m.v.shape[0], m.t.shape[0], int(comps['n'])
    out = dict(faces=torch.zeros(C, dtype=torch.int64, device=dev), vertices=torch.zeros(C, dtype=torch.int64, device=dev),
               area=torch.zeros(C, dtype=torch.float64, device=dev), volume=torch.zeros(C, dtype=torch.float64, device=dev),
               bounds=torch.zeros(C, 6, dtype=m.v.dtype, device=dev), closed=torch.zeros(C, dtype=torch.bool, device=dev))
    if T == 0 or C == 0:
        return out
    L = _lib.load()
    fc = comps['face_component'].contiguous()
    vc = comps['vertex_component'].contiguous()
    order = torch.sort(fc, stable=True).indices.contiguous()     # plumbing: the faces by component, each component's in face order
    with torch.cuda.device(dev):
        ws = _ws(L.hn_meshcc_measure_workspace_bytes(T, C), 'measure', dev)
        _check(L.hn_meshcc_measure(_lib.ptr(m.v), 1 if m.v.dtype == torch.float64 else 0, V, _lib.ptr(m.t), T, _lib.ptr(vc), _lib.ptr(fc),
                                   _lib.ptr(order), C, _lib.ptr(out['faces']), _lib.ptr(out['vertices']), _lib.ptr(out['area']),
                                   _lib.ptr(out['volume']), _lib.ptr(out['bounds']), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'measure')
    out['closed'] = _closed_per_component(m.t, fc, V, C)
    return out


def components(mesh):
    """-> dict: n (int, the number of components C), label int32 [C] (ascending: the smallest vertex index of each component),
    vertex_label, vertex_component int32 [V] (-1 for a vertex no triangle uses), face_label, face_component int32 [T].  One read-back
    (C) beside the index check.  A mesh without triangles has n = 0 and launches nothing."""
    return _components(_checked(mesh, 'mesh'))


def measure(mesh, comps=None):
    """Per component -> dict of device tensors [C]: faces, vertices int64; area fp64 (sum of 0.5 |(b - a) x (c - a)|); volume fp64 (sum
    of a . (b x c) / 6, signed: positive for an outward-oriented closed surface, as the mesher's are; not a volume for an open one);
    bounds [C, 6] in the vertices' precision (min xyz, max xyz of the used vertices); closed bool (`interaction.is_closed`'s rule on
    the component's faces).  Terms are fp64 from the vertices converted to fp64, summed in ascending face order with a fixed tree: fp32
    and fp64 vertices of the same values give the same bits.  `comps`: what components(mesh) returned (else it is computed)."""
    m = _checked(mesh, 'mesh')
    return _measure(m, _comps_of(m, comps))


def _criterion_mask(meas, C, dev, largest, min_faces, min_area_fraction, closed_only, mask):
    if largest is None and min_faces is None and min_area_fraction is None and not closed_only and mask is None:
        raise ValueError('keep: no criterion (largest, min_faces, min_area_fraction, closed_only or mask)')
    sel = torch.ones(C, dtype=torch.bool, device=dev)
    if mask is not None:
        mk = torch.as_tensor(mask)
        if mk.dim() != 1 or mk.shape[0] != C:
            raise ValueError('keep: mask of shape %s, expected [%d] (one entry per component)' % (tuple(mk.shape), C))
        sel &= mk.to(dev).bool()
    if largest is not None:
        if int(largest) != largest or int(largest) < 1:
            raise ValueError('keep: largest must be a positive integer, got %r' % (largest,))
        top = torch.sort(meas['faces'], descending=True, stable=True).indices[:int(largest)]     # ties: the smaller label first
        pick = torch.zeros(C, dtype=torch.bool, device=dev)
        pick[top] = True
        sel &= pick
    if min_faces is not None:
        sel &= meas['faces'] >= int(min_faces)
    if min_area_fraction is not None:
        sel &= meas['area'] >= float(min_area_fraction) * meas['area'].sum()
    if closed_only:
        sel &= meas['closed']
    return sel


def keep(mesh, comps=None, largest=None, min_faces=None, min_area_fraction=None, closed_only=False, mask=None):
    """The part of the mesh whose components pass every given criterion (they combine with AND) -> (vertices', triangles', info).
      largest=k            the k components with the most faces (ties go to the smaller label);
      min_faces=n          at least n faces;
      min_area_fraction=f  an area of at least f times the whole mesh's;
      closed_only=True     closed components only (measure's `closed`);
      mask                 an explicit bool [C].
    No criterion at all is a ValueError.  Kept vertices and faces stay in their original order; vertex rows are copied bit for bit (in
    their dtype), triangles are re-indexed (int64); vertices no triangle uses are dropped.  info: vertex_map int32 [V] and face_map int32
    [T] (the new index, or -1), kept int64 [K] (component indices), and the measures of the kept components (faces, vertices, area,
    volume, bounds, closed, each [K]).  One 16-byte read-back ({V', T'}) beside those of components().  A mesh without triangles
    comes back empty without a launch."""
    m = _checked(mesh, 'mesh')
    dev = m.v.device
    V, T = m.v.shape[0], m.t.shape[0]
    comps = _comps_of(m, comps)
    C = int(comps['n'])
    meas = _measure(m, comps)
    sel = _criterion_mask(meas, C, dev, largest, min_faces, min_area_fraction, closed_only, mask)
    kept = torch.nonzero(sel).reshape(-1)
    info = dict(kept=kept, **{k: meas[k][kept] for k in MEASURES})
    if T == 0:
        info.update(vertex_map=torch.full((V,), -1, dtype=torch.int32, device=dev), face_map=torch.zeros(0, dtype=torch.int32, device=dev))
        return m.v[:0].clone(), m.t[:0].clone(), info
    L = _lib.load()
    flags = sel.to(torch.uint8).contiguous()
    fc, vc = comps['face_component'].contiguous(), comps['vertex_component'].contiguous()
    f64 = 1 if m.v.dtype == torch.float64 else 0
    with torch.cuda.device(dev):
        ws = _ws(L.hn_meshcc_workspace_bytes(V, T), 'keep', dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        _check(L.hn_meshcc_compact_count(_lib.ptr(vc), V, _lib.ptr(fc), T, _lib.ptr(flags), C, _lib.ptr(totals), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), 'keep')
        Vk, Tk = (int(x) for x in totals.tolist())
        v_out = torch.empty(Vk, 3, dtype=m.v.dtype, device=dev)
        t_out = torch.empty(Tk, 3, dtype=torch.int64, device=dev)
        info['vertex_map'] = torch.empty(V, dtype=torch.int32, device=dev)
        info['face_map'] = torch.empty(T, dtype=torch.int32, device=dev)
        _check(L.hn_meshcc_compact_emit(_lib.ptr(m.v), f64, V, _lib.ptr(m.t), T, _lib.ptr(vc), _lib.ptr(fc), _lib.ptr(flags), C, _lib.ptr(ws), ws.numel(),
                                        Vk, Tk, _lib.ptr(v_out) if Vk else None, _lib.ptr(t_out) if Tk else None, _lib.ptr(info['vertex_map']),
                                        _lib.ptr(info['face_map']), _lib.stream_ptr()), 'keep')
    return v_out, t_out, info


def largest(mesh):
    """The component with the most faces -> (vertices', triangles'): keep(mesh, largest=1)[:2]."""
    return keep(mesh, largest=1)[:2]
