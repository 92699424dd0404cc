"""Ray casting of triangle meshes on the device (hn_meshcast.hip): what puts a mesh into a camera.

The meshes of a run -- what `extract_geometry(..., mesher='native')` / `interaction.hand_object_meshes` return, what `harness.read_ply`
reads, a CAD model placed with a pose -- are cast with the SAME rays as the volume render (`harness.image_rays`, hn_ray_gen), so a mesh
view and a field view are comparable pixel for pixel (`harness.render_mesh_buffers` against `harness.render_view_buffers`).

The intersection rule is DESIGN.md 3.21 (Woop, Benthin and Wald's watertight scheme in fp32, two-sided, the nearest hit the smallest
(t, face) pair); tests/meshcast_cases.py restates it in numpy.  There are no gradients: an input that requires grad is a ValueError.

Meshes are (vertices [V, 3], triangles [T, 3]): numpy arrays or CUDA tensors (a CPU tensor is refused), checked the way
`interaction` checks its meshes (one read-back of the index ranges).  Results stay on the device.
"""
import torch

from . import lib as _lib
from .interaction import _check, _device, _meshes, _tensor


def _is_pair(x):
    return isinstance(x, (tuple, list)) and len(x) == 2 and not isinstance(x[0], (tuple, list))


def _no_grad(x, what):
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise ValueError('%s requires grad: the mesh ray caster has no backward pass (detach it)' % what)


def morton_order(rows):
    """rows fp32 [T, 9] (a, b, c per triangle) -> int32 [T]: the triangles sorted by the 30-bit Morton code of their centroid in the
    mesh's bounds (stable: equal codes keep the caller's order).  Plumbing (torch.sort); a centroid that is not finite sorts first."""
    T = rows.shape[0]
    if T == 0:
        return torch.zeros(0, dtype=torch.int32, device=rows.device)
    c = torch.nan_to_num(rows.view(T, 3, 3).mean(1), nan=0.0, posinf=0.0, neginf=0.0)
    lo = c.amin(0)
    span = (c.amax(0) - lo).clamp_min(1e-30)
    q = ((c - lo) / span * 1023.0).clamp(0, 1023).long()
    q = (q | (q << 16)) & 0x30000FF
    q = (q | (q << 8)) & 0x300F00F
    q = (q | (q << 4)) & 0x30C30C3
    q = (q | (q << 2)) & 0x9249249
    code = (q[:, 0] << 2) | (q[:, 1] << 1) | q[:, 2]
    return torch.sort(code, stable=True).indices.to(torch.int32).contiguous()


class MeshCaster:
    """One or several meshes prepared for casting.  `meshes`: one (vertices, triangles) pair or a list of them; they are concatenated,
    every triangle remembers its mesh, and the workspace (the triangles in `order`, a box per 64 of them, a box per 32 boxes) is
    prepared once.  `order`: 'morton' (triangles sorted by the Morton code of their centroid: compact boxes whatever order the file
    had) or 'identity' (the caller's order); the results are the same bits either way.

    face_offsets: mesh i owns the faces face_offsets[i] <= face < face_offsets[i + 1] of the concatenation."""

    def __init__(self, meshes, order='morton'):
        if order not in ('morton', 'identity'):
            raise ValueError("MeshCaster: order must be 'morton' or 'identity', got %r" % (order,))
        if _is_pair(meshes):
            meshes = [meshes]
        if not isinstance(meshes, (tuple, list)) or not meshes:
            raise ValueError('MeshCaster: expected (vertices, triangles) or a non-empty list of such pairs')
        for i, m in enumerate(meshes):
            if _is_pair(m):
                _no_grad(m[0], 'MeshCaster: mesh %d vertices' % i)
        ms = _meshes(*[(m, 'MeshCaster mesh %d' % i) for i, m in enumerate(meshes)])
        dev = _device()
        self.n_meshes = len(ms)
        self.face_offsets = [0]
        v_off, vs, ts = 0, [], []
        for m in ms:
            vs.append(m.v32)
            ts.append(m.t + v_off)
            v_off += m.v.shape[0]
            self.face_offsets.append(self.face_offsets[-1] + m.t.shape[0])
        self.vertices = torch.cat(vs).contiguous()                  # fp32 [V, 3]
        self.triangles = torch.cat(ts).contiguous()                 # int64 [T, 3] into self.vertices
        self.n_tris = T = self.triangles.shape[0]
        self._ends = torch.tensor(self.face_offsets[1:], dtype=torch.int32, device=dev)
        L = _lib.load()
        nbytes = int(L.hn_meshcast_workspace_bytes(T))
        if nbytes == 0:
            raise ValueError('MeshCaster: %d triangles, at most 2^31 - 65 are cast' % T)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if T:
            if order == 'morton':
                self.order = morton_order(self.vertices[self.triangles].reshape(T, 9))
            else:
                self.order = torch.arange(T, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _check(L.hn_meshcast_prepare(_lib.ptr(self.vertices), self.vertices.shape[0], _lib.ptr(self.triangles), T, _lib.ptr(self.order),
                                             _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr()), 'MeshCaster')
        else:
            self.order = torch.zeros(0, dtype=torch.int32, device=dev)

    def cast(self, rays_o, rays_d, near, far, cull=True):
        """rays_o, rays_d [N, 3] (d as given: the harness passes unit directions), a hit needs near <= t <= far -> a dict of device
        tensors: t fp32 [N] (0 where nothing is hit), face int32 [N] (into the concatenation, -1), bary fp32 [N, 2] (the weights of
        the triangle's second and third vertex), normal fp32 [N, 3] (the triangle's own unit normal, world frame; 0), mesh int32 [N]
        (the index in the list, -1), hit bool [N].  cull=False walks every block of triangles: the same bits, slower."""
        _no_grad(rays_o, 'cast: rays_o')
        _no_grad(rays_d, 'cast: rays_d')
        o = _tensor(rays_o, 'cast: rays_o').to(torch.float32).contiguous()
        d = _tensor(rays_d, 'cast: rays_d').to(torch.float32).contiguous()
        if o.shape != d.shape:
            raise ValueError('cast: rays_o is %s, rays_d %s' % (tuple(o.shape), tuple(d.shape)))
        N, dev = o.shape[0], o.device
        launch = N > 0 and self.n_tris > 0
        new = torch.empty if launch else torch.zeros
        out = {'t': new(N, dtype=torch.float32, device=dev), 'face': new(N, dtype=torch.int32, device=dev),
               'bary': new(N, 2, dtype=torch.float32, device=dev), 'normal': new(N, 3, dtype=torch.float32, device=dev)}
        if launch:
            with torch.cuda.device(dev):
                _check(_lib.load().hn_meshcast(_lib.ptr(self._ws), self._ws.numel(), self.n_tris, _lib.ptr(o), _lib.ptr(d), N, float(near), float(far),
                                               1 if cull else 0, _lib.ptr(out['t']), _lib.ptr(out['face']), _lib.ptr(out['bary']),
                                               _lib.ptr(out['normal']), _lib.stream_ptr()), 'cast')
        else:
            out['face'].fill_(-1)
        out['hit'] = out['face'] >= 0
        mesh = torch.bucketize(out['face'], self._ends, right=True).to(torch.int32)
        out['mesh'] = torch.where(out['hit'], mesh, torch.full_like(mesh, -1))
        return out
