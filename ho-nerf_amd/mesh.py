"""Marching cubes on the device (hn_mcubes.hip): the mesher behind `extract_geometry(..., mesher='native')`.

What the reference hands to PyMCubes (`mcubes.marching_cubes(u, threshold)`, utils/renderer.py:279-284), with the volume and the
mesh both on the device.  A grid point is inside when its value < threshold; every crossing grid edge carries exactly one vertex,
shared by the cells around it; vertices are in index space, ordered by their edge's lower grid point and then axis x, y, z;
triangles are ordered by cell and face toward increasing value (outward for an SDF).  The output is the same bits on every run.
"""
import torch

from . import lib as _lib


def marching_cubes(volume, threshold=0.0):
    """volume: CUDA float32 [nx, ny, nz] (every dim >= 2) -> (vertices float32 [V, 3] in index space, triangles int64 [T, 3]),
    both on the volume's device, computed on the current stream.  Reads the two totals back (one 16-byte copy) to size the
    outputs."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() != 3:
        raise ValueError('marching_cubes takes a CUDA float32 volume [nx, ny, nz], got %s'
                         % (tuple(volume.shape) if isinstance(volume, torch.Tensor) else type(volume).__name__,))
    lib = _lib.load()
    vol = volume.contiguous()
    nx, ny, nz = (int(s) for s in vol.shape)
    dev = vol.device
    with torch.cuda.device(dev):
        need = lib.hn_mcubes_workspace_bytes(nx, ny, nz)
        ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        st = _lib.stream_ptr()
        _lib.check(lib.hn_mcubes_count(_lib.ptr(vol), nx, ny, nz, float(threshold), _lib.ptr(totals), _lib.ptr(ws), ws.numel(), st),
                   'hn_mcubes_count')
        V, T = (int(x) for x in totals.tolist())
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(T, 3, dtype=torch.int64, device=dev)
        if V and T:
            _lib.check(lib.hn_mcubes_emit(_lib.ptr(vol), nx, ny, nz, float(threshold), _lib.ptr(ws), ws.numel(), V, T, _lib.ptr(vertices),
                                          _lib.ptr(triangles), _lib.stream_ptr()), 'hn_mcubes_emit')
    return vertices, triangles
