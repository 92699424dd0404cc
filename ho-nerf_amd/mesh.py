"""Marching cubes on the device: the meshers behind `extract_geometry(..., mesher='native')` (hn_mcubes.hip, a dense volume) and
`mesher='sparse'` (hn_mcubes_sparse.hip, values in a band of blocks around the level set only; the same mesh, bit for bit).

What the reference hands to PyMCubes (`mcubes.marching_cubes(u, threshold)`, utils/renderer.py:279-284), with the volume and the
mesh both on the device.  A grid point is inside when its value < threshold; every crossing grid edge carries exactly one vertex,
shared by the cells around it; vertices are in index space, ordered by their edge's lower grid point and then axis x, y, z;
triangles are ordered by cell and face toward increasing value (outward for an SDF).  The output is the same bits on every run.

`marching_cubes_sparse` never sees a volume: it asks a callback for the field at grid indices -- first at the corners of blocks of
`block`^3 cells, then at the (block + 1)^3 points of every block the corners make a candidate -- and follows the surface into blocks
the corners missed, until no crossing edge leaves the band.  Field evaluations scale with the surface, not with the grid.
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


def marching_cubes_sparse(values_at, dims, threshold=0.0, *, block=8, reach, grow=True, max_grow=16, chunk=1 << 22, device=None):
    """The mesh `marching_cubes` gives for the volume `values_at` would fill, without the volume.

    values_at(idx): device int32 grid indices [n, 3] -> float32 values [n] on the same device; the value of a grid point must not
    depend on the call it is asked in.  dims = (nx, ny, nz), every dim in [2, 2048]; block = 4 or 8 cells per block edge.
    -> (vertices float32 [V, 3] in index space, triangles int64 [T, 3], info), computed on the current stream of `device` (default:
    the current CUDA device).

    1. the field at the block corners; 2. a block is a candidate if its 8 corners do not agree on value < threshold or one of them is
    within `reach` of the threshold (with reach >= L d / 2 for a field of gradient norm <= L and blocks of diagonal d, every block the
    surface passes through is one); 3. the (block + 1)^3 values of every candidate, asked in calls of at most `chunk` points;
    4. grow: a crossing grid edge on a candidate's boundary makes the blocks that share it candidates too, until none is added or
    `max_grow` rounds have passed (existing bricks keep their values; one 8-byte read-back per round); 5. marching cubes over the
    bricks; 6. torch.sort of the per-vertex and per-triangle keys puts both arrays in the dense mesher's order.

    A surface component that neither meets a corner test nor is connected to one that does is not found.  With leaks left (grow=False,
    or max_grow too small) the triangles whose vertex lies in a block outside the band are dropped: the mesh has holes there.

    info: blocks, active_initial, active, grow_rounds, leaks_left (0 when growth converged; with grow=False what one leak search
    found), evaluated (points passed to values_at in total), dense_points."""
    nx, ny, nz = (int(d) for d in dims)
    block = int(block)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    thr, P = float(threshold), (block + 1) ** 3
    g = (nx, ny, nz, block)
    with torch.cuda.device(dev):
        need = lib.hn_mcs_workspace_bytes(*g, 0)
        if need == 0:
            _lib.check(lib.hn_mcs_lattice(*g, None, _lib.stream_ptr()), 'hn_mcs_lattice')     # says which argument is refused
        nb = [-(-(n - 1) // block) for n in (nx, ny, nz)]
        n_blocks, n_lat = nb[0] * nb[1] * nb[2], (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1)
        info = dict(blocks=n_blocks, active_initial=0, active=0, grow_rounds=0, leaks_left=0, evaluated=0, dense_points=nx * ny * nz)

        def ask(idx):
            val = values_at(idx)
            if not isinstance(val, torch.Tensor) or val.dtype != torch.float32 or val.device != idx.device or val.numel() != idx.shape[0]:
                raise ValueError('values_at must return %d float32 values on %s' % (idx.shape[0], idx.device))
            info['evaluated'] += idx.shape[0]
            return val.reshape(-1)

        def fill(blocks, out):
            """The bricks of the block ids `blocks` (int32) into out [len(blocks), P]."""
            per = max(1, int(chunk) // P)
            for s0 in range(0, blocks.numel(), per):
                s1 = min(blocks.numel(), s0 + per)
                idx = torch.empty((s1 - s0) * P, 3, dtype=torch.int32, device=dev)
                _lib.check(lib.hn_mcs_brick_points(_lib.ptr(blocks), s0, s1, *g, _lib.ptr(idx), _lib.stream_ptr()), 'hn_mcs_brick_points')
                out[s0:s1] = ask(idx).reshape(s1 - s0, P)

        idx = torch.empty(n_lat, 3, dtype=torch.int32, device=dev)
        _lib.check(lib.hn_mcs_lattice(*g, _lib.ptr(idx), _lib.stream_ptr()), 'hn_mcs_lattice')
        lattice = ask(idx).contiguous()
        mask = torch.empty(n_blocks, dtype=torch.uint8, device=dev)
        _lib.check(lib.hn_mcs_classify(_lib.ptr(lattice), *g, thr, float(reach), _lib.ptr(mask), _lib.stream_ptr()), 'hn_mcs_classify')
        ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
        blist = torch.empty(n_blocks, dtype=torch.int32, device=dev)
        table = torch.empty(n_blocks, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)

        def compact():
            _lib.check(lib.hn_mcs_compact(_lib.ptr(mask), *g, _lib.ptr(blist), _lib.ptr(table), _lib.ptr(total), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()), 'hn_mcs_compact')
            return int(total.item())

        def leaks():
            _lib.check(lib.hn_mcs_leaks(_lib.ptr(bricks), _lib.ptr(blist), _lib.ptr(table), n, *g, thr, _lib.ptr(mask), _lib.ptr(total),
                                        _lib.stream_ptr()), 'hn_mcs_leaks')

        n = compact()
        info['active_initial'] = n
        bricks = torch.empty(n, P, dtype=torch.float32, device=dev)
        fill(blist[:n], bricks)
        if not grow:
            leaks()
            info['leaks_left'] = int(total.item())
        while grow:
            leaks()
            old = blist[:n].clone()
            n_new = compact()                       # the round's read-back: the new total says whether anything was added
            if n_new == n:
                break
            if info['grow_rounds'] == max_grow:     # marked but not filled: what is left
                info['leaks_left'] = n_new - n
                mask.zero_()
                mask[old.long()] = 1
                n = compact()
                break
            info['grow_rounds'] += 1
            kept = table[old.long()].long()          # where the bricks we hold sit in the new list
            grown = torch.empty(n_new, P, dtype=torch.float32, device=dev)
            grown[kept] = bricks
            is_new = torch.ones(n_new, dtype=torch.bool, device=dev)
            is_new[kept] = False
            new_slots = torch.nonzero(is_new).reshape(-1)
            fresh = torch.empty(new_slots.numel(), P, dtype=torch.float32, device=dev)
            fill(blist[:n_new][new_slots].contiguous(), fresh)
            grown[new_slots] = fresh
            bricks, n = grown, n_new
        info['active'] = n

        need = lib.hn_mcs_workspace_bytes(*g, n)
        ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.hn_mcs_count(_lib.ptr(bricks), _lib.ptr(blist), n, *g, thr, _lib.ptr(totals), _lib.ptr(ws), ws.numel(),
                                    _lib.stream_ptr()), 'hn_mcs_count')
        V, T = (int(x) for x in totals.tolist())
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(T, 3, dtype=torch.int64, device=dev)
        if not (V and T):
            return vertices, triangles, info
        vkeys = torch.empty(V, dtype=torch.int64, device=dev)
        tkeys = torch.empty(T, dtype=torch.int64, device=dev)
        _lib.check(lib.hn_mcs_emit(_lib.ptr(bricks), _lib.ptr(blist), _lib.ptr(table), n, *g, thr, _lib.ptr(ws), ws.numel(), V, T,
                                   _lib.ptr(vertices), _lib.ptr(vkeys), _lib.ptr(triangles), _lib.ptr(tkeys), _lib.stream_ptr()),
                   'hn_mcs_emit')
        del bricks, ws
        # brick-major -> the dense mesher's order: vertices by (owning point, axis), triangles by (cell, table slot); keys are unique
        _, order = torch.sort(vkeys)
        vertices = vertices[order]
        rank = torch.empty_like(order)
        rank[order] = torch.arange(V, dtype=torch.int64, device=dev)
        if info['leaks_left']:
            whole = (triangles >= 0).all(dim=1)
            triangles, tkeys = triangles[whole], tkeys[whole]
        triangles = rank[triangles]
        _, order = torch.sort(tkeys)
        triangles = triangles[order]
    return vertices, triangles, info
