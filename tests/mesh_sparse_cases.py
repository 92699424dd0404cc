"""The narrow-band mesher (hn_mcubes_sparse.hip, honerf_amd.mesh.marching_cubes_sparse) restated in numpy: the block lattice, the
classification of blocks, the growth along leaking edges, brick ownership, and the volumes both test files run.  The marching cubes
itself is tests/test_mesh_cpu.py's np_marching_cubes, run on a volume that holds the band's values and +inf everywhere else: what the
restatement returns was computed from band values alone."""
import numpy as np

from test_mesh_cpu import CORNERS, TRI_TABLE, noise_volume, np_marching_cubes, sphere_volume, torus_volume

BLOCKS = (4, 8)


def n_blocks(dims, b):
    return tuple(-(-(n - 1) // b) for n in dims)


def lattice_axes(dims, b):
    """Per axis the grid indices of the block corners: min(i b, n - 1), i = 0 .. nb."""
    return [np.minimum(np.arange(nb + 1) * b, n - 1) for n, nb in zip(dims, n_blocks(dims, b))]


def classify(lat, threshold, reach):
    """lat: float32 lattice values [nbx + 1, nby + 1, nbz + 1] -> bool [nbx, nby, nbz]: the 8 corners do not agree on
    value < threshold, or one of them has |value - threshold| <= reach (fp32, as the kernel)."""
    lat = np.asarray(lat, dtype=np.float32)
    thr, reach = np.float32(threshold), np.float32(reach)
    inside = lat < thr
    dist = np.abs(lat - thr)
    sx, sy, sz = (n - 1 for n in lat.shape)
    cnt = np.zeros((sx, sy, sz), dtype=np.int64)
    near = np.full((sx, sy, sz), np.inf, dtype=np.float32)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += inside[dx:dx + sx, dy:dy + sy, dz:dz + sz]
                near = np.minimum(near, dist[dx:dx + sx, dy:dy + sy, dz:dz + sz])
    return ((cnt != 0) & (cnt != 8)) | (near <= reach)


def containing_blocks(n, b):
    """For every grid index of an axis the (at most two) blocks c with c b <= g <= min((c + 1) b, n - 1), as two arrays (equal where
    there is one)."""
    nb = -(-(n - 1) // b)
    g = np.arange(n)
    hi = np.minimum(g // b, nb - 1)
    lo = np.where((g % b == 0) & (g > 0), g // b - 1, hi)
    for c in (lo, hi):
        assert (c * b <= g).all() and (g <= np.minimum((c + 1) * b, n - 1)).all()
    return lo, hi


def leaking_blocks(vol, threshold, b, active):
    """bool [blocks]: the inactive blocks that contain a crossing grid edge which an active block contains too."""
    dims = vol.shape
    nb = n_blocks(dims, b)
    inside = vol < np.float32(threshold)
    cand = [containing_blocks(n, b) for n in dims]
    add = np.zeros(nb, dtype=bool)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        g = np.stack(np.nonzero(inside[tuple(lo)] != inside[tuple(hi)]), -1)      # the lower end of every crossing edge along a
        if not len(g):
            continue
        u, w = (a + 1) % 3, (a + 2) % 3
        ids = []
        for su in (0, 1):
            for sw in (0, 1):
                c = [None] * 3
                c[a] = g[:, a] // b
                c[u] = cand[u][su][g[:, u]]
                c[w] = cand[w][sw][g[:, w]]
                ids.append((c[0] * nb[1] + c[1]) * nb[2] + c[2])
        ids = np.stack(ids, -1)
        act = active.reshape(-1)[ids]
        leak = act.any(1)[:, None] & ~act
        add.reshape(-1)[ids[leak]] = True
    return add


def band(vol, threshold, b, reach, grow=True, max_grow=16):
    """-> (active bool [blocks], info) as marching_cubes_sparse's steps 1 - 4 leave them."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    ax = lattice_axes(vol.shape, b)
    active = classify(vol[np.ix_(*ax)], threshold, reach)
    info = dict(blocks=int(active.size), active_initial=int(active.sum()), grow_rounds=0, leaks_left=0)
    while True:
        add = leaking_blocks(vol, threshold, b, active)
        k = int(add.sum())
        if not grow or k == 0 or info['grow_rounds'] == max_grow:
            info['leaks_left'] = k
            break
        info['grow_rounds'] += 1
        active = active | add
    info['active'] = int(active.sum())
    info['evaluated'] = int(np.prod([len(x) for x in ax])) + info['active'] * (b + 1) ** 3
    info['dense_points'] = int(vol.size)
    return active, info


def known_points(dims, b, active):
    """bool [dims]: the grid points some active brick holds (the block's points and its +x, +y, +z apron)."""
    known = np.zeros(dims, dtype=bool)
    for c in np.stack(np.nonzero(active), -1):
        known[tuple(slice(ci * b, min((ci + 1) * b, n - 1) + 1) for ci, n in zip(c, dims))] = True
    return known


def mesh_keys(vol, threshold):
    """The keys of np_marching_cubes' outputs, in its order: per vertex 3 (linear index of the owning point) + axis, per triangle
    8 (linear index of the cell's origin) + place in the table."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    inside = vol < np.float32(threshold)
    cross = np.zeros(vol.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vkeys = np.nonzero(cross.reshape(-1))[0].astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ntab = np.array([len(r) // 3 for r in TRI_TABLE])
    cells = np.stack(np.nonzero(ntab[case] > 0), -1)
    cnt = ntab[case[tuple(cells.T)]]
    lin = (cells[:, 0] * ny + cells[:, 1]) * nz + cells[:, 2]
    tkeys = np.concatenate([l * 8 + np.arange(k) for l, k in zip(lin, cnt)]).astype(np.int64) if len(lin) else np.zeros(0, np.int64)
    return vkeys, tkeys


def np_marching_cubes_sparse(vol, threshold, b, reach, grow=True, max_grow=16):
    """The narrow-band mesher on the volume `vol` -> (vertices float32 [V, 3], triangles int64 [T, 3], info).  Marching cubes sees the
    values of the band's bricks and +inf elsewhere; a vertex is kept where the block that owns its edge's lower point is active (a
    point belongs to block min(g // b, nb - 1) per axis), a triangle where the block of its cell is; a kept triangle that uses a
    vertex which is not kept (a leak that was not grown away) is dropped."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    dims = vol.shape
    nb = n_blocks(dims, b)
    active, info = band(vol, threshold, b, reach, grow, max_grow)
    seen = np.where(known_points(dims, b, active), vol, np.float32(np.inf))
    with np.errstate(all='ignore'):
        v, t = np_marching_cubes(seen, threshold)
    vkeys, tkeys = mesh_keys(seen, threshold)
    assert len(vkeys) == len(v) and len(tkeys) == len(t)

    def block_active(lin, top):
        g = np.stack(np.unravel_index(lin, dims), -1)
        c = np.minimum(g // b, np.array(top)[None, :])
        return active[c[:, 0], c[:, 1], c[:, 2]]
    keep_v = block_active(vkeys // 3, [k - 1 for k in nb])
    keep_t = block_active(tkeys // 8, [k - 1 for k in nb])
    new_id = np.cumsum(keep_v) - 1
    t = t[keep_t]
    whole = keep_v[t].all(1)
    assert info['leaks_left'] > 0 or whole.all()
    return v[keep_v], new_id[t[whole]], info


# ---- the volumes --------------------------------------------------------------------------------------------------------------------
def unit_reach(dims, b, lipschitz=1.0):
    """lipschitz x half the diagonal of a full block, for a grid over the unit box [-0.5, 0.5]^3."""
    h = np.array([1.0 / (n - 1) for n in dims])
    return float(lipschitz * 0.5 * b * np.sqrt((h * h).sum()))


def two_spheres_volume(res=64):
    """min of two sphere distances (1-Lipschitz): r = 0.25 at the centre, and r = 0.025 -- smaller than a block of 4 cells -- around a
    point in the interior of a block, away from the first."""
    ax = np.linspace(-0.5, 0.5, res, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    c = (np.array([52.5, 11.5, 43.5]) / (res - 1) - 0.5).astype(np.float32)
    big = np.sqrt(x * x + y * y + z * z) - np.float32(0.25)
    small = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - np.float32(0.025)
    return np.minimum(big, small).astype(np.float32)


def plane_volume(dims=(17, 9, 11)):
    """value = i / 4, exact in fp32: with threshold 2 the points of layer i = 8 (a block face for b = 4 and 8) equal the threshold,
    are not inside, and every vertex sits at t = 1 exactly."""
    return np.broadcast_to((np.arange(dims[0], dtype=np.float32) * np.float32(0.25))[:, None, None], dims).copy()


def steep_volume(res, r):
    """5 (|p| - r): gradient norm 5, meshed with a reach for lipschitz = 1."""
    return (np.float32(5.0) * sphere_volume(res, r)).astype(np.float32)


# Chosen with band(): at 40^3 three tips of the sphere r = 0.12 poke through the middle of a face into a block of 8 cells whose
# corners all lie outside, 2.0 voxels or more from the surface: 5 x 2.0 h = 10 h against a reach of 6.9 h.  The initial band has 8 of
# the 11 blocks that carry triangles.  (Blocks of 4 cells are not missed that way by this field: a cap through a face whose corners
# are more than reach / 5 = 0.69 voxels away needs a sphere of under 5.8 voxels radius, which then fits inside one block.)
STEEP = dict(res=40, r=0.12, block=8)


def cases():
    """name -> (volume, threshold, reach per block edge).  reach is the one of lipschitz = 1 over the unit box, except for the plane
    (index-valued: 1.0)."""
    out = {}
    for res in (33, 64):
        for thr in (0.0, 0.05):
            out['sphere %d thr %g' % (res, thr)] = (sphere_volume(res), thr, None)
    out['torus 50'] = (torus_volume(50), 0.0, None)
    out['noise 23x19x17'] = (noise_volume((23, 19, 17), seed=5), 0.0, None)
    out['two spheres 64'] = (two_spheres_volume(64), 0.0, None)
    out['plane 17x9x11 thr 2'] = (plane_volume(), 2.0, {4: 1.0, 8: 1.0})
    return {k: (v, thr, r or {b: unit_reach(v.shape, b) for b in BLOCKS}) for k, (v, thr, r) in out.items()}
