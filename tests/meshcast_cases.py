"""Cases of the mesh ray caster (ho-nerf_amd/csrc/hn_meshcast.hip): the meshes, the ray sets, and the intersection rule of DESIGN.md
3.21 in numpy.  A plain module, in the manner of gbuffer_cases: tests/test_meshcast_cpu.py (is the fp32 restatement the float64
reference on every settled ray?) and tests/test_gpu_meshcast.py (is the kernel the fp32 restatement on every ray?) both import it.

`rule(verts, tris, o, d, near, far, f)` is the rule, statement by statement, in the number format `f`:
  f = np.float64   the REFERENCE (on the same fp32 inputs cast up);
  f = np.float32   the FP32 RESTATEMENT: every product, difference, sum and quotient rounded to fp32 where the kernel rounds it, in the
                   kernel's operation order -- numpy's float32 arithmetic is correctly rounded, as the device's is, so the kernel is
                   expected to give these bits.

    kz = argmax |d_i| (lowest index on ties), kx, ky the next two cyclically, swapped when d[kz] < 0
    Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
    A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz]            (B, C likewise)
    U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;  where one is exactly 0: all three from float64 products, rounded to f
    a miss when one of U, V, W is negative while another is positive, and when det = (U + V) + W is 0
    t = ((U Az + V Bz) + W Cz) / det, Az = Sz A[kz];  a hit needs near <= t <= far;  weights of b, c: V / det, W / det
    the nearest hit: the smallest (t, face);  normal = normalize((b - a) x (c - a)), the length as sqrt((nx^2 + ny^2) + nz^2)
    never hit: a triangle with a vertex that is not finite or whose fp32 (b - a) x (c - a) has squared length 0 or not finite (its
    vertices become NaN, as in the kernel's workspace), and a ray with d[kz] = 0

A ray is SETTLED (`settled`, on the reference) when its nearest hit has every barycentric weight >= 1e-3 and the next hit of another
triangle is more than 1e-3 behind it, or, if it misses, no triangle with t in [near, far] is missed by less than 1e-3 in its smallest
weight.  Comparisons with float64 are made on settled rays only.

Meshes come from tests/test_mesh_cpu.py's numpy marching cubes on its sphere and torus volumes, scaled to [-0.5, 0.5]^3 in fp32.  The
48^3 sphere (7 484 triangles) spans four of the caster's groups of 2 048 triangles."""
import functools

import numpy as np

from test_mesh_cpu import np_marching_cubes, sphere_volume, torus_volume

NEAR, FAR = 0.1, 3.0
SETTLE = 1e-3
EYES = ((0.0, 0.0, -1.2), (0.9, 0.6, -0.7))              # head-on and grazing
GRID = (20, 24)                                          # rows, columns of the pinhole grids
MESHES = {'sphere16': (sphere_volume, 16), 'torus24': (torus_volume, 24), 'sphere32': (sphere_volume, 32), 'sphere48': (sphere_volume, 48)}
N_TRIS = {'sphere16': 716, 'torus24': 1648, 'sphere32': 3212}        # (what the issue counted; sphere48 is this file's choice)
SPHERE_R = 0.3
OUTSIDE = (0.3, -0.2, -1.5)                              # set (a)'s outside point
INSIDE = (0.05, -0.02, 0.08)                             # set (c)'s origin, inside the sphere


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (vertices float32 [V, 3] in [-0.5, 0.5]^3, triangles int64 [T, 3])."""
    make, res = MESHES[name]
    v, t = np_marching_cubes(make(res))
    v = (v / np.float32(res - 1) - np.float32(0.5)).astype(np.float32)
    return v, t


def cell(name):
    return 1.0 / (MESHES[name][1] - 1)


def grid_rays(eye, rows=GRID[0], cols=GRID[1], half=0.38):
    """rows x cols pinhole rays from `eye` toward the origin, the image plane half-width tan = `half`: (o, d) float32 [N, 3], unit d."""
    eye = np.asarray(eye, dtype=np.float64)
    fwd = -eye / np.linalg.norm(eye)
    up0 = np.array([0.31, 1.0, 0.0])                     # (rolled: the head-on pixel rows would run along the marching-cubes grid lines)
    right = np.cross(up0, fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    ys = (np.arange(rows) + 0.5) / rows * 2.0 - 1.0
    xs = (np.arange(cols) + 0.5) / cols * 2.0 - 1.0
    yy, xx = np.meshgrid(ys, xs, indexing='ij')
    d = fwd[None, :] + half * xx.reshape(-1, 1) * right[None, :] + half * rows / cols * yy.reshape(-1, 1) * up[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(eye, d.shape)
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


def edges_of(tris):
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


def through_rays(verts, tris, origin=OUTSIDE):
    """Set (a): from `origin` through every vertex and every edge midpoint -> (o, d) float32, unit d."""
    v = verts.astype(np.float64)
    e = edges_of(tris)
    tgt = np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
    d = tgt - np.asarray(origin, dtype=np.float64)[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(origin, dtype=np.float64), d.shape)
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


def horizon_targets(verts, tris, origin=OUTSIDE):
    """bool, one per ray of `through_rays`: the faces around the target (a vertex's fan, an edge's two faces) do not all face the ray
    the same way -- the target lies on a fold of the surface as seen from `origin`.  There the projected faces overlap instead of
    surrounding the target, and a ray a rounding error beside it may pass outside all of them, whatever the intersection rule."""
    v = verts.astype(np.float64)
    n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    e = edges_of(tris)
    tgt = np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
    d = tgt - np.asarray(origin, dtype=np.float64)[None, :]
    fan = [[] for _ in range(len(v))]
    for f, tri in enumerate(tris):
        for i in tri:
            fan[i].append(f)
    around = [fan[i] for i in range(len(v))] + [sorted(set(fan[a]) & set(fan[b])) for a, b in e]
    out = np.zeros(len(tgt), bool)
    for k, fs in enumerate(around):
        s = n[fs] @ d[k]
        out[k] = not ((s > 0).all() or (s < 0).all())
    return out


def axis_rays():
    """Set (b): rays along +-x, +-y, +-z (two components of d exactly 0) on a 5 x 5 lattice of offsets each -> (o, d) float32."""
    offs = np.linspace(-0.27, 0.27, 5)
    o, d = [], []
    for ax in range(3):
        for sign in (1.0, -1.0):
            for p in offs:
                for q in offs:
                    oo = np.zeros(3)
                    oo[ax] = -1.2 * sign
                    oo[(ax + 1) % 3], oo[(ax + 2) % 3] = p, q + 0.013
                    dd = np.zeros(3)
                    dd[ax] = sign
                    o.append(oo)
                    d.append(dd)
    return np.asarray(o, dtype=np.float32), np.asarray(d, dtype=np.float32)


def inside_rays(n=240, seed=4):
    """Set (c): n unit directions (seeded) from a point inside the sphere: every hit is a back face."""
    d = np.random.RandomState(seed).standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(INSIDE, dtype=np.float64), d.shape)
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


def with_bad_triangles(verts, tris):
    """Set (e): the mesh with a zero-area triangle (two corners the same vertex), one of three collinear points and one with a NaN
    vertex appended; all three lie in front of the surface as seen from EYES[0], where a sound triangle would be hit first."""
    extra = np.array([[0.0, 0.0, -0.45], [0.1, 0.0, -0.45], [0.2, 0.0, -0.45], [np.nan, 0.05, -0.45], [-0.2, -0.2, -0.45], [0.2, 0.3, -0.45]],
                     dtype=np.float32)
    n = len(verts)
    v = np.concatenate([verts, extra])
    t = np.concatenate([tris, np.array([[n + 4, n + 5, n + 5], [n, n + 1, n + 2], [n + 3, n + 4, n + 5]], dtype=np.int64)])
    return v, t


def two_meshes():
    """Set (f): the 16^3 sphere scaled to a half inside the 24^3 torus's hole, tilted views see both -> [(v, t), (v, t)], torus first."""
    vs, ts = mesh('sphere16')
    vt, tt = mesh('torus24')
    return [(vt, tt), ((vs * np.float32(0.5)).astype(np.float32), ts)]


def concat(meshes):
    """-> (vertices, triangles of the concatenation, face offsets)."""
    vs, ts, off, voff = [], [], [0], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + voff)
        voff += len(v)
        off.append(off[-1] + len(t))
    return np.concatenate(vs), np.concatenate(ts), off


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def sound_triangles(verts, tris):
    """bool [T]: the triangles that can be hit -- finite vertices and an fp32 (b - a) x (c - a) of finite, non-zero squared length (the
    kernel's k_mc_prepare, same fp32 operations)."""
    with np.errstate(all='ignore'):
        v = verts.astype(np.float32)
        a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        n2 = (nx * nx + ny * ny) + nz * nz
        fin = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
        return fin & (n2 > 0) & np.isfinite(n2)


def _setup(d, f):
    """Per ray: (kx, ky, kz) int [N, 3], Sx, Sy, Sz in f, and which rays can hit at all."""
    ad = np.abs(d)
    kz = np.argmax(ad, axis=1)                           # (the first of equal maxima)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    n = np.arange(len(d))
    dkz = d[n, kz]
    swap = dkz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all='ignore'):
        Sx, Sy, Sz = d[n, kx] / dkz, d[n, ky] / dkz, f(1.0) / dkz
    return np.stack([kx, ky, kz], 1), Sx.astype(f), Sy.astype(f), Sz.astype(f), dkz != 0


def _pairs(P, o, perm, Sx, Sy, Sz, f):
    """Edge functions, det and t of every (ray, triangle) pair of a chunk: P [T, 3, 3] in f (NaN for unsound triangles), rays [n]."""
    n = len(o)
    idx = np.arange(n)
    Pk = np.transpose(P[:, :, perm], (2, 0, 1, 3))        # [n, T, vertex, (kx, ky, kz)]
    ok = o[idx[:, None], perm]                            # [n, 3]
    with np.errstate(all='ignore'):
        rel = Pk - ok[:, None, None, :]
        kzc = rel[..., 2]
        x = rel[..., 0] - Sx[:, None, None] * kzc
        y = rel[..., 1] - Sy[:, None, None] * kzc
        Ax, Bx, Cx = x[..., 0], x[..., 1], x[..., 2]
        Ay, By, Cy = y[..., 0], y[..., 1], y[..., 2]
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        z = (U == 0) | (V == 0) | (W == 0)
        if z.any():
            g = np.float64
            U = np.where(z, (Cx.astype(g) * By.astype(g) - Cy.astype(g) * Bx.astype(g)).astype(f), U)
            V = np.where(z, (Ax.astype(g) * Cy.astype(g) - Ay.astype(g) * Cx.astype(g)).astype(f), V)
            W = np.where(z, (Bx.astype(g) * Ay.astype(g) - By.astype(g) * Ax.astype(g)).astype(f), W)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        zs = Sz[:, None, None] * kzc
        t = ((U * zs[..., 0] + V * zs[..., 1]) + W * zs[..., 2]) / det
    return U, V, W, det, t, mixed


def rule(verts, tris, o, d, near=NEAR, far=FAR, f=np.float32, chunk=96, detail=False):
    """The rule in the number format f -> dict of hit bool [N], t f [N] (0), face int32 [N] (-1), bary f [N, 2] (0), normal f [N, 3] (0).
    detail=True adds `settled` bool [N] (meaningful for f = float64: the reference)."""
    verts32 = np.asarray(verts, dtype=np.float32)
    tris = np.asarray(tris, dtype=np.int64)
    N, T = len(o), len(tris)
    o, d = np.asarray(o, dtype=np.float32).astype(f), np.asarray(d, dtype=np.float32).astype(f)
    near, far = f(np.float32(near)), f(np.float32(far))
    P = verts32.astype(f)[tris]                           # [T, 3, 3]
    P[~sound_triangles(verts32, tris)] = np.nan
    perm, Sx, Sy, Sz, can = _setup(d, f)
    out = {'hit': np.zeros(N, bool), 't': np.zeros(N, f), 'face': np.full(N, -1, np.int32), 'bary': np.zeros((N, 2), f),
           'normal': np.zeros((N, 3), f)}
    settled = np.zeros(N, bool)
    faces = np.arange(T)
    for s in range(0, N if T else 0, chunk):
        e = min(N, s + chunk)
        U, V, W, det, t, mixed = _pairs(P, o[s:e], perm[s:e], Sx[s:e], Sy[s:e], Sz[s:e], f)
        with np.errstate(all='ignore'):
            inside = (det != 0) & (t >= near) & (t <= far) & can[s:e, None]
            hit = inside & ~mixed
            tt = np.where(hit, t, np.inf)
            best_t = tt.min(1)
            best = np.where(tt == best_t[:, None], faces[None, :], T).min(1)     # the lowest face among the nearest
            any_hit = hit.any(1)
            r = np.arange(e - s)
            b = np.minimum(best, T - 1)
            out['hit'][s:e] = any_hit
            out['t'][s:e] = np.where(any_hit, t[r, b], 0)
            out['face'][s:e] = np.where(any_hit, b, -1)
            out['bary'][s:e, 0] = np.where(any_hit, V[r, b] / det[r, b], 0)
            out['bary'][s:e, 1] = np.where(any_hit, W[r, b] / det[r, b], 0)
            if detail:
                wmin = np.minimum(np.minimum(U / det, V / det), W / det)          # the smallest barycentric weight
                wmin_b = wmin[r, b]
                others = np.where(hit & (faces[None, :] != b[:, None]), t, np.inf).min(1)
                ok_hit = (wmin_b >= SETTLE) & (others > best_t + SETTLE)
                near_miss = (inside & mixed & (wmin > -SETTLE)).any(1)
                settled[s:e] = np.where(any_hit, ok_hit, ~near_miss)
    if T:
        with np.errstate(all='ignore'):
            a, b_, c = (P[np.maximum(out['face'], 0), k] for k in range(3))
            e1, e2 = b_ - a, c - a
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
            nrm = np.stack([nx / ln, ny / ln, nz / ln], 1)
            out['normal'] = np.where(out['hit'][:, None], nrm, 0).astype(f)
    if detail:
        out['settled'] = settled
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _sphere_far_window():
    """Set (d) on the head-on view of the 32^3 sphere: the first surface lies at t in [0.9, 1.2], the second at [1.2, 1.5]."""
    return {'second': (1.2, FAR), 'nothing': (NEAR, 0.85)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: verts, tris, o, d, near, far (and `offsets` for the two-mesh case).  The six grid cases are 'sphere16/0' .. 'sphere48/1'
    (mesh / eye); the extra sets 'through', 'axis', 'inside', 'second', 'nothing', 'bad', 'two/0', 'two/1'; ray counts 'n1', 'n65'."""
    c = {'near': NEAR, 'far': FAR}
    if '/' in name and name.split('/')[0] in MESHES:
        m, eye = name.split('/')
        c['verts'], c['tris'] = mesh(m)
        c['o'], c['d'] = grid_rays(EYES[int(eye)])
    elif name == 'through':
        c['verts'], c['tris'] = mesh('sphere16')
        c['o'], c['d'] = through_rays(*mesh('sphere16'))
    elif name == 'axis':
        c['verts'], c['tris'] = mesh('sphere16')
        c['o'], c['d'] = axis_rays()
    elif name == 'inside':
        c['verts'], c['tris'] = mesh('sphere16')
        c['o'], c['d'] = inside_rays()
    elif name in ('second', 'nothing'):
        c['verts'], c['tris'] = mesh('sphere32')
        c['o'], c['d'] = grid_rays(EYES[0])
        c['near'], c['far'] = _sphere_far_window()[name]
    elif name == 'bad':
        c['verts'], c['tris'] = with_bad_triangles(*mesh('sphere16'))
        c['o'], c['d'] = grid_rays(EYES[0])
    elif name.startswith('two/'):
        c['meshes'] = two_meshes()
        c['verts'], c['tris'], c['offsets'] = concat(c['meshes'])
        c['o'], c['d'] = grid_rays(((0.0, 0.9, -0.9), (0.9, 0.6, -0.7))[int(name[4:])])
    elif name in ('n1', 'n65'):
        c['verts'], c['tris'] = mesh('torus24')
        o, d = grid_rays(EYES[1])
        n = int(name[1:])
        c['o'], c['d'] = o[200:200 + n].copy(), d[200:200 + n].copy()
    else:
        raise KeyError(name)
    return c


GRID_CASES = tuple('%s/%d' % (m, e) for m in MESHES for e in (0, 1))
CAPPED = GRID_CASES + ('axis', 'inside', 'second', 'nothing', 'bad', 'two/0', 'two/1')     # at most 2 % of their rays unsettled
ALL_CASES = CAPPED + ('through', 'n1', 'n65')


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return rule(c['verts'], c['tris'], c['o'], c['d'], c['near'], c['far'], np.float64, detail=True)


@functools.lru_cache(maxsize=None)
def restatement(name):
    c = case(name)
    return rule(c['verts'], c['tris'], c['o'], c['d'], c['near'], c['far'], np.float32)


def mesh_of(face, offsets):
    """int32 [N]: the mesh of every face index (-1 stays -1)."""
    m = np.searchsorted(np.asarray(offsets[1:]), face, side='right').astype(np.int32)
    return np.where(face >= 0, m, -1).astype(np.int32)


def ulps(a, b):
    """The distance of two float32 arrays in units in the last place (0 for equal bits and for +0 / -0)."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)
