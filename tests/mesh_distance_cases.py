"""Cases of the mesh distance queries (ho-nerf_amd/csrc/hn_meshdist.hip, honerf_amd.mesh_distance) and the contract of DESIGN.md 3.27 in
numpy, in float64.  A plain module, in the manner of meshcast_cases: tests/test_mesh_distance_cpu.py (is the restatement right on
analytic shapes?) and tests/test_gpu_mesh_distance.py (is the device the restatement?) both import it.

  np_closest        the closest point on a mesh per query: Ericson's region tests (Real-Time Collision Detection 5.1.5) per pair, the
                    winner the smallest (d^2, face) -> (distance, face, point)
  np_tri_closest    the same against ONE given triangle per query
  mix64, draws      the sampler's integer hash: three successive splitmix64 outputs started at (seed << 32) | i, the top 24 bits of each
                    as (k + 0.5) / 2^24
  np_sample         the sampler: fp64 areas from the fp32 vertices, inclusive cumulative areas, sample i at (i + r0) / n * A in the first
                    triangle whose cumulative area exceeds it, the point (1 - sqrt r1) a + sqrt r1 (1 - r2) b + sqrt r1 r2 c
  np_surface_metrics  the metrics from given samples
"""
import functools

import numpy as np

from meshcast_cases import edges_of, mesh as mc_mesh
from meshcc_cases import sphere_mesh

T_EDGES = (1, 63, 64, 65, 2047, 2048, 2049, 4097)        # the block (64) and group (2048) edges
P_EDGES = (1, 63, 64, 65, 255, 256, 257, 1000)
MASK64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def uv_sphere(r, n_lat=12, n_lon=16, center=(0.0, 0.0, 0.0)):
    """A latitude / longitude sphere, every vertex exactly (in float64, then rounded to fp32) at radius r: (vertices float32, triangles)."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * np.pi * j / n_lon
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    t = []
    for j in range(n_lon):
        t.append((0, ring(1, j), ring(1, j + 1)))
        t.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            t.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            t.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    v = np.asarray(v, np.float64) * r + np.asarray(center, np.float64)[None]
    return v.astype(np.float32), np.asarray(t, np.int64)


def sagitta(verts, tris, r, center=(0.0, 0.0, 0.0)):
    """How far the facets of a mesh inscribed in the sphere (r, center) lie inside it at most: r minus the smallest distance from the
    centre to a facet's plane (float64)."""
    v = verts.astype(np.float64) - np.asarray(center, np.float64)[None]
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(r - np.abs((n * a).sum(1)).min())


@functools.lru_cache(maxsize=None)
def mesh_T(T):
    """A mesh of exactly T triangles: the first T of a marching-cubes torus (24^3: 1 648 triangles) or sphere (48^3: 7 484)."""
    v, t = mc_mesh('torus24' if T <= 1648 else 'sphere48')
    assert len(t) >= T
    return v, np.ascontiguousarray(t[:T])


def doubled(verts, tris, copies_first=False):
    """Every triangle listed twice: i and T + i identical.  copies_first: the copies in REVERSED order in front of the originals, so
    that triangle i's copy is T - 1 - i and the original T + i."""
    return verts, np.concatenate([tris[::-1], tris] if copies_first else [tris, tris])


def centroids(verts, tris):
    v = verts.astype(np.float64)
    return (v[tris[:, 0]] + v[tris[:, 1]] + v[tris[:, 2]]) / 3.0


def unit_normals(verts, tris):
    v = verts.astype(np.float64)
    n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def query_set(verts, tris, kind, n, seed=0):
    """n query points (float32 [n, 3]) of one of the issue's sets, cycled or cut to n:
    'surface'  the mesh's own vertices, edge midpoints and centroids;   'near'  +-1 mm and +-5 cm along face normals from centroids;
    'far'      points 100 m away;   'centre'  the mean of the vertices and points 1e-4 around it;   'random'  uniform in 1.5 x the bounds."""
    v = verts.astype(np.float64)
    used = np.unique(tris)
    rs = np.random.RandomState(seed)
    if kind == 'surface':
        e = edges_of(tris)
        q = np.concatenate([v[used], 0.5 * (v[e[:, 0]] + v[e[:, 1]]), centroids(verts, tris)])
        q = q[rs.permutation(len(q))]
    elif kind == 'near':
        c, nn = centroids(verts, tris), unit_normals(verts, tris)
        q = np.concatenate([c + s * nn for s in (0.001, -0.001, 0.05, -0.05)])
        q = q[rs.permutation(len(q))]
    elif kind == 'far':
        d = rs.standard_normal((n, 3))
        q = 100.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    elif kind == 'centre':
        c = v[used].mean(0)
        q = np.concatenate([c[None], c[None] + 1e-4 * rs.standard_normal((max(n - 1, 1), 3))])
    elif kind == 'random':
        lo, hi = v[used].min(0), v[used].max(0)
        mid, half = 0.5 * (lo + hi), 0.75 * (hi - lo) + 1e-3
        q = mid[None] + half[None] * rs.uniform(-1.0, 1.0, (n, 3))
    else:
        raise KeyError(kind)
    q = np.concatenate([q] * (n // len(q) + 1))[:n]
    return np.ascontiguousarray(q, dtype=np.float32)


QUERY_KINDS = ('surface', 'near', 'far', 'centre', 'random')


# ---- the closest point ---------------------------------------------------------------------------------------------------------------
def _dot(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def _segment(p, a, b):
    ab = b - a
    den = _dot(ab, ab)
    with np.errstate(all='ignore'):
        s = np.where(den > 0, _dot(p - a, ab) / np.where(den > 0, den, 1.0), 0.0)
    return a + np.clip(s, 0.0, 1.0)[..., None] * ab


def closest_pairs(p, a, b, c):
    """Closest point on triangle (a, b, c) to p, broadcasting ([..., 3] each, float64) -> (q [..., 3], d2 [...]).  Ericson 5.1.5: the
    face region by default, the edge and vertex regions override; a pair that yields no finite point that way (a triangle without
    area) takes the nearest of its three edges' closest points."""
    with np.errstate(all='ignore'):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = va + vb + vc
        v, w = vb / den, vc / den
        e43, e56 = d4 - d3, d5 - d6
        m = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        wbc = e43 / (e43 + e56)
        v, w = np.where(m, 1.0 - wbc, v), np.where(m, wbc, w)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = np.where(m, 0.0, v), np.where(m, d2 / (d2 - d6), w)
        m = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(m, 0.0, v), np.where(m, 1.0, w)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = np.where(m, d1 / (d1 - d3), v), np.where(m, 0.0, w)
        m = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(m, 1.0, v), np.where(m, 0.0, w)
        m = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(m, 0.0, v), np.where(m, 0.0, w)
        q = a + v[..., None] * ab + w[..., None] * ac
        bad = ~(np.isfinite(q).all(-1) & (den > 0))
        if bad.any():                                     # no area: a segment or a point
            shape = np.broadcast(p, a).shape
            pb, ab_, bb, cb = (np.broadcast_to(x, shape)[bad] for x in (p, a, b, c))
            cand = np.stack([_segment(pb, ab_, bb), _segment(pb, bb, cb), _segment(pb, cb, ab_)])
            dd = ((cand - pb[None]) ** 2).sum(-1)
            dd = np.where(np.isnan(dd), np.inf, dd)
            pick = dd.argmin(0)
            q = np.array(np.broadcast_to(q, shape))
            q[bad] = cand[pick, np.arange(len(pick))]
        d2_ = ((q - p) ** 2).sum(-1)
        fin = np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & np.isfinite(c).all(-1)
        d2_ = np.where(fin, d2_, np.inf)                  # a triangle with a coordinate that is not finite never wins
    return q, d2_


def np_closest(verts, tris, pts, pairs=1 << 18):
    """-> (distance float64 [P] (inf without a finite triangle), face int64 [P] (-1), point float64 [P, 3] (0)): the smallest (d^2, face)."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    P, T = len(p), len(t)
    dist, face, point = np.full(P, np.inf), np.full(P, -1, np.int64), np.zeros((P, 3))
    if T == 0 or P == 0:
        return dist, face, point
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    step = max(1, pairs // T)
    for s in range(0, P, step):
        q, d2 = closest_pairs(p[s:s + step, None, :], a, b, c)
        d2 = np.where(np.isnan(d2), np.inf, d2)
        f = d2.argmin(1)                                  # (the first of equal minima: the smallest face)
        r = np.arange(len(f))
        ok = np.isfinite(d2[r, f])
        dist[s:s + step] = np.where(ok, np.sqrt(d2[r, f]), np.inf)
        face[s:s + step] = np.where(ok, f, -1)
        point[s:s + step] = np.where(ok[:, None], q[r, f], 0.0)
    return dist, face, point


def np_tri_closest(verts, tris, pts, face):
    """Each query against its own triangle `face` -> (distance float64 [P], point float64 [P, 3])."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)[np.asarray(face, np.int64)]
    p = np.asarray(pts, np.float64)
    q, d2 = closest_pairs(p, v[t[:, 0]], v[t[:, 1]], v[t[:, 2]])
    return np.sqrt(d2), q


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def mix64(z):
    """splitmix64's output function on Python integers."""
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draws24(seed, i):
    """The three 24-bit integers of sample i."""
    ctr = ((seed << 32) | i) & MASK64
    return tuple(mix64(ctr + (j + 1) * GAMMA) >> 40 for j in range(3))


def draws(seed, n):
    """-> float64 [n, 3]: (r0, r1, r2) of samples 0 .. n-1, vectorised in uint64 (wrapping products)."""
    with np.errstate(over='ignore'):
        ctr = (np.uint64(seed) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        out = []
        for j in range(3):
            z = ctr + np.uint64(((j + 1) * GAMMA) & MASK64)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            out.append(((z >> np.uint64(40)).astype(np.float64) + 0.5) / 16777216.0)
    return np.stack(out, 1)


def np_face_areas(verts, tris):
    """-> (area float64 [T], unit normal float64 [T, 3]): |(b - a) x (c - a)| / 2 from the fp32 vertices; 0 and 0 where that is 0 or
    not finite."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    t = np.asarray(tris, np.int64)
    with np.errstate(all='ignore'):
        e1, e2 = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        has = (ln > 0) & np.isfinite(ln)
        safe = np.where(has, ln, 1.0)
        nrm = np.where(has[:, None], np.stack([nx / safe, ny / safe, nz / safe], 1), 0.0)
    return np.where(has, 0.5 * ln, 0.0), nrm


def np_sample(verts, tris, n, seed=0, detail=False):
    """-> (points float64 [n, 3], face int64 [n], normal float64 [n, 3]); detail=True adds (u float64 [n], cum float64 [T])."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    t = np.asarray(tris, np.int64)
    area, nrm = np_face_areas(verts, tris)
    cum = np.cumsum(area)
    r = draws(seed, n)
    u = (np.arange(n, dtype=np.float64) + r[:, 0]) / float(n) * cum[-1]
    f = np.minimum(np.searchsorted(cum, u, side='right'), len(t) - 1)
    s = np.sqrt(r[:, 1])
    w0, w1, w2 = 1.0 - s, s * (1.0 - r[:, 2]), s * r[:, 2]
    pts = (w0[:, None] * v[t[f, 0]] + w1[:, None] * v[t[f, 1]]) + w2[:, None] * v[t[f, 2]]
    return (pts, f, nrm[f], u, cum) if detail else (pts, f, nrm[f])


def knot_gap(verts, tris, n, seed=0, rel=1e-9):
    """bool [n]: the samples whose position lies within rel * A_total of a cumulative-area knot (there a cumulative sum made in another
    order may pick the neighbouring triangle)."""
    _, _, _, u, cum = np_sample(verts, tris, n, seed, detail=True)
    k = np.searchsorted(cum, u)
    lo, hi = cum[np.maximum(k - 1, 0)], cum[np.minimum(k, len(cum) - 1)]
    return np.minimum(np.abs(u - lo), np.abs(u - hi)) < rel * cum[-1]


# ---- the metrics ---------------------------------------------------------------------------------------------------------------------
def np_surface_metrics(pred, gt, pred_points, pred_normals, gt_points, gt_normals, taus=(0.005, 0.010), detail=False, faces=None):
    """surface_metrics from given samples, in float64.  faces: (the nearest face of gt per pred sample, of pred per gt sample) to take
    the normals from, for a caller whose query settled ties between equally near faces its own way."""
    acc, fa, _ = np_closest(gt[0], gt[1], pred_points)
    comp, fc, _ = np_closest(pred[0], pred[1], gt_points)
    if faces is not None:
        fa, fc = np.asarray(faces[0], np.int64), np.asarray(faces[1], np.int64)
    nca = np.abs((np.asarray(pred_normals, np.float64) * np_face_areas(*gt)[1][fa]).sum(1)).mean()
    ncc = np.abs((np.asarray(gt_normals, np.float64) * np_face_areas(*pred)[1][fc]).sum(1)).mean()
    out = dict(chamfer_l1=(acc.mean() + comp.mean()) / 2.0, chamfer_l2=(acc ** 2).mean() + (comp ** 2).mean(), hausdorff=max(acc.max(), comp.max()),
               accuracy=acc.mean(), completeness=comp.mean(), normal_consistency=(nca + ncc) / 2.0, n=len(acc),
               pred_area=np_face_areas(*pred)[0].sum(), gt_area=np_face_areas(*gt)[0].sum())
    for t in taus:
        p, r = float((acc <= t).mean()), float((comp <= t).mean())
        out['precision@%g' % t], out['recall@%g' % t] = p, r
        out['fscore@%g' % t] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return (out, acc, comp) if detail else out


# the sampler cases of the GPU tests: (mesh, n, seed), each chosen so that no sample lies in the knot gap (test_mesh_distance_cpu.py)
def sampler_mesh(name):
    if name == 'one':
        return np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.1], [0.0, 0.2, 0.0]], np.float32), np.array([[0, 1, 2]], np.int64)
    if name == 'torus24':
        return mc_mesh('torus24')
    if name == 'sphere16+flat':                          # a zero-area triangle in the middle of the list: never drawn
        v, t = mc_mesh('sphere16')
        return v, np.concatenate([t[:300], np.array([[5, 5, 9]], np.int64), t[300:]])
    if name == 'spheres':
        return sphere_mesh((0.0, 0.0, 0.0), 0.05, 16)
    raise KeyError(name)


SAMPLER_CASES = (('one', 1, 0), ('one', 1000, 3), ('torus24', 1, 0), ('torus24', 1000, 0), ('torus24', 4099, 7), ('sphere16+flat', 777, 1),
                 ('spheres', 2000, 0), ('spheres', 2000, 1))
