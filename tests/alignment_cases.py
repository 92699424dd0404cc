"""Cases of the alignment kernels (ho-nerf_amd/csrc/hn_align.hip, honerf_amd.alignment) and the contract of DESIGN.md 3.28 in numpy, in
float64.  A plain module, in the manner of mesh_distance_cases: tests/test_alignment_cpu.py (do two independent formulations agree, do
they recover what was planted, is the ICP scene fair?) and tests/test_gpu_alignment.py (is the device the restatement?) import it.

  umeyama_svd       the weighted similarity / rigid Procrustes by numpy's SVD of the cross-covariance with the determinant correction
                    (Umeyama, PAMI 13, 1991)
  horn_quaternion   the same transform from the top eigenvector (numpy.linalg.eigh) of Horn's symmetric 4 x 4 matrix (JOSA A 4, 1987)
  np_moments        the 18 moments per frame and, per entry, the sum of the absolute terms (what a summation bound is made of)
  np_apply          x -> float32(s ((R0 x + R1 y) + R2 z) + t), the device's order of operations
  residual          sum w |s R a + t - b|^2
  cases             the seeded inputs, fp32-exact coordinates
  blob_mesh, icp_scene, icp_reference   the ICP scene and the float64 ICP over a brute-force closest point
"""
import functools

import numpy as np

from honerf_amd.alignment import CHUNK
from mesh_distance_cases import np_closest, np_sample, uv_sphere

N_EDGES = (1, 2, 3, 4, 21, 778, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
F_EDGES = (1, 2, 65)
EPS64 = 2.0 ** -52
FLOOR = 1e-13
# What test_alignment_cpu.py measured between the two float64 formulations per kind (the largest |difference| over the kind's cases and
# frames): R (entries), s, t (metres), and the residual relative to sum w |b - cb|^2.  That test asserts the spread it measures stays
# within these; the device is held to 8 x these, and to FLOOR at least (tests/test_gpu_alignment.py).  Rounded up to one digit.
SPREAD = {
    'similarity': dict(R=7e-15, s=2e-15, t=9e-15, res=1e-20),
    'rigid': dict(R=1e-15, s=0.0, t=7e-16, res=2e-21),
    'identity': dict(R=4e-15, s=5e-16, t=3e-15, res=1e-29),
    'mirror': dict(R=4e-14, s=7e-16, t=6e-15, res=1e-15),
    'planar': dict(R=2e-12, s=2e-15, t=3e-12, res=2e-20),          # (N = 4 on a lattice: the SVD's third singular vector is free in sign)
    'wzeros': dict(R=2e-15, s=9e-16, t=3e-15, res=2e-21),
    'wspan': dict(R=2e-15, s=2e-15, t=2e-15, res=6e-21),
    'noise': dict(R=3e-15, s=2e-15, t=4e-15, res=5e-17),
}


# ---- the two formulations ------------------------------------------------------------------------------------------------------------
def _centred(a, b, w):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.ones(len(a)) if w is None else np.asarray(w, np.float64)
    W = w.sum()
    ca, cb = (w[:, None] * a).sum(0) / W, (w[:, None] * b).sum(0) / W
    return a - ca, b - cb, w, ca, cb


def umeyama_svd(a, b, w=None, scale=True):
    """a, b [N, 3], w [N] or None -> (R [3, 3], s, t [3]) minimising sum w |s R a + t - b|^2 over proper rotations."""
    da, db, w, ca, cb = _centred(a, b, w)
    H = (w[:, None, None] * db[:, :, None] * da[:, None, :]).sum(0)            # sum w db da^T
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt)) or 1.0])
    R = U @ D @ Vt
    va = (w * (da * da).sum(1)).sum()
    s = float((S * np.diag(D)).sum() / va) if scale and va > 0 else 1.0
    return R, s, cb - s * R @ ca


def horn_quaternion(a, b, w=None, scale=True):
    """The same, from the eigenvector of the largest eigenvalue of Horn's 4 x 4 matrix; proper by construction."""
    da, db, w, ca, cb = _centred(a, b, w)
    S = (w[:, None, None] * da[:, :, None] * db[:, None, :]).sum(0)            # S[p, q] = sum w da_p db_q
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    lam, vec = np.linalg.eigh(N)
    q = vec[:, -1] / np.linalg.norm(vec[:, -1])
    R = quat_matrix(q)
    va = (w * (da * da).sum(1)).sum()
    s = float(max((R * S.T).sum(), 0.0) / va) if scale and va > 0 else 1.0
    return R, s, cb - s * R @ ca


def quat_matrix(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` (radians) about `axis`, float64."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def residual(a, b, w, R, s, t):
    """sum w |s R a + t - b|^2 in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.ones(len(a)) if w is None else np.asarray(w, np.float64)
    d = s * (a @ np.asarray(R, np.float64).T) + np.asarray(t, np.float64) - b
    return float((w * (d * d).sum(1)).sum())


def np_apply(p, R, s, t):
    """float32(s ((R0 x + R1 y) + R2 z) + t) row by row: hn_align_apply's order of operations, no fused multiply-add."""
    p = np.asarray(p, np.float32).astype(np.float64)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    cols = [float(s) * ((R[d, 0] * x + R[d, 1] * y) + R[d, 2] * z) + t[d] for d in range(3)]
    return np.stack(cols, 1).astype(np.float32)


def np_compose(second, first):
    (R2, s2, t2), (R1, s1, t1) = second, first
    return R2 @ R1, s2 * s1, s2 * (R2 @ t1) + t2


def np_moments(a, b, w=None, ca=None, cb=None):
    """-> (moments float64 [18], abs float64 [18]): W, ca, cb, H (row-major, sum w (b - cb)(a - ca)^T), va, vb of one frame from the fp32
    clouds, and per entry the sum of the absolute values of the terms that were added (for ca and cb: of w a / W).  ca, cb: the
    centroids to centre on (the device's own, so that the second moments are sums of the same terms); None: this function's."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    w = np.ones(len(a)) if w is None else np.asarray(w, np.float32).astype(np.float64)
    W = w.sum()
    m, ab = np.zeros(18), np.zeros(18)
    m[0] = ab[0] = W
    if W > 0:
        m[1:4], m[4:7] = (w[:, None] * a).sum(0) / W, (w[:, None] * b).sum(0) / W
        ab[1:4], ab[4:7] = np.abs(w[:, None] * a).sum(0) / W, np.abs(w[:, None] * b).sum(0) / W
    da = a - (m[1:4] if ca is None else np.asarray(ca, np.float64))
    db = b - (m[4:7] if cb is None else np.asarray(cb, np.float64))
    terms = (w[:, None] * db)[:, :, None] * da[:, None, :]
    m[7:16], ab[7:16] = terms.sum(0).reshape(-1), np.abs(terms).sum(0).reshape(-1)
    ta = w * ((da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2])
    tb = w * ((db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + db[:, 2] * db[:, 2])
    m[16], m[17], ab[16], ab[17] = ta.sum(), tb.sum(), ta.sum(), tb.sum()
    return m, ab


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
ANGLES = (0.0, 5.0, 90.0, 179.9)
SCALES = (0.5, 2.0)
RANK3_KINDS = ('similarity', 'rigid', 'identity', 'mirror', 'planar', 'wzeros', 'wspan', 'noise')


def _cloud(rs, n, size=0.05, centre=0.8):
    """n points within `size` of a centre `centre` metres out, fp32."""
    c = rs.standard_normal(3)
    c = centre * c / np.linalg.norm(c)
    return (c[None] + size * rs.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)


def _planted(rs, k, with_scale=True):
    axis = rs.standard_normal(3)
    R = rotation(axis, np.deg2rad(ANGLES[k % 4]))
    s = SCALES[(k // 4) % 2] if with_scale else 1.0
    t = rs.standard_normal(3)
    return R, s, 0.8 * t / np.linalg.norm(t)


def _image(a, R, s, t):
    """The similarity image of the fp32 cloud a, evaluated in float64 and rounded once."""
    return (s * (a.astype(np.float64) @ R.T) + t).astype(np.float32)


def _lattice(rs, n, dims):
    """n points p0 + i u (+ j v): every coordinate a small dyadic rational, exact in fp32, exactly collinear (dims 1) or coplanar (2)."""
    p0 = np.array([0.75, -0.5, 0.25])
    u, v = np.array([2.0, 3.0, -4.0]) / 1024.0, np.array([-3.0, 1.0, 2.0]) / 1024.0
    i = rs.permutation(max(n, 32))[:n] - 8
    j = rs.randint(-8, 9, n) if dims == 2 else np.zeros(n, np.int64)
    if dims == 2 and n >= 3:
        i[:3], j[:3] = (0, 5, 1), (0, 1, 6)                                 # (never all on one line)
    a = p0[None] + i[:, None] * u[None] + j[:, None] * v[None]
    assert (a.astype(np.float32).astype(np.float64) == a).all()
    return a.astype(np.float32)


def _case(kind, F, N, seed):
    rs = np.random.RandomState(seed)
    A, B, Wt, P = [], [], [], []
    rank, scale, weighted = 3, kind != 'rigid', kind in ('wzeros', 'wone', 'wspan')
    for f in range(F):
        R, s, t = _planted(rs, f + seed, with_scale=scale)
        w = None
        if kind in ('similarity', 'rigid', 'wzeros', 'wspan', 'wone'):
            a = _cloud(rs, N)
            b = _image(a, R, s, t)
        elif kind == 'identity':
            a = _cloud(rs, N)
            b, (R, s, t) = a.copy(), (np.eye(3), 1.0, np.zeros(3))
        elif kind == 'mirror':                                              # no proper rotation reaches b: nothing is planted
            a = _cloud(rs, N)
            b = _image((a.astype(np.float64) * np.array([1.0, 1.0, -1.0])).astype(np.float32), R, s, t)
        elif kind == 'planar':
            a = _lattice(rs, N, 2)
            b = _image(a, R, s, t)
        elif kind == 'collinear':
            a = _lattice(rs, N, 1)
            b = _image(a, R, s, t)
        elif kind == 'coincident':
            a = np.repeat(_cloud(rs, 1), N, 0)
            b = _cloud(rs, N)
        elif kind == 'noise':                                               # 1 mm on a 5 cm cloud
            a = _cloud(rs, N)
            b = (_image(a, R, s, t).astype(np.float64) + 0.001 * rs.standard_normal((N, 3))).astype(np.float32)
        else:
            raise KeyError(kind)
        if kind == 'wzeros':
            w = rs.uniform(0.25, 1.0, N).astype(np.float32)
            w[rs.permutation(N)[:N // 3]] = 0.0
            b[w == 0] += np.float32(0.3)                                    # what carries no weight must not matter
        elif kind == 'wspan':
            w = (10.0 ** rs.uniform(-6.0, 0.0, N)).astype(np.float32)
        elif kind == 'wone':
            w = np.zeros(N, np.float32)
            w[rs.randint(N)] = 1.0
        A.append(a), B.append(b), Wt.append(w), P.append((R, s, t))
    if kind == 'collinear' or (kind in ('similarity', 'rigid') and N == 2):
        rank = 1
    if kind in ('coincident', 'wone') or N == 1:
        rank = 0
    planted = None if kind in ('mirror', 'coincident') else (np.stack([p[0] for p in P]), np.array([p[1] for p in P]), np.stack([p[2] for p in P]))
    return dict(name='%s F=%d N=%d' % (kind, F, N), kind=kind, a=np.stack(A), b=np.stack(B), w=np.stack(Wt) if weighted else None, scale=scale,
                planted=planted, exact=kind not in ('noise',), rank=rank)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, built once: a dict each of name, kind, a, b fp32 [F, N, 3], w fp32 [F, N] or None, scale, planted (R, s, t per frame,
    or None), rank (the expected one of every frame)."""
    out, seed = [], 0
    for N in N_EDGES:                                                       # the N edges: two frames each, N = 1 and 2 degenerate
        out.append(_case('similarity', 2, N, seed))
        seed += 1
    for F in F_EDGES:                                                       # the F edges: short clouds and a cloud of more than one chunk
        for N in (21, CHUNK + 1):
            out.append(_case('similarity', F, N, seed))
            seed += 1
    for kind in ('rigid', 'identity', 'mirror', 'planar', 'collinear', 'coincident', 'wzeros', 'wone', 'wspan', 'noise'):
        for N in (4, 21, 778, CHUNK + 1) if kind in ('planar', 'collinear') else (21, 778, CHUNK + 1):
            out.append(_case(kind, 8, N, seed))
            seed += 1
    return tuple(out)


def rank3(case):
    return case['rank'] == 3


# ---- ICP -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_mesh():
    """A closed mesh without any symmetry, 168 faces, 4 to 12 cm across, half a metre from the origin: a latitude / longitude sphere whose
    radius varies with direction, stretched along x and flattened along z: (vertices float32 [86, 3], triangles int64 [168, 3])."""
    v, t = uv_sphere(1.0, n_lat=8, n_lon=12)
    d = v.astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r = 0.04 * (1.0 + 0.30 * x + 0.20 * y * y - 0.25 * y * z + 0.15 * x * z * z + 0.20 * z * z * z + 0.10 * x * y)
    return (d * r[:, None] * np.array([1.4, 0.8, 0.45]) + np.array([0.1, -0.2, 0.5])).astype(np.float32), t


MOTIONS = {'small': (5.0, 0.005), 'large': (15.0, 0.02)}                     # degrees, metres


def icp_scene(motion, n=2000, outliers=0.0):
    """-> (mesh, points float32 [n (+ outliers), 3], planted (R, s, t)): n stratified surface samples of the blob (the float64 sampler
    of mesh_distance_cases), moved by the INVERSE of the planted rigid motion about the blob's centre, so that the planted motion
    brings them back onto the surface; `outliers` x n more points 1 m away, appended."""
    mesh = blob_mesh()
    deg, shift = MOTIONS[motion]
    rs = np.random.RandomState(int(deg))
    p = np_sample(mesh[0], mesh[1], n, seed=5)[0]
    axis, dirn = rs.standard_normal(3), rs.standard_normal(3)
    R = rotation(axis, np.deg2rad(deg))
    c = mesh[0].astype(np.float64).mean(0)
    t = c - R @ c + shift * dirn / np.linalg.norm(dirn)                       # x -> R (x - c) + c + shift
    q = (p - t) @ R                                                          # R^T (p - t)
    if outliers:
        far = rs.standard_normal((int(round(outliers * n)), 3))
        q = np.concatenate([q, c[None] + 1.0 * far / np.linalg.norm(far, axis=1, keepdims=True)])
    return mesh, q.astype(np.float32), (R, 1.0, t)


def icp_reference(points, mesh, iters, scale=False, max_distance=None):
    """alignment.icp in float64 over a brute-force closest point -> dict(R, s, t, rms float64 [iters + 1], last_step: (dR, ds, dt), the
    largest change the last iteration still made to the transform)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    acc = (np.eye(3), 1.0, np.zeros(3))
    rms, last = [], None

    def query(moved):
        d, _, q = np_closest(mesh[0], mesh[1], moved)
        w = np.ones(len(d)) if max_distance is None else (d <= max_distance).astype(np.float64)
        return d, q, w

    for _ in range(iters):
        moved = acc[1] * (p @ acc[0].T) + acc[2]
        d, q, w = query(moved)
        rms.append(np.sqrt((w * d * d).sum() / w.sum()))
        new = np_compose(umeyama_svd(moved, q, w, scale), acc)
        last = (np.abs(new[0] - acc[0]).max(), abs(new[1] - acc[1]), np.abs(new[2] - acc[2]).max())
        acc = new
    d, _, w = query(acc[1] * (p @ acc[0].T) + acc[2])
    rms.append(np.sqrt((w * d * d).sum() / w.sum()))
    return dict(R=acc[0], s=acc[1], t=acc[2], rms=np.asarray(rms), last_step=last)


ICP_ITERS = 30


@functools.lru_cache(maxsize=None)
def icp_cases(motion, outliers=0.0):
    """The scene and its float64 reference, computed once per process and shared."""
    mesh, pts, planted = icp_scene(motion, outliers=outliers)
    ref = icp_reference(pts, mesh, ICP_ITERS, max_distance=0.1 if outliers else None)
    return mesh, pts, planted, ref
