"""Rigid and similarity alignment on the device (hn_align.hip): Procrustes of paired clouds and point-to-surface ICP against a mesh.

DESIGN.md 3.28 is the contract; tests/alignment_cases.py restates it in float64 numpy.  A transform is x -> s R x + t with R a proper
rotation (det +1), float64 on the device.  `procrustes` is the closed form (Kabsch / Umeyama, here in Horn's quaternion form): the
weighted moments of the two clouds in a summation tree fixed by the point count, then the best rotation from a 4 x 4 eigenproblem
that is linear in the cross-covariance.  `icp` puts `mesh_distance.MeshIndex.closest` and that solver in a loop of fixed length that
never waits for the device.

Arguments are numpy arrays or torch tensors, on either device, float32 or float64 (`pose_metrics`' conventions); results are device
tensors.  There are no gradients.
"""
import torch

from . import lib as _lib
from .interaction import _check
from .pose_metrics import _clouds, _paired, _tensor

CHUNK = 1024              # the points one wave sums (hn_align_chunk): the summation tree of the moments changes shape at its multiples
HOST_COPIES = 0           # device-to-host copies this module has made (every one goes through _to_host): `icp` makes one, at its end


def _to_host(x):
    global HOST_COPIES
    HOST_COPIES += 1
    return x.cpu()


# ---- private passes on checked device tensors ------------------------------------------------------------------------------------------
def _moments(a, b, w):
    """a, b fp32 [F, N, 3] contiguous, w fp32 [F, N] contiguous or None -> fp64 [F, 18] (hn_align_moments)."""
    F, N = a.shape[0], a.shape[1]
    L = _lib.load()
    with torch.cuda.device(a.device):
        need = int(L.hn_align_workspace_bytes(F, N))
        if need == 0:
            raise ValueError('alignment: %d frames x %d points is beyond what one call takes (2^31 - %d)' % (F, N, CHUNK))
        ws = torch.empty(need, dtype=torch.uint8, device=a.device)
        m = torch.empty(F, 18, dtype=torch.float64, device=a.device)
        _check(L.hn_align_moments(_lib.ptr(a), _lib.ptr(b), _lib.ptr(w), F, N, _lib.ptr(m), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               'alignment moments')
    return m


def _solve(m, scale):
    """moments fp64 [F, 18] -> (R [F, 3, 3], s [F], t [F, 3] fp64, rank [F] int32) (hn_align_solve)."""
    F, dev = m.shape[0], m.device
    R = torch.empty(F, 3, 3, dtype=torch.float64, device=dev)
    s = torch.empty(F, dtype=torch.float64, device=dev)
    t = torch.empty(F, 3, dtype=torch.float64, device=dev)
    rank = torch.empty(F, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_lib.load().hn_align_solve(_lib.ptr(m), F, 1 if scale else 0, _lib.ptr(R), _lib.ptr(s), _lib.ptr(t), _lib.ptr(rank),
                                          _lib.stream_ptr()), 'alignment solve')
    return R, s, t, rank


def _apply(p, R, s, t):
    """p fp32 [F, N, 3], (R, s, t) fp64 for F frames or for one -> fp32 [F, N, 3] (hn_align_apply)."""
    F, N = p.shape[0], p.shape[1]
    out = torch.empty_like(p)
    with torch.cuda.device(p.device):
        _check(_lib.load().hn_align_apply(_lib.ptr(p), F, N, _lib.ptr(R), _lib.ptr(s), _lib.ptr(t), R.shape[0], _lib.ptr(out), _lib.stream_ptr()),
               'alignment apply')
    return out


def _compose(second, first):
    """second o first, both (R, s, t) fp64 of F frames -> (R, s, t) (hn_align_compose)."""
    (R2, s2, t2), (R1, s1, t1) = second, first
    F = R1.shape[0]
    R, s, t = torch.empty_like(R1), torch.empty_like(s1), torch.empty_like(t1)
    with torch.cuda.device(R1.device):
        _check(_lib.load().hn_align_compose(_lib.ptr(R2), _lib.ptr(s2), _lib.ptr(t2), _lib.ptr(R1), _lib.ptr(s1), _lib.ptr(t1), F, _lib.ptr(R),
                                            _lib.ptr(s), _lib.ptr(t), _lib.stream_ptr()), 'alignment compose')
    return R, s, t


def _rms(d, w):
    """d fp32 [F, N] distances, w fp32 [F, N] or None -> fp64 [F]: sqrt(sum w d^2 / sum w) (0 without weight)."""
    d2 = d.double() ** 2
    if w is None:
        return d2.mean(1).sqrt()
    W = w.double().sum(1)
    return torch.where(W > 0, (w.double() * d2).sum(1) / W.clamp_min(1e-300), torch.zeros_like(W)).sqrt()


def _transform_arg(R, s, t, F, what):
    """(R, s, t) of a caller -> contiguous fp64 device tensors [K, 3, 3], [K], [K, 3] with K = F or 1."""
    R = _tensor(R, what + ': R', (3, 3), (2, 3)).double()
    R = R[None] if R.dim() == 2 else R
    K = R.shape[0]
    if K not in (1, F):
        raise ValueError('%s: R holds %d transforms for %d frames: pass one, or one per frame' % (what, K, F))
    s = torch.as_tensor(s).detach().to(device=R.device, dtype=torch.float64).reshape(-1)
    t = _tensor(t, what + ': t', (3,), (1, 2)).double().reshape(-1, 3)
    if s.shape[0] != K:
        raise ValueError('%s: s holds %d scales for %d transforms' % (what, s.shape[0], K))
    if t.shape[0] != K:
        raise ValueError('%s: t holds %d translations for %d transforms' % (what, t.shape[0], K))
    return R.contiguous(), s.contiguous(), t.contiguous()


# ---- public --------------------------------------------------------------------------------------------------------------------------
def procrustes(src, dst, weights=None, scale=True):
    """The similarity (scale=True) or rigid (False) transform that takes `src` onto `dst` in the weighted least-squares sense:
    minimises sum_i w_i |s R src_i + t - dst_i|^2 per frame.  src, dst [N, 3] or [F, N, 3], paired row by row; weights [N] / [F, N],
    >= 0, or None (ones).  -> a dict of device tensors: R float64 [F, 3, 3] (det +1, also for a mirrored dst: the best PROPER
    rotation), s float64 [F], t float64 [F, 3], rank int32 [F] (3: the rotation is unique, planar clouds included; 1: collinear points,
    the optimal rotation of the smallest angle is returned; 0: coincident points or no weight, R = I), aligned float32 [F, N, 3] (src
    under the transform), rms float64 [F] (sqrt(sum w |aligned - dst|^2 / sum w)); without the frame axis for [N, 3] inputs.

    float64 inputs are taken relative to dst's first point of each frame before they are rounded to fp32 (`pose_metrics._centred`),
    and t is corrected for that shift: R, s and t refer to the caller's coordinates, as does `aligned`."""
    a, b, flat = _clouds(src, dst, 'src', 'dst', same_points=True)
    F, N = a.shape[0], a.shape[1]
    w = None
    if weights is not None:
        w = _tensor(weights, 'weights', (N,), (1, 2))
        w = w[None] if w.dim() == 1 else w
        if w.shape[0] != F:
            raise ValueError('weights has %d frames and src has %d' % (w.shape[0], F))
        if bool(_to_host((w < 0).any() | ~torch.isfinite(w).all())):
            raise ValueError('weights: negative or not finite')
        w = w.to(torch.float32).contiguous()
    if a.dtype == b.dtype == torch.float32:
        c, a32, b32 = None, a.contiguous(), b.contiguous()
    else:
        c = b[:, 0].double()                                          # [F, 3]
        a32, b32 = (a.double() - c[:, None]).float().contiguous(), (b.double() - c[:, None]).float().contiguous()
    R, s, t, rank = _solve(_moments(a32, b32, w), scale)
    aligned = _apply(a32, R, s, t)
    rms = _rms(_paired(aligned, b32), w)
    if c is not None:                                                 # x -> s R (x - c) + t + c
        t = t + c - s[:, None] * torch.einsum('fik,fk->fi', R, c)
        aligned = (aligned.double() + c[:, None]).float()
    out = dict(R=R, s=s, t=t, rank=rank, aligned=aligned, rms=rms)
    return {k: v[0] for k, v in out.items()} if flat else out


def transform(points, R, s, t):
    """points [N, 3] or [F, N, 3] under x -> s R x + t, evaluated in float64 and rounded once -> float32 on the device
    (hn_align_apply).  R [3, 3] / [F, 3, 3], s a number / [F], t [3] / [F, 3]: one transform for every frame, or one per frame."""
    p = _tensor(points, 'points', (3,), (2, 3))
    flat = p.dim() == 2
    p = (p[None] if flat else p).to(torch.float32).contiguous()
    R, s, t = _transform_arg(R, s, t, p.shape[0], 'transform')
    out = _apply(p, R, s, t)
    return out[0] if flat else out


def icp(points, target, iters=30, scale=False, max_distance=None, init=None):
    """Point-to-surface ICP with least-squares steps: `points` [N, 3] aligned to the surface of `target`, a mesh (vertices,
    triangles) or a prepared `mesh_distance.MeshIndex`.  Each of the `iters` iterations applies the accumulated transform to the
    ORIGINAL points (nothing drifts from re-rounding), finds every point's closest surface point (`MeshIndex.closest`), weights it 1,
    or 0 beyond `max_distance`, solves the rigid (scale=False) or similarity Procrustes of the moved points onto their closest points,
    and composes the step into the accumulated transform.  The count is fixed and nothing inside the loop waits for the device; the
    RMS of the weighted distances before each step, and after the last, goes into a device array that is read back once at the end.
    `init`: a dict with R, s, t (or that tuple) to start from.

    -> dict: R float64 [3, 3], s float64 [], t float64 [3], aligned float32 [N, 3] (device tensors), rms (float64 numpy [iters + 1], the
    trace), converged_at (the first iteration after which the RMS changes by less than 1e-9, or `iters`).

    Point-to-plane, symmetric and robust-kernel variants are out of scope, as is any correspondence other than the closest point: a
    start far from the answer converges to a local minimum, as with every ICP."""
    from .mesh_distance import MeshIndex
    iters = int(iters)
    if iters < 1:
        raise ValueError('icp: iters = %d, at least one iteration' % iters)
    if max_distance is not None and not float(max_distance) > 0.0:
        raise ValueError('icp: max_distance = %r must be positive' % (max_distance,))
    p = _tensor(points, 'points', (3,), (2,)).to(torch.float32).contiguous()[None]        # [1, N, 3]
    index = target if isinstance(target, MeshIndex) else MeshIndex(target)
    if index.n_tris == 0:
        raise ValueError('icp: target has no triangles')
    dev = p.device
    if init is None:
        acc = (torch.eye(3, dtype=torch.float64, device=dev)[None].contiguous(), torch.ones(1, dtype=torch.float64, device=dev),
               torch.zeros(1, 3, dtype=torch.float64, device=dev))
    else:
        init = (init['R'], init['s'], init['t']) if isinstance(init, dict) else init
        acc = _transform_arg(init[0], init[1], init[2], 1, 'icp init')
    trace = torch.zeros(iters + 1, dtype=torch.float64, device=dev)

    def query(moved):
        r = index.closest(moved[0], want=('dist', 'point'))
        w = None if max_distance is None else (r['dist'] <= float(max_distance)).to(torch.float32)[None].contiguous()
        return r['dist'][None], r['point'][None].contiguous(), w

    for k in range(iters):
        moved = _apply(p, *acc)
        d, q, w = query(moved)
        trace[k:k + 1] = _rms(d, w)
        R, s, t, _ = _solve(_moments(moved, q, w), scale)
        acc = _compose((R, s, t), acc)
    moved = _apply(p, *acc)
    d, _, w = query(moved)
    trace[iters:] = _rms(d, w)
    rms = _to_host(trace).numpy()                                     # the one read-back
    conv = iters
    for k in range(iters):
        if abs(rms[k + 1] - rms[k]) < 1e-9:
            conv = k
            break
    return dict(R=acc[0][0], s=acc[1][0], t=acc[2][0], aligned=moved[0], rms=rms, converged_at=conv)
