"""Cases of the pose side of a fitting step (ho-nerf_amd/csrc/hn_pose_rigid.hip, hn_pose_chain.hip): the float64 references and the
seeded fp32 inputs.  A plain module, in the manner of composite_cases / gbuffer_cases: tests/test_pose_side_cases_cpu.py (are the
references and the generators what they claim to be?) and tests/test_gpu_pose_side.py (are the kernels within their bounds of the
references?) both import it.

Every reference takes the fp32 values the kernel gets, casts them up and works in float64 from there, so that the only differences
left are the kernel's own roundings.  The bounds those are held to (U = 2^-24, the unit roundoff of fp32):

  hn_pose_chain, hn_rigid_pose   compute in double and round ONCE: |got - want| <= 2 U max |want| per tensor and frame (DOUBLE_ONCE)
  fp32 contractions              |got - want| <= K U sum |addends| per output, K the length of the longest chain of dependent
                                 roundings of that kernel (K_VJP, K_CHAIN_BWD, K_SIDE_OBJ, k_verts_*)
  hn_adam_step                   |p - p64| <= U |p64| + 16 U |dp64|; m, v: 4 U relative (adam_bounds)

The generators return, beside each case, the quantity its bound is scaled by."""
import math

import numpy as np
import torch

from oracle.losses import rot6d_to_matrix

U = 2.0 ** -24
DOUBLE_ONCE = 2.0 * U            # one rounding double -> fp32 (<= U relative), with a factor 2

F64 = torch.float64


def f64(a):
    return torch.as_tensor(np.asarray(a)).to(F64) if not isinstance(a, torch.Tensor) else a.detach().cpu().to(F64)


def _rotations(n, g):
    """n random proper rotations [n,3,3], float64."""
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=F64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    return q * torch.linalg.det(q)[:, None, None]


# ---- hn_rigid_pose -------------------------------------------------------------------------------------------------------------
# out [F,412] = [bt_inv 336 | joint_3d 63 | obj_r 9 | obj_t 3 | joint loss 1] of params [F,18] = [obj_rot 6 | obj_trans 3 | palm_rot 6 |
# palm_trans 3] (include/honerf.h): G p = R_palm (p - root) + root + T_palm, bt_inv = bt_inv0 G^-1, joint_3d = G joints0,
# obj_r = rot6d(obj_rot) Ro_pred, obj_t = To_pred + obj_trans, joint loss = mean_j |joints0_j - joint_3d_j|
RIGID_SEGMENTS = (('bt_inv', 0, 336), ('joint_3d', 336, 399), ('obj_r', 399, 408), ('obj_t', 408, 411), ('joint_loss', 411, 412))


def _rigid_frame(prm, bt0, j0, Ro, To, with_palm):
    """One frame: prm [18] -> out [412] (float64 torch; differentiable in prm).  with_palm == 0: the hand entries are NaN."""
    obj_r = rot6d_to_matrix(prm[0:6].reshape(1, 3, 2))[0] @ Ro
    obj_t = To + prm[6:9]
    if not with_palm:
        nan = torch.full((399,), float('nan'), dtype=F64)
        return torch.cat([nan, obj_r.reshape(-1), obj_t, nan[:1]])
    R = rot6d_to_matrix(prm[9:15].reshape(1, 3, 2))[0]
    T = prm[15:18]
    root = j0[0]
    joint_3d = (j0 - root) @ R.T + root + T
    Ginv = torch.zeros(4, 4, dtype=F64)
    Ginv[:3, :3] = R.T
    Ginv[:3, 3] = root - R.T @ (root + T)
    Ginv[3, 3] = 1.0
    bt_inv = bt0 @ Ginv
    loss = torch.linalg.vector_norm(j0 - joint_3d, dim=-1).mean()      # (its derivative at 0 is 0: torch's convention, and the kernel's)
    return torch.cat([bt_inv.reshape(-1), joint_3d.reshape(-1), obj_r.reshape(-1), obj_t, loss.reshape(1)])


def rigid_pose_f64(bt_inv0, joints0, Ro_pred, To_pred, params, with_palm=1, want_jac=False):
    """hn_rigid_pose in float64 on the given (fp32) values: out [F,412]; with want_jac also jac [F,412,18] (autograd).  Entries the
    kernel leaves untouched for with_palm == 0 are NaN."""
    prm = f64(params).reshape(-1, 18)
    F = prm.shape[0]
    Ro, To = f64(Ro_pred).reshape(F, 3, 3), f64(To_pred).reshape(F, 3)
    bt0 = f64(bt_inv0).reshape(F, 21, 4, 4) if with_palm else [None] * F
    j0 = f64(joints0).reshape(F, 21, 3) if with_palm else [None] * F
    outs, jacs = [], []
    for f in range(F):
        fn = lambda x: _rigid_frame(x, bt0[f], j0[f], Ro[f], To[f], with_palm)
        outs.append(fn(prm[f]).detach())
        if want_jac:
            J = torch.autograd.functional.jacobian(fn, prm[f]).detach()
            if not with_palm:
                J[:399] = float('nan')
                J[411:] = float('nan')
            jacs.append(J)
    out = torch.stack(outs)
    return (out, torch.stack(jacs)) if want_jac else out


def rot6d_offnormal(n, g):
    """n 6-D rotation inputs [n,6] (row-major [3][2]) that are NOT normalised: column norms 0.3 .. 3, the second column up to 60 degrees
    from orthogonal to the first (rot6d's Gram-Schmidt has real work to do, and so has its derivative)."""
    a = torch.randn(n, 3, generator=g, dtype=F64)
    a = a / a.norm(dim=-1, keepdim=True)
    b = torch.randn(n, 3, generator=g, dtype=F64)
    b = b - (b * a).sum(-1, keepdim=True) * a
    b = b / b.norm(dim=-1, keepdim=True)
    th = (torch.rand(n, 1, generator=g, dtype=F64) * 2 - 1) * math.radians(60.0)
    n1 = 0.3 + 2.7 * torch.rand(n, 1, generator=g, dtype=F64)
    n2 = 0.3 + 2.7 * torch.rand(n, 1, generator=g, dtype=F64)
    c1, c2 = n1 * a, n2 * (torch.cos(th) * b + torch.sin(th) * a)
    return torch.stack([c1, c2], dim=-1).reshape(n, 6)


def rigid_case(F, seed, initial=False):
    """fp32 inputs of hn_rigid_pose for F frames: dict of numpy arrays bt_inv0 [F,21,4,4] (rigid maps), joints0 [F,21,3], Ro_pred, To_pred,
    params [F,18].  initial: the state a fit starts from (identity 6-D blocks, zero translations)."""
    g = torch.Generator().manual_seed(seed)
    bt = torch.zeros(F, 21, 4, 4, dtype=F64)
    bt[:, :, :3, :3] = _rotations(F * 21, g).reshape(F, 21, 3, 3)
    bt[:, :, :3, 3] = 0.1 * torch.randn(F, 21, 3, generator=g, dtype=F64)
    bt[:, :, 3, 3] = 1.0
    joints = torch.tensor([0.0, 0.0, 0.9], dtype=F64) + 0.08 * torch.randn(F, 21, 3, generator=g, dtype=F64)
    Ro = _rotations(F, g)
    To = torch.tensor([0.0, 0.0, 0.9], dtype=F64) + 0.05 * torch.randn(F, 3, generator=g, dtype=F64)
    if initial:
        eye6 = torch.eye(3, dtype=F64)[:, :2].reshape(1, 6).expand(F, 6)
        prm = torch.cat([eye6, torch.zeros(F, 3, dtype=F64), eye6, torch.zeros(F, 3, dtype=F64)], dim=1)
    else:
        prm = torch.cat([rot6d_offnormal(F, g), 0.05 * torch.randn(F, 3, generator=g, dtype=F64), rot6d_offnormal(F, g),
                         0.05 * torch.randn(F, 3, generator=g, dtype=F64)], dim=1)
    c = lambda x: np.ascontiguousarray(x.numpy().astype(np.float32))
    return dict(bt_inv0=c(bt), joints0=c(joints), Ro_pred=c(Ro), To_pred=c(To), params=c(prm))


# ---- hn_verts_loss -------------------------------------------------------------------------------------------------------------
def verts_loss_f64(Ra, ta, Rb, tb, verts, want_grad=False):
    """loss [P] = mean_v |(Ra - Rb) v + (ta - tb)| in float64; with want_grad also d loss[p] / d (Ra, ta, Rb, tb)[p] by autograd."""
    x = [f64(Ra).reshape(-1, 3, 3), f64(ta).reshape(-1, 3), f64(Rb).reshape(-1, 3, 3), f64(tb).reshape(-1, 3)]
    v = f64(verts).reshape(-1, 3)
    x = [a.clone().requires_grad_(want_grad) for a in x]
    e = torch.einsum('pij,vj->pvi', x[0] - x[2], v) + (x[1] - x[3])[:, None, :]
    loss = torch.linalg.vector_norm(e, dim=-1).mean(dim=1)
    if not want_grad:
        return loss.detach()
    grads = torch.autograd.grad(loss.sum(), x)          # (pairs are independent: the sum's gradient is each pair's own)
    return (loss.detach(),) + tuple(g_.detach() for g_ in grads)


def verts_bounds(Ra, ta, Rb, tb, verts):
    """hn_verts_loss's bounds, float64: per pair U mean_v K_v |addend_v| for each of the 13 sums (loss [P], gR [P,3,3], gt [P,3]) with
    K_v = k_verts_loss / k_verts_grad at the vertex's own conditioning kappa_v = (|D| |v| + |d|) / |e| of its residual e = D v + d
    (Frobenius / Euclidean norms), and kappa [P,V] itself (0 where e == 0 exactly: such a vertex contributes exact zeros)."""
    D = f64(Ra).reshape(-1, 3, 3) - f64(Rb).reshape(-1, 3, 3)
    d = f64(ta).reshape(-1, 3) - f64(tb).reshape(-1, 3)
    v = f64(verts).reshape(-1, 3)
    V = v.shape[0]
    e = torch.einsum('pij,vj->pvi', D, v) + d[:, None, :]
    n = e.norm(dim=-1)                                                                    # [P,V]
    u = torch.where(n[..., None] > 0, e / n[..., None].clamp_min(1e-300), torch.zeros_like(e))
    kappa = (D.flatten(1).norm(dim=-1)[:, None] * v.norm(dim=-1)[None, :] + d.norm(dim=-1)[:, None]) / n.clamp_min(1e-300)
    kappa = torch.where(n > 0, kappa, torch.zeros_like(kappa))
    kl, kg = k_verts_loss(V, kappa), k_verts_grad(V, kappa)                                # [P,V]
    b_loss = U * (kl * n).mean(dim=1)
    b_gR = U * (kg[:, :, None, None] * (u[:, :, :, None] * v[None, :, None, :]).abs()).mean(dim=1)
    b_gt = U * (kg[:, :, None] * u.abs()).mean(dim=1)
    return b_loss, b_gR, b_gt, kappa


def k_verts_loss(V, kappa):
    """K of the loss: ceil(V / 256) adds in a thread's accumulator + 6 shuffle steps + 3 adds of the four waves + 1 division by V, and per
    term: D = Ra - Rb rounds once and the three products and three adds of e at most five times more, all relative to
    |D| |v| + |d| = kappa |e|: 6 kappa; e . e 3, halved by the root: 1.5; the root itself at most 1.5 -> 6 kappa + 3.
    (kappa: a number or a tensor of per-vertex values)"""
    return math.ceil(V / 256.0) + 10 + 6.0 * kappa + 3


def k_verts_grad(V, kappa):
    """K of gR / gt: the same chain (ceil(V / 256) + 10), and per term u = e / |e|: the residual's error 6 kappa enters twice (through e and
    through |e|), the norm's own 3, the reciprocal and its product 2 (2 U each at worst: 4), the product with the vertex coordinate 1."""
    return math.ceil(V / 256.0) + 10 + 12.0 * kappa + 8


def verts_case(V, P, seed, kind='regular'):
    """fp32 inputs of hn_verts_loss: Ra, ta, Rb, tb [P,...], verts [V,3] (an object's vertices: a few centimetres).
    regular: two poses some degrees and centimetres apart, kappa_v <= 10 for every vertex (asserted: the unit residual is then well
    defined in fp32, and a failure means the kernel);  same: identical poses (every residual exactly 0);
    zero: regular with vertex 0 at the origin and ta == tb (one exactly zero residual among non-zero ones; without a translation a
    vertex near the rotation axis has a large kappa_v, which its own term of the bound carries)."""
    g = torch.Generator().manual_seed(seed)
    # |v| <= 0.05, a relative rotation of at most 0.3 rad (|D| = 2 sqrt(2) sin(angle / 2) <= 0.43) and 0.05 <= |d| <= 0.08:
    # |D| |v| <= 0.022 < |d|, so kappa_v <= (0.022 + |d|) / (|d| - 0.022) <= 2.6 by construction
    verts = 0.02 * torch.randn(V, 3, generator=g, dtype=F64)
    verts = verts * (0.05 / verts.norm(dim=-1, keepdim=True)).clamp(max=1.0)
    Rb = _rotations(P, g)
    ang = 0.1 * torch.randn(P, 3, generator=g, dtype=F64)
    ang = ang * (0.3 / ang.norm(dim=-1, keepdim=True)).clamp(max=1.0)
    K = torch.zeros(P, 3, 3, dtype=F64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -ang[:, 2], ang[:, 1], -ang[:, 0]
    Ra = torch.matrix_exp(K - K.transpose(1, 2)) @ Rb
    tb = torch.tensor([0.0, 0.0, 0.9], dtype=F64) + 0.05 * torch.randn(P, 3, generator=g, dtype=F64)
    dirs = torch.randn(P, 3, generator=g, dtype=F64)
    ta = tb + dirs / dirs.norm(dim=-1, keepdim=True) * (0.05 + 0.03 * torch.rand(P, 1, generator=g, dtype=F64))
    if kind == 'same':
        Ra, ta = Rb.clone(), tb.clone()
    if kind == 'zero':
        verts[0] = 0.0
        ta = tb.clone()
    c = lambda x: np.ascontiguousarray(x.numpy().astype(np.float32))
    case = dict(Ra=c(Ra), ta=c(ta), Rb=c(Rb), tb=c(tb), verts=c(verts))
    kappa = verts_bounds(case['Ra'], case['ta'], case['Rb'], case['tb'], case['verts'])[3]
    if kind == 'regular':
        assert float(kappa.max()) <= 10.0, 'verts_case(%d, %d, %d): kappa %.2f > 10' % (V, P, seed, float(kappa.max()))
    case['kappa_max'] = float(kappa.max()) if kind != 'same' else 0.0
    return case


# ---- stored-Jacobian contractions ------------------------------------------------------------------------------------------------
def vjp_f64(jac, g):
    """out [F,n_in] = jac [F,n_out,n_in]^T g [F,n_out] in float64, and the sum of the addends' magnitudes [F,n_in]."""
    J, gg = f64(jac), f64(g)
    gg = gg.reshape(J.shape[0], J.shape[1])
    return torch.einsum('fok,fo->fk', J, gg), torch.einsum('fok,fo->fk', J.abs(), gg.abs())


def k_vjp(n_out):
    """k_jacobian_vjp / the hand half of k_pose_side_vjp: wave w walks the outputs o = w (mod 4) with four accumulators: ceil(n_out / 16)
    fused multiply-adds in the longest, at most 3 more in the 4-strided tail, then (a0 + a1) + (a2 + a3): 2, and the four waves'
    (p0 + p1) + (p2 + p3): 2.  The issue's count: ceil(n_out / 16) + 8."""
    return math.ceil(n_out / 16.0) + 8


K_CHAIN_BWD = 400     # k_pose_chain_bwd: ONE chain of 336 + 63 = 399 fused multiply-adds, + 1
K_SIDE_OBJ = 13       # k_pose_side_vjp's object columns: g + g2 (1, relative to |g| + |g2|), a chain of 12 fused multiply-adds; the
#                       combining adds that follow add exact zeros


def pose_side_vjp_f64(jac_h, jac_o, g_bt, g_j3, g_or, g_ot, g_or2, g_ot2, which, F, prefill):
    """hn_pose_side_vjp in float64: out [F,45], the sum of the addends' magnitudes [F,45], and the mask of the columns `which` selects
    (the others hold `prefill` in out).  A None upstream gradient counts as zero; jac_h [F,399,36], jac_o [F,412,18] (rows 399 .. 410,
    columns 0 .. 8 are read)."""
    z = lambda n: torch.zeros(F, n, dtype=F64)
    opt = lambda a, n: z(n) if a is None else f64(a).reshape(F, n)
    out = torch.full((F, 45), float(prefill), dtype=F64)
    mag = torch.zeros(F, 45, dtype=F64)
    sel = torch.zeros(45, dtype=torch.bool)
    if which & 1:
        go = torch.cat([opt(g_bt, 336), opt(g_j3, 63)], dim=1)
        out[:, :36], mag[:, :36] = vjp_f64(f64(jac_h).reshape(F, 399, 36), go)
        sel[:36] = True
    if which & 2:
        Jo = f64(jac_o).reshape(F, 412, 18)[:, 399:411, 0:9]
        g1, g2 = torch.cat([opt(g_or, 9), opt(g_ot, 3)], dim=1), torch.cat([opt(g_or2, 9), opt(g_ot2, 3)], dim=1)
        out[:, 36:45] = torch.einsum('fok,fo->fk', Jo, g1 + g2)
        mag[:, 36:45] = torch.einsum('fok,fo->fk', Jo.abs(), g1.abs() + g2.abs())
        sel[36:45] = True
    return out, mag, sel


# ---- the window's rows of the six pose leaves <-> the chain's input blocks ----------------------------------------------------------
# leaves (in the order of hn_leaf_rows_gather's pointers): obj_rot [n,6], obj_trans [n,3], palm_rot [n,6], palm_trans [n,3],
# joint_refine_angle [n,20], palm_refine_angle [n,7]
LEAF_WIDTHS = (6, 3, 6, 3, 20, 7)
# column range of prm_hand [36] / g[0:36] and of prm_obj [0:9] / g[36:45] that each leaf fills: (leaf, first column in g's 45)
LEAF_COLUMNS = ((4, 0), (5, 20), (2, 27), (3, 33), (0, 36), (1, 42))


def leaf_rows_gather_ref(leaves, rows):
    """(prm_hand [F,36], prm_obj [F,18]) as indexing: a row outside [0, n) reads NaN in the 45 gathered columns; prm_obj[:, 9:18] = 0."""
    n = leaves[0].shape[0]
    F = len(rows)
    g45 = np.full((F, 45), np.nan, dtype=np.float32)
    for f, r in enumerate(rows):
        if 0 <= r < n:
            for leaf, c0 in LEAF_COLUMNS:
                g45[f, c0:c0 + LEAF_WIDTHS[leaf]] = leaves[leaf][r]
    prm_o = np.zeros((F, 18), dtype=np.float32)
    prm_o[:, :9] = g45[:, 36:]
    return g45[:, :36].copy(), prm_o


def leaf_rows_scatter_ref(g45, rows, n, candidates=False):
    """The six gradient blocks [n,w] (zero where no row points) as indexing; rows outside [0, n) write nothing.  A row that appears twice
    has no defined writer: candidates=True returns, per block, the list of the arrays each writer alone would leave."""
    outs = [np.zeros((n, w), dtype=np.float32) for w in LEAF_WIDTHS]
    alts = [[] for _ in LEAF_WIDTHS]
    for f, r in enumerate(rows):
        if 0 <= r < n:
            for leaf, c0 in LEAF_COLUMNS:
                outs[leaf][r] = g45[f, c0:c0 + LEAF_WIDTHS[leaf]]
                alts[leaf].append((r, g45[f, c0:c0 + LEAF_WIDTHS[leaf]].copy()))
    return (outs, alts) if candidates else outs


LEAF_ROWS_N = 7
LEAF_ROWS = (6, 0, 3, 3, -1, 7)              # the gather's rows: a repeat, and one row off either end
LEAF_ROWS_SCATTER = (6, 0, 3, 5, -1, 7)      # the exact-compare scatter: no repeats (the last writer of a repeated row is unordered)
LEAF_ROWS_REPEAT = (3, 1, 3)                 # the repeat's own case: row 3 holds what one of its two writers wrote


def leaf_case(seed=0):
    """The six leaves [7,w] and g [6,45], every entry a distinct small integer-valued float (exact in fp32, so 'equal' means equal)."""
    leaves, at = [], 1
    for w in LEAF_WIDTHS:
        leaves.append((at + np.arange(LEAF_ROWS_N * w)).reshape(LEAF_ROWS_N, w).astype(np.float32))
        at += LEAF_ROWS_N * w
    g = (1000 + np.arange(len(LEAF_ROWS) * 45)).reshape(len(LEAF_ROWS), 45).astype(np.float32)
    return leaves, g


# ---- hn_adam_step ---------------------------------------------------------------------------------------------------------------------
def adam_f64(p, g, m, v, lr, b1, b2, eps, step):
    """torch.optim.Adam's update as hn_pose_rigid.hip states it, in float64 on the fp32 values the kernel gets (lr, b1, b2, eps are
    passed as fp32):  m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g g;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    Returns (p, m, v, dp) with dp the step taken."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m2 = m + (g - m) * (1.0 - b1)
    v2 = b2 * v + (1.0 - b2) * g * g
    dp = (lr / (1.0 - b1 ** step)) * m2 / (np.sqrt(v2) / math.sqrt(1.0 - b2 ** step) + eps)
    return p - dp, m2, v2, dp


def adam_bounds(p64, m64, v64, dp64):
    """Per element.  p: the final subtraction rounds once (U |p|), and the step carries 16 U: m 3 (g - m, its product, the sum: the moments
    and gradients of adam_case have one sign per element, so nothing cancels), v 3 (two products of the g term, the b2 product, the sum of
    positive terms: 4, one shared), its root 1.5 + 1, the bias correction sqrt(1 - b2^t) rounded to fp32 1 and the division by it 1, + eps
    1, the quotient m / denom 1, lr / (1 - b1^t) 2, the product 1: 15.5 with correctly rounded root and division.  m, v: 4 U relative."""
    return U * np.abs(p64) + 16 * U * np.abs(dp64), 4 * U * np.abs(m64), 4 * U * np.abs(v64)


ADAM_SIZES_16 = (0, 1, 255, 256, 257, 0, 1023, 1024, 1025, 3, 20, 7, 6, 0, 4096, 5)
ADAM_BIG = ((40000, 30000), (100000, 100000, 100000))       # totals above 65 536 (64 blocks) and above 262 144 (256: the grid-stride walk)


def adam_case(sizes, seed, first_step=False):
    """fp32 blocks p, g, m, v of the given sizes (numpy), per-block step counts 1 .. and learning rates.  Gradients span 1e-6 .. 10 with
    exact zeros among them; the moments are those of earlier steps of same-signed gradients (m has g's sign, v > 0) -- with mixed signs
    m + (g - m)(1 - b1) cancels and NO relative bound holds for it in any precision -- except where the step count is 1 or the
    gradient is an exact zero on the first elements of a block: there the moments are zero too (p must not move)."""
    rng = np.random.RandomState(seed)
    blocks = []
    for t, n in enumerate(sizes):
        step = 1 if first_step else t + 1
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
        g[rng.rand(n) < 0.1] = 0.0
        p = rng.standard_normal(n).astype(np.float32)
        if step == 1:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            sgn = np.where(g != 0, np.sign(g), np.sign(rng.standard_normal(n))).astype(np.float32)
            mag = (10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
            m, v = (sgn * mag).astype(np.float32), (mag * mag * rng.uniform(0.5, 2.0, n)).astype(np.float32)
            z = (g == 0) & (np.arange(n) < 8)
            m[z], v[z] = 0.0, 0.0
        blocks.append(dict(p=p, g=g, m=m, v=v, step=step, lr=float(np.float32(1e-4 * (1 + t)))))
    return blocks
