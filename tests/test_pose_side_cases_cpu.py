"""The references and case generators of tests/pose_side_cases.py, checked without a GPU, and the LEFT-hand pose chain on the host:
the float64 oracle (ho-nerf_amd/csrc/hn_pose_chain.h compiled for the host) against tests/golden/pose_chain_left.npz -- what the
reference's own statements give with their handedness flags set to zero (tests/golden/make_golden.py, HONERF_GOLDEN_ONLY=pose_left)."""
import os

import numpy as np
import pytest
import torch

import pose_side_cases as C
from helpers import bounded, record

GOLD_LEFT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_chain_left.npz')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_chain.npz')


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def test_left_hand_oracle_matches_the_reference():
    """Values, joints and the full Jacobian of the 12 left hands at the right-hand test's bound, per hand."""
    from oracle.pose_chain import pose_chain
    g = np.load(GOLD_LEFT)
    assert g['ori_pose'].shape[0] == 12 and not g['is_right'].any()
    assert os.path.getsize(GOLD_LEFT) < 500 * 1024
    bt, j3, jac = pose_chain(g['ori_pose'], g['bone_len'], g['params'], is_right=False)
    assert np.isfinite(jac).all() and np.isfinite(g['jac']).all()
    for name, got, want in (('bt_inv', bt, g['bt_inv']), ('joint_3d', j3, g['joint_3d']), ('jacobian', jac, g['jac'])):
        worst = max(rel(got[f], want[f]) for f in range(got.shape[0]))
        record('left-hand pose chain oracle (fp64) vs reference fp64, worst hand: ' + name, worst, 1e-9)
        assert worst <= 1e-9, (name, worst)   # observed <= 7.8e-12
    # the same hands as right hands are another function: the fixture's own right-hand twins differ by O(1)
    r = np.load(GOLD)
    twin = g['case_of_pose_chain']
    assert np.array_equal(r['ori_pose'][twin], g['ori_pose']) and np.array_equal(r['params'][twin], g['params'])
    assert np.abs(r['bt_inv'][twin] - g['bt_inv']).max() > 0.5 and np.abs(r['jac'][twin] - g['jac']).max() > 0.5
    # and a right-hand evaluation does not pass for a left-hand one
    bt_r, _, _ = pose_chain(g['ori_pose'], g['bone_len'], g['params'], is_right=True, want_jac=False)
    assert rel(bt_r, g['bt_inv']) > 1e-2


@pytest.mark.parametrize('is_right', (True, False))
def test_per_finger_form_is_the_whole_hand_form(is_right):
    """The per-finger form of the chain (what the device kernel runs: four phases, three exchanges) against the whole-hand form, values
    and every Jacobian column, on the fixture's hands.  1e-9 absolute: the bound the host harness (tests/san) holds right hands to;
    the outputs are O(1) and the two forms are the same arithmetic."""
    from oracle.pose_chain import pose_chain_forms_differ
    g = np.load(GOLD_LEFT)
    d = pose_chain_forms_differ(g['ori_pose'], g['bone_len'], g['params'], is_right=is_right)
    bounded('pose chain, per-finger form vs whole-hand form (%s hands), max abs' % ('right' if is_right else 'left'), d, 1e-9, kind='abs')


def test_rigid_reference_matches_the_torch_form():
    """rigid_pose_f64 against RigidPoseChain's CPU form (torch fp32 operators, the reference's lines) where the two overlap: bt_inv,
    joint_3d, obj_r, obj_t.  64 U of each tensor's largest entry: ~30 fp32 roundings along the longest path of the torch form
    (normalise 5, projection 7, cross 3, two 3-term products 5 each, the 4-term affine product 7) times the Gram-Schmidt step's
    amplification 1 / cos 60 deg = 2 on these inputs."""
    from honerf_amd import fitting as F
    for nf, seed in ((1, 1), (5, 2)):
        c = C.rigid_case(nf, seed)
        chain = F.RigidPoseChain(c['bt_inv0'], np.zeros((nf, 21, 3), np.float32), c['joints0'], c['Ro_pred'], c['To_pred'],
                                 np.zeros((4, 3), np.float32), device='cpu')
        prm = torch.from_numpy(c['params'])
        with torch.no_grad():
            chain.obj_rot.copy_(prm[:, 0:6].reshape(nf, 3, 2))
            chain.obj_trans.copy_(prm[:, 6:9])
            chain.palm_rot.copy_(prm[:, 9:15].reshape(nf, 3, 2))
            chain.palm_trans.copy_(prm[:, 15:18])
            pose = chain()
        want = C.rigid_pose_f64(c['bt_inv0'], c['joints0'], c['Ro_pred'], c['To_pred'], c['params'], 1)
        for (name, a, b), key in zip(C.RIGID_SEGMENTS[:4], ('bt_inv', 'joint_3d', 'obj_r', 'obj_t')):
            w = want[:, a:b].numpy()
            e = rel(pose[key].reshape(nf, -1).numpy(), w)
            bounded('rigid_pose_f64 vs RigidPoseChain (torch fp32, CPU), F = %d: %s' % (nf, name), e, 64 * C.U)
        # the object half alone: the same numbers, the rest NaN
        half = C.rigid_pose_f64(None, None, c['Ro_pred'], c['To_pred'], c['params'], 0)
        assert torch.equal(half[:, 399:411], want[:, 399:411]) and torch.isnan(half[:, :399]).all() and torch.isnan(half[:, 411]).all()


def test_rigid_reference_jacobian_matches_central_differences():
    for seed in (3, 4):
        c = C.rigid_case(1, seed)
        args = [C.f64(c[k])[0] for k in ('bt_inv0', 'joints0', 'Ro_pred', 'To_pred')]
        prm = C.f64(c['params'])[0]
        _, jac = C.rigid_pose_f64(c['bt_inv0'], c['joints0'], c['Ro_pred'], c['To_pred'], c['params'], 1, want_jac=True)
        h = 1e-6
        fd = torch.empty(412, 18, dtype=torch.float64)
        for k in range(18):
            e = torch.zeros(18, dtype=torch.float64)
            e[k] = h
            fd[:, k] = (C._rigid_frame(prm + e, *args, 1) - C._rigid_frame(prm - e, *args, 1)) / (2 * h)
        bounded('rigid_pose_f64: autograd Jacobian vs central differences (h = 1e-6), seed %d' % seed,
                float((jac[0] - fd).abs().max() / jac[0].abs().max()), 1e-6)
        assert float(jac[0].abs().max()) > 0.1 and float(jac[0][399:411, 9:18].abs().max()) == 0.0


def test_rigid_initial_state_reference():
    """At the state a fit starts from the joint loss is exactly 0 and its row of the Jacobian exactly 0 (norm's derivative at 0)."""
    c = C.rigid_case(2, 5, initial=True)
    out, jac = C.rigid_pose_f64(c['bt_inv0'], c['joints0'], c['Ro_pred'], c['To_pred'], c['params'], 1, want_jac=True)
    assert float(out[:, 411].abs().max()) == 0.0 and float(jac[:, 411].abs().max()) == 0.0 and torch.isfinite(jac).all()
    assert torch.equal(out[:, :336], C.f64(c['bt_inv0']).reshape(2, 336))


def test_generator_conditions():
    # rot6d inputs: off the manifold as announced
    g = torch.Generator().manual_seed(0)
    r6 = C.rot6d_offnormal(64, g).reshape(64, 3, 2)
    n1, n2 = r6[:, :, 0].norm(dim=-1), r6[:, :, 1].norm(dim=-1)
    cosang = (r6[:, :, 0] * r6[:, :, 1]).sum(-1) / (n1 * n2)
    assert 0.3 <= float(min(n1.min(), n2.min())) and float(max(n1.max(), n2.max())) <= 3.0
    assert float(cosang.abs().max()) <= np.sin(np.radians(60.0)) + 1e-12 and float(cosang.abs().max()) > 0.5
    # vertex loss: the kappa cap of the regular cases (verts_case asserts it), and the exact zeros of the others
    for V in (1, 63, 256, 257, 1000):
        for P in (1, 3):
            c = C.verts_case(V, P, 100 + V + P)
            assert 0.0 < c['kappa_max'] <= 10.0
    c = C.verts_case(63, 3, 7, 'same')
    assert np.array_equal(c['Ra'], c['Rb']) and np.array_equal(c['ta'], c['tb'])
    out = C.verts_loss_f64(c['Ra'], c['ta'], c['Rb'], c['tb'], c['verts'], want_grad=True)
    assert all(float(x.abs().max()) == 0.0 and torch.isfinite(x).all() for x in out)
    c = C.verts_case(63, 3, 8, 'zero')
    assert not c['verts'][0].any() and np.array_equal(c['ta'], c['tb']) and c['verts'][1:].any(axis=1).all()
    kap = C.verts_bounds(c['Ra'], c['ta'], c['Rb'], c['tb'], c['verts'])[3]
    assert float(kap[:, 0].max()) == 0.0 and float(kap[:, 1:].min()) >= 1.0
    # Adam: exact zero gradients on zero moments exist in the blocks that have history, and leave p where it is
    blocks = C.adam_case(C.ADAM_SIZES_16, 1)
    assert [b['step'] for b in blocks] == list(range(1, 17)) and [b['p'].size for b in blocks] == list(C.ADAM_SIZES_16)
    assert sum(int(((b['g'] == 0) & (b['m'] == 0) & (b['v'] == 0)).sum()) for b in blocks if b['step'] > 1) >= 8
    for b in blocks:
        p2, m2, v2, dp = C.adam_f64(b['p'], b['g'], b['m'], b['v'], b['lr'], 0.9, 0.999, 1e-8, b['step'])
        still = (b['g'] == 0) & (b['m'] == 0) & (b['v'] == 0)
        assert np.array_equal(p2[still], b['p'][still].astype(np.float64)) and np.isfinite(p2).all()
        assert (b['m'] * b['g'] >= 0).all() and (b['v'] >= 0).all()
    # leaf rows: the exact-compare scatter has no repeated row, the repeat's case has one
    assert len(set(C.LEAF_ROWS_SCATTER)) == len(C.LEAF_ROWS_SCATTER) and len(set(C.LEAF_ROWS_REPEAT)) < len(C.LEAF_ROWS_REPEAT)
    assert C.LEAF_ROWS == (6, 0, 3, 3, -1, 7)


def test_adam_reference_is_torch_adam():
    """adam_f64 against torch.optim.Adam in float64 over three steps (the formula, not the kernel)."""
    rng = np.random.RandomState(0)
    p0 = rng.standard_normal(50)
    p = torch.nn.Parameter(torch.tensor(p0))
    lr, b1, b2, eps = (float(np.float32(x)) for x in (3e-4, 0.9, 0.999, 1e-8))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    q, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    for step in (1, 2, 3):
        g = rng.standard_normal(50)
        p.grad = torch.tensor(g)
        opt.step()
        q, m, v, _ = C.adam_f64(q, g, m, v, lr, b1, b2, eps, step)
    bounded('adam_f64 vs torch.optim.Adam (float64), three steps: difference / movement',
            float(np.abs(q - p.detach().numpy()).max() / np.abs(q - p0).max()), 1e-12)


def test_index_references():
    leaves, g = C.leaf_case()
    h, o = C.leaf_rows_gather_ref(leaves, C.LEAF_ROWS)
    assert np.array_equal(h[0, :20], leaves[4][6]) and np.array_equal(h[1, 27:33], leaves[2][0]) and np.array_equal(o[2, 6:9], leaves[1][3])
    assert np.isnan(h[4:]).all() and np.isnan(o[4:, :9]).all() and not o[:, 9:].any()
    outs = C.leaf_rows_scatter_ref(g, C.LEAF_ROWS_SCATTER, C.LEAF_ROWS_N)
    assert np.array_equal(outs[4][5], g[3, 0:20]) and np.array_equal(outs[0][6], g[0, 36:42]) and not outs[3][[1, 2, 4]].any()
    assert sum(int((x != 0).sum()) for x in outs) == 4 * 45
    # vjp: the magnitude sum bounds the value
    J, gg = np.random.RandomState(1).standard_normal((2, 29, 18)).astype(np.float32), np.random.RandomState(2).standard_normal((2, 29)).astype(np.float32)
    val, mag = C.vjp_f64(J, gg)
    assert (val.abs() <= mag).all() and np.allclose(val.numpy(), np.einsum('fok,fo->fk', J.astype(np.float64), gg.astype(np.float64)))
