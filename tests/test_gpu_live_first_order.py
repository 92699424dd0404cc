"""Live-first sample order of the dense hand-field launch of NeuSRenderer.render (HONERF_LIVE_FIRST): the final
evaluation runs on the list [live samples | far samples] and its outputs are brought back to dense order.  Every sample is
evaluated either way, and no result depends on the lane, wave or tile a sample sits in, so the render must return the SAME BITS
with the order off (HONERF_LIVE_FIRST=0) and on at every size (=2).  The shapes are the smallest at which the permutation can go
wrong; each case also checks, with the classification restated in torch, that its scene is what its name says."""
import numpy as np
import pytest
import torch

from honerf_amd import synth

pytestmark = pytest.mark.gpu

CUTOFF = torch.tensor([0.08, 0.03, 0.03, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02, 0.02, 0.02, 0.03, 0.02,
                       0.02, 0.02])
FOCAL = 2.0
BT_INV, T_POSE, JOINTS = synth.synth_hand_pose(9)


@pytest.fixture(scope='module')
def renderers():
    """One hand renderer per precision, made on first use and shared by the cases (packing is the expensive part)."""
    from honerf_amd.nets import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
    from honerf_amd.renderer import NeuSRenderer
    made = {}

    def get(precision, n_samples):
        if precision not in made:
            dev = torch.device('cuda')
            sdf, col, var = SDFNetwork().to(dev), RenderingNetwork(use_gradients=True).to(dev), SingleVarianceNetwork(0.3).to(dev)
            sdf.reset_parameters(21)
            col.reset_parameters(22)
            ren = NeuSRenderer(sdf, var, col, 'hand', n_samples, 0, 0, 4, 1.0)
            ren.precision = precision
            made[precision] = ren
        made[precision].n_samples = n_samples
        return made[precision]
    return get


def rays_through(points):
    """Rays of a camera at the origin looking along +z (R = I, T = 0, focal 2) through the given world points:
    unproject at depth 1 and 2, d = normalize(p2 - p1), o = p1 - d."""
    p = torch.as_tensor(np.asarray(points), dtype=torch.float32)
    xy = FOCAL * p[:, :2] / p[:, 2:3]
    p1 = torch.cat([xy / FOCAL, torch.ones(len(p), 1)], dim=-1)
    d = torch.nn.functional.normalize(p1, dim=-1)
    return (p1 - d).contiguous(), d.contiguous()


def depth_of(point):
    """The depth t at which the ray through `point` reaches it: o + d t = d (|p1| + t - 1) with |p1| = |point| / point_z."""
    n = float(np.linalg.norm(point))
    return n - n / float(point[2]) + 1.0


def live_mask(o, d, z, near, far, n_samples):
    """The classification of the ordering pass (far only if 200 (v_b - cutoff_b) > 17 for every bone) at the section mid-points."""
    z = z.cpu()
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], (far - near) / n_samples)], dim=-1)
    pts = o.cpu()[:, None, :] + d.cpu()[:, None, :] * (z + 0.5 * dist)[..., None]
    bt, tp = torch.from_numpy(BT_INV), torch.from_numpy(T_POSE)
    q = torch.einsum('bij,nsj->nsbi', bt[:, :3, :3], pts) + bt[:, :3, 3] - tp
    return (~(200.0 * (q.norm(dim=-1) - CUTOFF) > 17.0)).any(-1).reshape(-1)


def render(ren, o, d, near, far, t_rand, monkeypatch, mode):
    monkeypatch.setenv('HONERF_LIVE_FIRST', mode)
    with torch.no_grad():
        out = ren.render(o.cuda(), d.cuda(), near, far, torch.from_numpy(BT_INV).cuda(), torch.from_numpy(T_POSE).cuda(), None, None, None, 0, t_rand=t_rand.cuda())
    out = {k: v.clone() for k, v in out.items()}
    out['z_vals'] = ren.last_z_vals.clone()
    torch.cuda.synchronize()
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), '%s: %s differs' % (what, k)


def off_and_on(ren, o, d, near, far, t_rand, monkeypatch):
    off = render(ren, o, d, near, far, t_rand, monkeypatch, '0')
    on = render(ren, o, d, near, far, t_rand, monkeypatch, '2')
    assert_same(off, on, 'live-first order on / off')
    assert bool(torch.isfinite(off['color_fine']).all())
    return off


def mixed_rays():
    """Six rays that pass joints of the hand at 5 mm (a sample ON a joint is NaN, as in the reference) and one that misses the hand."""
    return rays_through(np.concatenate([JOINTS[[0, 4, 8, 12, 16, 20]] + np.float32(0.005), np.array([[0.5, 0.5, 0.9]], dtype=np.float32)]))


def wrist_rays(n):
    """n rays through points about 1 cm from the wrist joint."""
    off = 0.01 * torch.nn.functional.normalize(torch.randn(n, 3, generator=torch.Generator().manual_seed(3)), dim=-1).numpy()
    return rays_through(JOINTS[0][None] + off.astype(np.float32))


@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
def test_two_tiles_with_the_boundary_inside_a_wave(renderers, monkeypatch, precision):
    """7 rays x 24 samples = 168 samples: two tiles, the second one partial; live and far samples alternate along the dense list and the
    boundary between the two parts of the ordered list falls inside a wave."""
    ren = renderers(precision, 24)
    o, d = mixed_rays()
    tr = torch.rand(7, 1, generator=torch.Generator().manual_seed(1))
    out = off_and_on(ren, o, d, 0.4, 1.5, tr, monkeypatch)
    live = live_mask(o, d, out['z_vals'], 0.4, 1.5, 24)
    n_live = int(live.sum())
    assert live.numel() == 168 and 0 < n_live < 168 and n_live % 32 != 0, n_live
    assert not bool(live.reshape(7, 24)[6].any()) and all(bool(r.any()) and not bool(r.all()) for r in live.reshape(7, 24)[:6])


def test_every_sample_far(renderers, monkeypatch):
    """A depth range far behind the hand: the live part of the ordered list is empty."""
    ren = renderers('f16x3', 24)
    o, d = mixed_rays()
    tr = torch.rand(7, 1, generator=torch.Generator().manual_seed(2))
    out = off_and_on(ren, o, d, 3.0, 4.0, tr, monkeypatch)
    assert not bool(live_mask(o, d, out['z_vals'], 3.0, 4.0, 24).any())


def test_every_sample_live(renderers, monkeypatch):
    """A depth range hugging the wrist joint: the far part of the ordered list is empty."""
    ren = renderers('f16x3', 24)
    o, d = wrist_rays(7)
    r = depth_of(JOINTS[0])
    tr = torch.rand(7, 1, generator=torch.Generator().manual_seed(3))
    out = off_and_on(ren, o, d, r - 0.05, r + 0.05, tr, monkeypatch)
    assert bool(live_mask(o, d, out['z_vals'], r - 0.05, r + 0.05, 24).all())


def test_one_ray_two_samples(renderers, monkeypatch):
    """1 ray x 2 samples, the first one 1 cm from the wrist joint (live), the second one 0.75 behind it (far)."""
    ren = renderers('f16x3', 2)
    target = JOINTS[0] + np.float32([0.01, 0.0, 0.0])
    o, d = rays_through(target[None])
    r = depth_of(target)
    tr = torch.full((1, 1), 0.5)
    out = off_and_on(ren, o, d, r - 0.5, r + 0.5, tr, monkeypatch)
    assert live_mask(o, d, out['z_vals'], r - 0.5, r + 0.5, 2).tolist() == [True, False]


def test_compaction_on_equals_compaction_off(renderers, monkeypatch):
    """The far-field skip (hn_field_set_compaction) is a path of its own, taken from 4096 samples: 32 rays x 128 samples through it equal
    the dense render in either order.  (32 rays, because `gradient_error` is a sum that the compositing kernel's blocks add with one
    float atomic each, 16 rays of 128 samples per block: two addends give the same bits in either order of arrival, three or more do
    not -- from run to run of the SAME launches.  Every case of this file stays within two blocks, so that `torch.equal` can be asked of
    every returned array.)"""
    ren = renderers('f16x3', 128)
    g = torch.Generator().manual_seed(4)
    through = JOINTS[torch.randint(0, 21, (32,), generator=g).numpy()] + (0.03 * torch.randn(32, 3, generator=g)).numpy().astype(np.float32)
    o, d = rays_through(through)
    tr = torch.rand(32, 1, generator=g)
    dense = off_and_on(ren, o, d, 0.4, 1.5, tr, monkeypatch)
    live = live_mask(o, d, dense['z_vals'], 0.4, 1.5, 128)
    assert live.numel() == 4096 and 0 < int(live.sum()) < 4096
    ren.compact_far_field = True
    try:
        for mode in ('0', '2'):
            assert_same(dense, render(ren, o, d, 0.4, 1.5, tr, monkeypatch, mode), 'compaction on (HONERF_LIVE_FIRST=%s) / off' % mode)
    finally:
        ren.compact_far_field = False
