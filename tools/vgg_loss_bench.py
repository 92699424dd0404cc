"""Times of the device VGG19 perceptual loss (hn_vggloss.hip + hn_conv3x3.h through honerf_amd.training.VggLoss), forward + backward on one
`--side` x `--side` patch (21: the confs' 441 rays), against the same loss written with torch operators in float32 on the device
(`training.vgg_loss_reference`: F.conv2d, F.max_pool2d, F.l1_loss and autograd -- the path a user had through `extra_loss` before),
alternating in one process; and of `training.train_step` on the object nets at side^2 rays with no extra loss, with the torch term and
with the device term.  The weights are seeded random numbers (randn sqrt(2 / (9 Cin)), biases 0.1 randn): the times do not depend on
their values.

Device events around windows of `--iters` calls after `--warmup` untimed calls of each arm; min / median / max per call over `--windows`
(5) alternating windows.  Beside the loss's times: the bytes of packed weights one forward + backward pair streams (taps outside the
image are not read) over the median time, next to the HBM peak -- the time is event to event, launch gaps included, so this is a
lower bound of what the kernels reach.  `accepted`: the device arm's median does not exceed the torch arm's, for the loss alone and
inside train_step.  If torch's convolution cannot run on the device, that is recorded instead of a time.  Needs a GPU.

    python tools/vgg_loss_bench.py [--side 21] [--iters 20] [--windows 5] [--warmup 5] [--out profiles/vgg_loss/vgg_loss_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TB_S = 8.0            # MI355X, 8 stacks of HBM3E


def make_state(seed=0):
    from honerf_amd.training import VGG19_CONV_COUT, VGG19_CONV_INDEX
    g = torch.Generator().manual_seed(seed)
    sd, ci = {}, 3
    for i, co in zip(VGG19_CONV_INDEX, VGG19_CONV_COUT):
        sd['features.%d.weight' % i] = torch.randn(co, ci, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * ci)))
        sd['features.%d.bias' % i] = 0.1 * torch.randn(co, generator=g)
        ci = co
    return sd


def weight_bytes(side):
    """Bytes of packed weights one forward and one backward pass read at side x side: per layer Cout x Cin (padded as packed) x live taps."""
    from honerf_amd.training import VGG19_CONV_COUT, VGG19_POOL_BEFORE
    fwd = bwd = 0
    s, ci = side, 3
    for l, co in enumerate(VGG19_CONV_COUT):
        if l in VGG19_POOL_BEFORE:
            s //= 2
        live = 9 if s > 1 else 1
        fwd += co * (32 if l == 0 else live * ci) * 4
        bwd += max(ci, 64) * live * co * 4
        ci = co
    return fwd, bwd


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters, out


def race(arms, iters, windows, warmup):
    """Alternating windows -> {arm: per-call ms of each window}, {arm: last value}; an arm that raises is dropped with its message."""
    times, last, failed = {k: [] for k in arms}, {}, {}
    for name, fn in list(arms.items()):
        try:
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
        except Exception as exc:      # (torch's convolution backend missing or refusing the shape: recorded, not fatal)
            failed[name] = '%s: %s' % (type(exc).__name__, str(exc)[:300])
            del arms[name], times[name]
    for _ in range(windows):
        for name, fn in arms.items():
            ms, last[name] = window(fn, iters)
            times[name].append(ms)
    return times, last, failed


def rows_of(times):
    return {k: dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), ms_all=t) for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--side', type=int, default=21)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vgg_loss', 'vgg_loss_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vgg_loss_bench: no GPU')
    if args.windows < 5:
        raise SystemExit('vgg_loss_bench: at least 5 windows')
    from honerf_amd import training
    from honerf_amd.nets import RenderingNetwork_OBJ, SDFNetwork_OBJ, SingleVarianceNetwork
    from honerf_amd.renderer import NeuSRenderer
    dev = torch.device('cuda:0')
    n, P = args.side, args.side * args.side
    sd = make_state()
    vgg = training.VggLoss(sd)
    w_dev, b_dev = [w.to(dev) for w in vgg.conv_weight], [b.to(dev) for b in vgg.conv_bias]
    g = torch.Generator().manual_seed(1)
    color = torch.rand(P, 3, generator=g).to(dev)
    true = (color.cpu() + 0.1 * torch.randn(P, 3, generator=g)).clamp(0.0, 1.0).to(dev)

    def torch_term(c, t):
        return training.vgg_loss_reference(w_dev, b_dev, training.patch_image(c, n, n), training.patch_image(t, n, n))[0]

    def loss_arm(term):
        def run():
            c = color.detach().requires_grad_(True)
            loss = term(c, true)
            loss.backward()
            return loss.detach(), c.grad
        return run

    arms = {'hip': loss_arm(lambda c, t: vgg.patch_loss(c, t)), 'torch_operators': loss_arm(torch_term)}
    times, last, failed = race(arms, args.iters, args.windows, args.warmup)
    rows = rows_of(times)
    fwd_b, bwd_b = weight_bytes(n)
    result = dict(tool='vgg_loss_bench', device=torch.cuda.get_device_name(0), side=n, iters=args.iters, windows=args.windows, warmup=args.warmup,
                  weight_bytes_forward=fwd_b, weight_bytes_backward=bwd_b, hbm_peak_tb_per_s=HBM_PEAK_TB_S, loss=rows, not_measured=failed)
    if 'hip' in rows:
        rows['hip']['weights_streamed_tb_per_s'] = (fwd_b + bwd_b) / (rows['hip']['ms_median'] * 1e-3) / 1e12
    if 'hip' in last and 'torch_operators' in last:
        (la, ga), (lb, gb) = last['hip'], last['torch_operators']
        result['loss_hip'], result['loss_torch_operators'] = float(la), float(lb)
        result['largest_gradient_difference_relative'] = float((ga - gb).abs().max() / gb.abs().max())
        result['loss_accepted'] = rows['hip']['ms_median'] <= rows['torch_operators']['ms_median']
    for name, r in rows.items():
        print('%-16s forward + backward, %d x %d | min %8.3f  median %8.3f  max %8.3f ms' % (name, n, n, r['ms_min'], r['ms_median'], r['ms_max']), flush=True)

    # train_step at side^2 rays: the object nets of the confs (64 + 64 samples), rays through the unit sphere
    sdf_net, col_net, var = SDFNetwork_OBJ().to(dev), RenderingNetwork_OBJ().to(dev), SingleVarianceNetwork(0.3).to(dev)
    sdf_net.reset_parameters(11)
    col_net.reset_parameters(12)
    ren = NeuSRenderer(sdf_net, var, col_net, 'obj', 64, 64, 0, 4, 1.0)
    opt = training.make_optimizer(ren, 1e-5)
    xs = torch.linspace(-0.5, 0.5, n)
    d = torch.stack([xs.repeat_interleave(n), xs.repeat(n), torch.ones(P)], -1)
    rays_d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    rays_o = torch.tensor([0.0, 0.0, -1.0]).expand(P, 3).contiguous().to(dev)
    mask, Ro, To = torch.ones(P, 1, device=dev), torch.eye(3, device=dev), torch.zeros(3, device=dev)

    def step_arm(extra):
        return lambda: training.train_step(ren, opt, rays_o, rays_d, 0.4, 1.5, None, None, Ro, To, true, mask, 1.0, 1.0, extra_loss=extra)['loss'].detach()

    step_arms = {'no_extra_loss': step_arm(None), 'hip_term': step_arm(training.vgg_extra_loss(vgg, true, 1.0, 1.0))}
    if 'torch_operators' in rows:
        step_arms['torch_term'] = step_arm(lambda out: torch_term(out['color_fine'], true))
    times, _, failed_step = race(step_arms, args.iters, args.windows, args.warmup)
    result['train_step'] = rows_of(times)
    result['not_measured'].update(failed_step)
    for name, r in result['train_step'].items():
        print('train_step %-14s %d rays | min %8.3f  median %8.3f  max %8.3f ms' % (name, P, r['ms_min'], r['ms_median'], r['ms_max']), flush=True)
    if 'hip_term' in result['train_step'] and 'torch_term' in result['train_step']:
        result['train_step_accepted'] = result['train_step']['hip_term']['ms_median'] <= result['train_step']['torch_term']['ms_median']
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
