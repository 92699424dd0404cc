"""analys_results/analys_psnr_ssim_lpips.py on the device: PSNR, SSIM and, given the weights, LPIPS (VGG) of the held-out renders of
a fit against the ground-truth images.

Walks the reference's tree (:52-70): the ground-truth images are `gt_path/<obj>/<frame>/MASK/<file>`, the renders
`ours_path/<fit>/<obj>/<frame>/render_<fit>/<file>` (the file of the same stem; `harness.render_views` + `harness.write_image`
write them).  Files whose view name, `name.split('.')[0].split('_')[1]`, is one of the training views are skipped (:58-60).  Images
of equal size go through `honerf_amd.image_metrics.image_metrics` in one call.  Prints the number of images, the reference's header
line and the means (:75-82); `--json` writes the per-file values keyed `obj+frame+file` (:66).  The lpips column needs the pretrained
weights, which are not part of this repository: `--lpips-weights BACKBONE [LIN]` names a torch.save'd state dict of VGG16
(torchvision's `vgg16`, its `.features`, or a whole `lpips.LPIPS(net='vgg')`) and, unless that file holds them too, lpips' linear
layers (`lin<k>.model.1.weight`); see `honerf_amd.image_metrics.LpipsVgg`.  Without the option the header and the means have two
columns.  A render that is missing for a ground-truth file is an error naming the file.  `.ppm` files are read by
`harness.read_image` itself, anything else needs PIL.  Needs a GPU.

    python tools/image_eval.py <gt_path> <ours_path> [--fit-type 12] [--train-views 21320027 21320030 21320035] [--json FILE]
                               [--lpips-weights BACKBONE [LIN]]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRAIN_VIEWS = ['21320027', '21320030', '21320035']        # analys_psnr_ssim_lpips.py:39
BATCH_BYTES = 256 << 20                                   # images of one size per device call


def view_of(file_name):
    parts = file_name.split('.')[0].split('_')
    if len(parts) < 2:
        raise SystemExit('image_eval: %s: no view name (expected <prefix>_<view>[...].<ext>)' % file_name)
    return parts[1]


def render_of(render_dir, file_name):
    """The render of a ground-truth file: the same name, else the one file of the same stem."""
    exact = os.path.join(render_dir, file_name)
    if os.path.isfile(exact):
        return exact
    stem = os.path.splitext(file_name)[0]
    same = sorted(n for n in os.listdir(render_dir) if os.path.splitext(n)[0] == stem) if os.path.isdir(render_dir) else []
    if len(same) != 1:
        raise SystemExit('image_eval: %s render for %s under %s' % ('no' if not same else 'more than one', file_name, render_dir))
    return os.path.join(render_dir, same[0])


def pairs_of(gt_path, ours_path, fit, train_views):
    """[(key, gt file, render file)] in sorted order of the tree."""
    out = []
    for obj in sorted(os.listdir(gt_path)):
        obj_path = os.path.join(gt_path, obj)
        if not os.path.isdir(obj_path):
            continue
        for frame in sorted(os.listdir(obj_path)):
            mask_path = os.path.join(obj_path, frame, 'MASK')
            if not os.path.isdir(mask_path):
                continue
            for name in sorted(os.listdir(mask_path)):
                if view_of(name) in train_views:
                    continue
                ours = render_of(os.path.join(ours_path, fit, obj, frame, 'render_' + fit), name)
                out.append((obj + '+' + frame + '+' + name, os.path.join(mask_path, name), ours))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('gt_path')
    ap.add_argument('ours_path')
    ap.add_argument('--fit-type', default='12')
    ap.add_argument('--train-views', nargs='*', default=TRAIN_VIEWS)
    ap.add_argument('--json', default=None, help='write the per-file values here')
    ap.add_argument('--lpips-weights', nargs='+', default=None, metavar='FILE', help='VGG16 state dict [and the linear layers]: adds the lpips column')
    args = ap.parse_args()
    if args.lpips_weights is not None and len(args.lpips_weights) > 2:
        ap.error('--lpips-weights takes one or two files')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('image_eval: no GPU')
    from honerf_amd import harness
    from honerf_amd.image_metrics import LpipsVgg, image_metrics
    model = LpipsVgg.load(*args.lpips_weights) if args.lpips_weights is not None else None
    pairs = pairs_of(args.gt_path, args.ours_path, str(args.fit_type), set(args.train_views))
    if not pairs:
        raise SystemExit('image_eval: no held-out image under %s' % args.gt_path)
    psnr, ssim, lpips = np.empty(len(pairs)), np.empty(len(pairs)), np.empty(len(pairs))
    by_shape = {}
    for i, (key, gt_file, our_file) in enumerate(pairs):
        g, o = harness.read_image(gt_file), harness.read_image(our_file)
        if g.shape != o.shape:
            raise SystemExit('image_eval: %s is %s and %s is %s' % (gt_file, g.shape, our_file, o.shape))
        by_shape.setdefault(g.shape, []).append((i, o, g))

    def flush(batch):
        m = image_metrics(np.stack([o for _, o, _ in batch]), np.stack([g for _, _, g in batch]), lpips=model)
        idx = [i for i, _, _ in batch]
        psnr[idx], ssim[idx] = m['psnr'], m['ssim']
        if model is not None:
            lpips[idx] = m['lpips']

    for shape, items in by_shape.items():
        per_call = max(1, BATCH_BYTES // int(np.prod(shape)))
        for s in range(0, len(items), per_call):
            flush(items[s:s + per_call])
    print(len(pairs))
    if model is None:
        print('     psnr,     ssim')
        print('ours:  %.4f %.6f' % (psnr.mean(), ssim.mean()))
    else:
        print('     psnr,     ssim,     lpips')
        print('ours:  %.4f %.6f %.6f' % (psnr.mean(), ssim.mean(), lpips.mean()))
    if args.json:
        extra = (lambda i: dict(lpips=float(lpips[i]))) if model is not None else (lambda i: {})
        with open(args.json, 'w') as f:
            json.dump({key: dict(psnr=float(psnr[i]), ssim=float(ssim[i]), **extra(i)) for i, (key, _, _) in enumerate(pairs)}, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
