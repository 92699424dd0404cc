#!/usr/bin/env python3
"""Generate tests/golden/vgg_loss.npz by importing the REFERENCE's own VGGLoss (utils/fields.py:407-433) on CPU.  Run where the
reference tree is present (HONERF_REFERENCE, default /root/reference):

    python tests/golden/make_golden_vgg.py

torchvision is not installed here and its pretrained file is not ours to ship, so `torchvision.models.vgg19(pretrained=True).features`
is stubbed with the 37-module layout of VGG19's `features` (configuration E: 16 3x3 convolutions with ReLU, 5 pools) at 1/16 of its
width -- 4, 8, 16, 32, 32 channels -- with seeded weights (randn sqrt(2 / (9 Cin)), biases 0.1 randn: activations neither die nor
grow).  Everything VGGLoss itself does -- the slicing by feature_layers, the no_grad on the target, the L1 means, their sum -- is the
reference's statements, unmodified; the image is built with exp_runner.py:229-230's reshape / permute.

Stored: the weights under torchvision's state-dict names; per case (21 x 21: n0 = n1 = 21; 18 x 23: reshape(18, 23, 3)) color_fine and
true_rgb [P, 3], and in float32 and float64 the reference's loss, the five per-tap L1 means (its own `layers` and `criterion`) and
autograd's d loss / d color_fine.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('HONERF_REFERENCE', '/root/reference')
sys.dont_write_bytecode = True

CFG_E = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M')
WIDTH_DIVISOR = 16


def narrow_vgg19_features(seed=0):
    g = torch.Generator().manual_seed(seed)
    mods, cin = [], 3
    for v in CFG_E:
        if v == 'M':
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(cin, v // WIDTH_DIVISOR, kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * float(np.sqrt(2.0 / (9 * cin))))
            conv.bias.copy_(0.1 * torch.randn(conv.bias.shape, generator=g))
        mods += [conv, nn.ReLU(inplace=True)]
        cin = v // WIDTH_DIVISOR
    assert len(mods) == 37
    return nn.Sequential(*mods)


FEATURES = narrow_vgg19_features()
tv = types.ModuleType('torchvision')
tv.models = types.ModuleType('torchvision.models')
tv.models.vgg19 = lambda pretrained=False: types.SimpleNamespace(features=FEATURES)
sys.modules['torchvision'] = tv
sys.modules['torchvision.models'] = tv.models
sys.path.insert(0, REF)

import utils.fields as rf      # noqa: E402  (reference)


def main():
    torch.set_num_threads(4)
    out = {'features.' + k: v.detach().numpy().copy() for k, v in FEATURES.state_dict().items()}
    assert 'features.28.weight' in out and 'features.34.bias' in out
    ref = rf.VGGLoss('cpu')
    g = torch.Generator().manual_seed(1)
    for name, n0, n1 in (('21x21', 21, 21), ('18x23', 18, 23)):
        P = n0 * n1
        color = torch.rand(P, 3, generator=g)
        true = (color + 0.1 * torch.randn(P, 3, generator=g)).clamp(0.0, 1.0)
        out[name + '.n0n1'] = np.array([n0, n1])
        out[name + '.color_fine'], out[name + '.true_rgb'] = color.numpy(), true.numpy()
        for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
            ref = ref.to(dtype)
            c = color.detach().to(dtype).clone().requires_grad_(True)
            pred_img = c.reshape((n0, n1, 3)).permute(2, 1, 0).unsqueeze(0)                   # exp_runner.py:229
            gt_img = true.to(dtype).reshape((n0, n1, 3)).permute(2, 1, 0).unsqueeze(0)        # :230
            loss = ref(pred_img, gt_img)
            loss.backward()
            means, s, t = [], pred_img.detach(), gt_img
            for layer in ref.layers:
                s, t = layer(s), layer(t)
                means.append(float(ref.criterion(s, t)))
            out['%s.loss%s' % (name, tag)] = np.array(float(loss.detach()))
            out['%s.means%s' % (name, tag)] = np.array(means)
            out['%s.grad%s' % (name, tag)] = c.grad.numpy().copy()
            print(name, tag, 'loss %.9f' % float(loss), 'means', ' '.join('%.6f' % m for m in means), 'max |grad| %.3e' % float(c.grad.abs().max()))
    path = os.path.join(HERE, 'vgg_loss.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
