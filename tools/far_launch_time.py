"""Event-timed hn_field_eval over all-far sample lists: every tile takes the all-far tile program of the hand kernel.
256 tiles (32 768 points) per round; per round count the median of N launches between two events.  One process per library:
   HONERF_LIB=<library> python tools/far_launch_time.py <label> [rounds ...]      (default rounds: 1 8 64)"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np, torch
from helpers import *
from honerf_amd.nets import PackedField
from honerf_amd import lib as L, synth
label = sys.argv[1] if len(sys.argv) > 1 else 'lib'
rounds = [int(x) for x in sys.argv[2:]] or [1, 8, 64]
lib = L.load()
m = product_modules()
f = PackedField('hand', m['sdf_hand'], m['color_hand'], m['var_hand'], precision=os.environ.get('PRECISION', 'f16x3'))
bt_inv, T_pose, joints = synth.synth_hand_pose(5)
bt, tp = torch.from_numpy(bt_inv).cuda().reshape(1, 21, 4, 4), torch.from_numpy(T_pose).cuda().reshape(1, 21, 3)
gen = torch.Generator().manual_seed(3)
for r in rounds:
    n = 32768 * r
    p = (torch.from_numpy(joints).mean(0) + torch.tensor([0.0, 0.0, 1.25]) + 0.05 * torch.rand(n, 3, generator=gen)).cuda()
    d = torch.nn.functional.normalize(torch.randn(n // 64, 3, generator=gen), dim=-1).cuda()
    sdf, grad, rgb = torch.empty(n, device='cuda'), torch.empty(n, 3, device='cuda'), torch.empty(n, 3, device='cuda')
    wsb = lib.hn_field_workspace_bytes(f.handle, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    def full():
        L.check(lib.hn_field_eval(f.handle, L.ptr(p), L.ptr(d), n, 64, L.ptr(bt), L.ptr(tp), 1, n, L.ptr(sdf), L.ptr(grad), L.ptr(rgb), None,
                                  L.ptr(ws), wsb, L.stream_ptr()), 'eval')
    for _ in range(3): full()
    torch.cuda.synchronize()
    assert bool((grad == 0).all()) and bool((sdf == sdf[0]).all()), 'the points are not all far'
    ms = []
    for _ in range(7 if r >= 64 else 15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); full(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print('%-10s rounds %3d  median %.4f ms  min %.4f  max %.4f  per round %.4f ms' % (label, r, np.median(ms), min(ms), max(ms), np.median(ms) / r), flush=True)
