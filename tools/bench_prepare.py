"""python tools/bench_prepare.py -- the fine-tuning batch preparation at B=32, P=8192 -> 1200 -> 1024:
FPS alone, (a) resample(), (b) resample() + the reference's per-cloud transform loop in torch ops,
(c) resample_transformed(..., PointcloudRotate(), out=buf).  Rounds alternate a, b, c, fps; every figure = host clock
around ITERS calls ending in a device synchronise, per call; then the host time to issue one call."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from point_dae_amd.data_transforms import PointcloudRotate, resample_transformed
from point_dae_amd.graph_step import use_created_stream
from point_dae_amd.pointnet2_utils import furthest_point_sample
from point_dae_amd.runner_finetune import resample
from point_dae_amd.synthetic import shapenet_like_clouds

B, P, NP, ITERS, ROUNDS = 32, 8192, 1024, 100, 7
torch.cuda.set_device(0)
use_created_stream(torch.device('cuda', 0))
pts = torch.from_numpy(shapenet_like_clouds(B, P, seed=1)).cuda()
buf = torch.zeros(B, NP, 3, device='cuda')
rot = PointcloudRotate()


def ref_rotate(pc):                      # the reference's loop, datasets/data_transforms.py:6-18
    for i in range(pc.size(0)):
        a = np.random.uniform() * 2 * np.pi
        c, s = np.cos(a), np.sin(a)
        R = torch.from_numpy(np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).astype(np.float32)).to(pc.device)
        pc[i, :, :] = torch.matmul(pc[i], R)
    return pc


def fps_only():
    return furthest_point_sample(pts, 1200)

def a():
    return resample(pts, NP)

def b():
    return ref_rotate(resample(pts, NP))

def c():
    return resample_transformed(pts, NP, rot, out=buf)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e3

def host_enqueue(fn):
    """host time per call to ISSUE the work (no synchronise inside the window; the device drains afterwards)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    dt = (time.perf_counter() - t0) / ITERS * 1e3
    torch.cuda.synchronize()
    return dt

# same seeded inputs: (c) against (b) within rounding, identity against (a) bit for bit
np.random.seed(3); xb = b()
np.random.seed(3); xc = c().clone()
np.random.seed(3); xa = a()
np.random.seed(3); xi = resample_transformed(pts, NP)
print('max |c - b| =', (xc - xb).abs().max().item(), ' identity == a:', torch.equal(xa, xi), flush=True)
fns = dict(a=a, b=b, c=c, fps=fps_only)
for f in fns.values():
    for _ in range(20):
        f()
res = {k: [] for k in fns}
for r in range(ROUNDS):
    for k, f in fns.items():
        res[k].append(timed(f))
    print('round', r, {k: round(v[-1], 4) for k, v in res.items()}, flush=True)
host = {k: [host_enqueue(f) for _ in range(3)] for k, f in fns.items()}
print('host enqueue ms per call:', {k: [round(x, 4) for x in v] for k, v in host.items()}, flush=True)
summary = {k: dict(min=min(v), median=float(np.median(v)), max=max(v)) for k, v in res.items()}
print(json.dumps(summary, indent=1))
