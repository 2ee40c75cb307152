"""Times the task-affinity protocol's linear probe (--task_affinity) on both backends and prints ONE JSON line.

Synthetic features: --n rows (default 8192) x 1024, 55 unit-variance Gaussian classes around random means of scale
--scale; the reference's recipe (300 epochs of floor(n / 64) batches, AdamW 1e-3 / 0.05, cosine schedule).  The initial
values and the permutations are drawn once, before anything is timed, and given to both backends.  Each backend is a child
process under its own time limit; the first one that fails ends the run (nothing more is started on the GPU after a
fault or a time-out).

  hip     affinity_ops.train_linear_probe (csrc/affinity.hip: one launch per step)
  torch   affinity_ops.torch_train_linear_probe (PDAE_AFFINITY=torch: the reference's loop as framework ops on the device)

HIP events around the whole call -- no event per step and no host synchronisation inside --, one warm-up call of
--warmup-epochs epochs, then --repeats timed calls: the median, the smallest and the largest are reported.

    python tools/bench_affinity.py [--backends hip,torch] [--n 8192] [--epochs 300] [--repeats 3] [--limit 600]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, CLASSES = 1024, 55


def child(args):
    import numpy as np
    import torch
    from point_dae_amd import affinity_ops
    rng = np.random.default_rng(0)
    means = rng.standard_normal((CLASSES, DIM)) * args.scale
    y = rng.integers(0, CLASSES, args.n)
    X = torch.from_numpy((means[y] + rng.standard_normal((args.n, DIM))).astype(np.float32)).cuda()
    torch.manual_seed(0)
    init = affinity_ops.draw_init(DIM, CLASSES)
    perms = affinity_ops.draw_perms(args.n, args.epochs)
    fn = affinity_ops.train_linear_probe if args.child == 'hip' else affinity_ops.torch_train_linear_probe

    def timed(epochs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(X, y, CLASSES, epochs=epochs, init=init, perms=perms[:epochs])
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out
    timed(min(args.warmup_epochs, args.epochs))
    ms = []
    for _ in range(args.repeats):
        t, out = timed(args.epochs)
        ms.append(t)
    W = out[0] if args.child == 'hip' else out.weight
    steps = args.epochs * (args.n // 64)
    print(json.dumps(dict(backend=args.child, n=args.n, D=DIM, K=CLASSES, epochs=args.epochs, steps=steps,
                          ms=[round(t, 1) for t in ms], median_ms=round(float(np.median(ms)), 1),
                          us_per_step=round(float(np.median(ms)) * 1e3 / max(steps, 1), 2),
                          w_norm=float(W.detach().double().norm()))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--backends', default='hip,torch')
    p.add_argument('--n', type=int, default=8192)
    p.add_argument('--epochs', type=int, default=300)
    p.add_argument('--warmup-epochs', type=int, default=5)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--scale', type=float, default=0.06)
    p.add_argument('--limit', type=int, default=600, help='seconds per child')
    p.add_argument('--child', default=None)
    args = p.parse_args()
    if args.child:
        return child(args)
    result = {}
    for name in args.backends.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--n', str(args.n), '--epochs', str(args.epochs),
               '--warmup-epochs', str(args.warmup_epochs), '--repeats', str(args.repeats), '--scale', str(args.scale)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            result[name] = dict(error='time limit of %d s' % args.limit)
            break
        if r.returncode != 0:
            result[name] = dict(error='exit status %d' % r.returncode, stderr=r.stderr[-1000:])
            break
        result[name] = json.loads(r.stdout.strip().splitlines()[-1])
    if 'median_ms' in result.get('hip', {}) and 'median_ms' in result.get('torch', {}):
        result['torch_over_hip'] = round(result['torch']['median_ms'] / result['hip']['median_ms'], 2)
    print(json.dumps(result))
    return 0 if all('error' not in v for v in result.values() if isinstance(v, dict)) else 1


if __name__ == '__main__':
    sys.exit(main())
