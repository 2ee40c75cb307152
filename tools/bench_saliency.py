"""Input-point gradients at the fine-tuning shape: B = 32 clouds of N = 1024 points, G = 64 groups, depth 12 (the
config's PointTransformer, scratch weights, eval mode, every parameter frozen).  Three variants of
saliency_ops.input_gradients (one eval forward + one data-only backward), DESIGN.md §7:

    hip                 PDAE_SALIENCY=hip: the model's own chain, weight gradients skipped
    torch               PDAE_SALIENCY=torch: grouping, embedder and position embedding as framework ops under autograd
    hip, wgrad kept     hip with rows.SKIP_FROZEN_WGRAD off: the backward still issues every weight gradient

The variants are warmed up and then alternated ROUNDS times; a figure is CALLS calls inside one host-clock window that
ends in a device synchronise, divided by CALLS.  One line per window, a RESULT line per variant, and the number of
library launches of one hip backward (every C entry the backward calls, counted through _lib.CALL_HOOK).

    python tools/bench_saliency.py [ROUNDS] [CALLS] [B]
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from point_dae_amd import _lib, builder, rows, saliency_ops  # noqa: E402
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.graph_step import use_created_stream  # noqa: E402
from point_dae_amd.synthetic import labelled_clouds  # noqa: E402

CFG = 'cfgs/finetune_modelnet_transferring_features.yaml'


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    if not torch.cuda.is_available():
        raise RuntimeError('bench_saliency needs an MI355X: there is no CPU path')
    use_created_stream()
    config = cfg_from_yaml_file(os.path.join(ROOT, CFG))
    torch.manual_seed(0)
    model = builder.model_builder(config.model)
    model.load_model_from_ckpt(None, log=lambda *a: None)
    model = model.cuda().eval()
    for p in model.parameters():
        p.requires_grad_(False)
    x, y = labelled_clouds(B, config.npoints, seed=1, classes=3)
    pts, labels = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    print('B %d N %d G %d depth %d' % (B, config.npoints, config.model.num_group, config.model.depth), flush=True)

    def run(backend, skip, n):
        os.environ['PDAE_SALIENCY'] = backend
        rows.SKIP_FROZEN_WGRAD = skip
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            _, grad = saliency_ops.input_gradients(model, pts, labels)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n, grad

    variants = [('hip', 'hip', True), ('torch', 'torch', True), ('hip, wgrad kept', 'hip', False)]
    grads = {}
    for label, backend, skip in variants:
        dt, grads[label] = run(backend, skip, 3)
        print('warm-up', label, '%.3f ms' % (dt * 1e3), flush=True)
    ref = grads['hip'].double()
    for label in ('torch', 'hip, wgrad kept'):
        print('gradient of %r against hip: rel-L2 %.3e' % (label, float((grads[label].double() - ref).norm() / ref.norm())),
              flush=True)
    times = {label: [] for label, _, _ in variants}
    for r in range(rounds):
        for label, backend, skip in variants:
            dt, _ = run(backend, skip, calls)
            times[label].append(dt)
            print('round %d' % r, label, '%.3f ms' % (dt * 1e3), flush=True)
    for label, v in times.items():
        s = sorted(v)
        print('RESULT', label, 'median %.3f ms' % (s[len(s) // 2] * 1e3), 'min %.3f max %.3f' % (s[0] * 1e3, s[-1] * 1e3),
              flush=True)
    faster = all(h < t for h, t in zip(times['hip'], times['torch']))
    print('hip faster than torch in every round: %s' % faster, flush=True)

    # the launches of one backward: library entries, counted from the first one after the forward returns
    for label, skip in (('hip', True), ('hip, wgrad kept', False)):
        os.environ['PDAE_SALIENCY'], rows.SKIP_FROZEN_WGRAD = 'hip', skip
        x_in = pts.clone().requires_grad_()
        logits = model(x_in)
        seen = []
        _lib.CALL_HOOK = lambda name, args: seen.append(name)
        try:
            logits.backward(torch.zeros_like(logits).scatter_(1, labels[:, None], 1.0))
        finally:
            _lib.CALL_HOOK = None
        print('LAUNCHES backward (%s): %d library entries' % (label, len(seen)), flush=True)
    rows.SKIP_FROZEN_WGRAD = True


if __name__ == '__main__':
    main()
