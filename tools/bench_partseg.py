"""PointTransformerPartSeg's evaluation forward at the shipping shapes (cfgs/segmentation_shapenetpart_transformer.yaml), B
clouds of N points, seeded weights, eval mode -- the figures of DESIGN.md §7:

    forward   the whole forward (trunk + head) under PDAE_PARTSEG=hip (csrc/partseg.hip: the first layer's feature
              columns once per token, the global columns once per cloud, one tail pass) against PDAE_PARTSEG=layers (the
              head as the reference writes it, on kernels that predate csrc/partseg.hip plus framework glue)
    head      partseg_ops.head alone on a precomputed trunk output, both forms, with the metric's counts
    trunk     grouping, the patch embedder, the blocks up to the last tap (the same code under both forms)

The two forms of a pair are warmed up and then alternated ROUNDS times; a figure is CALLS calls between two device
events, divided by CALLS; (median, min, max) over the rounds, in ms.  The outputs of the two forms are compared at the
timed size first.  One JSON object per batch size.

    python tools/bench_partseg.py [ROUNDS] [B ...]          # default 7 rounds at B = 16, N = 2048
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import weights  # noqa: E402
from point_dae_amd import builder  # noqa: E402,F401
from point_dae_amd import partseg_ops  # noqa: E402
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.datasets import synthetic_part_shapes  # noqa: E402
from point_dae_amd.graph_step import use_created_stream  # noqa: E402
from point_dae_amd.registry import MODELS  # noqa: E402

N = 2048


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def alternate(fns, calls, rounds, warm=2):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for fn, acc in zip(fns, times):
            acc.append(window(fn, calls))
    return [(round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)) for t in times]


def under(mode, fn):
    def run():
        os.environ['PDAE_PARTSEG'] = mode
        return fn()
    return run


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@torch.no_grad()
def bench(B, rounds, model):
    clouds, cls, segs = synthetic_part_shapes(B, N, seed=3)
    pts = torch.stack([torch.from_numpy(c[:N]) for c in clouds]).cuda()
    seg = torch.stack([torch.from_numpy(s[:N]) for s in segs]).cuda()
    cls = torch.from_numpy(cls).cuda()
    out = {'B': B, 'N': N, 'rounds': rounds}
    hip, layers = under('hip', lambda: model(pts, cls)), under('layers', lambda: model(pts, cls))
    out['forward_hip_vs_layers_rel'] = rel(hip(), layers())
    out['forward_hip_ms'], out['forward_layers_ms'] = alternate([hip, layers], 3, rounds)
    out['forward_speedup'] = round(out['forward_layers_ms'][0] / out['forward_hip_ms'][0], 2)
    out['clouds_per_s_hip'] = round(B / (out['forward_hip_ms'][0] * 1e-3), 1)
    out['clouds_per_s_layers'] = round(B / (out['forward_layers_ms'][0] * 1e-3), 1)
    center, F = model.trunk(pts)
    center, F = center.clone(), F.clone()
    counts = partseg_ops.Counts(B, pts.device)

    def head():
        counts.filled = 0
        return partseg_ops.head(model, pts, center, F, cls, seg, counts)
    a, b = under('hip', head)(), under('layers', head)()
    out['head_hip_vs_layers_rel'] = rel(a[0], b[0])
    out['head_pred_agreement'] = float((a[1] == b[1]).double().mean())
    out['head_hip_ms'], out['head_layers_ms'] = alternate([under('hip', head), under('layers', head)], 5, rounds)
    out['head_speedup'] = round(out['head_layers_ms'][0] / out['head_hip_ms'][0], 2)
    out['trunk_ms'] = alternate([lambda: model.trunk(pts)], 3, rounds)[0]
    print(json.dumps(out), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    sizes = [int(a) for a in sys.argv[2:]] or [16]
    use_created_stream()
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'segmentation_shapenetpart_transformer.yaml')).model
    model = weights.fill_state(MODELS.build(cfg), 7).cuda().eval()
    for B in sizes:
        bench(B, rounds, model)


if __name__ == '__main__':
    main()
