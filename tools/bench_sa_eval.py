"""PointNetv2_feat feature extraction at the shipping shapes (cfgs/finetune_modelnet_svm_pointnetv2.yaml), B clouds of 1024
points, seeded weights, eval mode -- the figures of DESIGN.md §7:

    feature       the whole forward under PDAE_SA_EVAL=hip (one pdae_sa_eval_forward per grouped level, csrc/sa_eval.hip)
                  against PDAE_SA_EVAL=layers (the layer-by-layer form: grouped rows, three row GEMMs with framework
                  BatchNorm + ReLU, a framework max)
    level1..3     each set-abstraction module alone on the previous level's output, both forms; FPS and the ball query
                  run in both, and `geometry` times them alone
    kernel1/2     the level's dense part alone under hip: sa_eval_ops.level on precomputed indices
    transformer   PointTransformerNoClassTokenSVMFeature (cfgs/finetune_modelnet_svm_transformer.yaml): clouds per second

The two forms of a pair are warmed up and then alternated ROUNDS times; a figure is CALLS calls inside one host-clock
window that ends in a device synchronise, divided by CALLS; (median, min, max) over the rounds, in ms.  One JSON object
per batch size.

    python tools/bench_sa_eval.py [ROUNDS] [B ...]          # default 7 rounds at B = 32 and 128
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import weights  # noqa: E402
from point_dae_amd import builder  # noqa: E402,F401
from point_dae_amd import sa_eval_ops  # noqa: E402
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.graph_step import use_created_stream  # noqa: E402
from point_dae_amd.pointnet2_utils import ball_query, furthest_point_sample_with_centres  # noqa: E402
from point_dae_amd.registry import MODELS  # noqa: E402
from point_dae_amd.synthetic import shapenet_like_clouds  # noqa: E402


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


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
        os.environ['PDAE_SA_EVAL'] = mode
        return fn()
    return run


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def build(cfg):
    return weights.fill_state(MODELS.build(cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', cfg)).model), 7).cuda().eval()


@torch.no_grad()
def bench(B, rounds, model, transformer):
    pts = torch.from_numpy(shapenet_like_clouds(B, 1024, seed=3)).cuda()
    enc = model.pointnetv2_encoder
    out = {'B': B, 'rounds': rounds}
    hip, layers = under('hip', lambda: model(pts)), under('layers', lambda: model(pts))
    out['feature_hip_vs_layers_rel'] = rel(hip(), layers())
    out['feature_hip_ms'], out['feature_layers_ms'] = alternate([hip, layers], 3, rounds)
    out['speedup'] = round(out['feature_layers_ms'][0] / out['feature_hip_ms'][0], 2)
    out['clouds_per_s_hip'] = round(B / (out['feature_hip_ms'][0] * 1e-3), 1)
    out['clouds_per_s_layers'] = round(B / (out['feature_layers_ms'][0] * 1e-3), 1)
    xyz, feats = pts, None
    for lvl, sa in enumerate((enc.sa1, enc.sa2, enc.sa3), 1):
        a, b = alternate([under('hip', lambda: sa(xyz, feats)), under('layers', lambda: sa(xyz, feats))], 3, rounds)
        out['level%d_hip_ms' % lvl], out['level%d_layers_ms' % lvl] = a, b
        if sa.npoint is not None:
            def geometry():
                _, c = furthest_point_sample_with_centres(xyz, sa.npoint)
                return c, ball_query(sa.radius, sa.nsample, xyz, c)
            new_xyz, idx = geometry()
            out['geometry%d_ms' % lvl] = alternate([geometry], 3, rounds)[0]
            out['kernel%d_hip_ms' % lvl] = alternate(
                [lambda: sa_eval_ops.level(xyz, new_xyz, idx, feats, list(sa.mlps[0]))], 5, rounds)[0]
        os.environ['PDAE_SA_EVAL'] = 'hip'
        xyz, feats = sa(xyz, feats)
    out['transformer_feature_ms'] = alternate([lambda: transformer(pts)], 3, rounds)[0]
    out['transformer_clouds_per_s'] = round(B / (out['transformer_feature_ms'][0] * 1e-3), 1)
    print(json.dumps(out), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    sizes = [int(a) for a in sys.argv[2:]] or [32, 128]
    use_created_stream()
    model = build('finetune_modelnet_svm_pointnetv2.yaml')
    transformer = build('finetune_modelnet_svm_transformer.yaml')
    for B in sizes:
        bench(B, rounds, model, transformer)


if __name__ == '__main__':
    main()
