"""Point-M2AE feature extraction at the shipping shapes (cfgs/finetune_modelnet_svm_pointm2ae.yaml), B clouds of 2048
points, seeded weights, eval mode -- the figures of DESIGN.md §7:

    embed0        the level-0 token embedder on B*512 patches of 16 points: point_m2ae.token_embed_points (second_conv's
                  products kept on chip) against patch_embed.patch_embed_layerwise with the BatchNorms in eval mode on the
                  same input (the route a 16-point patch took before)
    attn          pdae_attention_local_forward alone at the three levels' shapes
    feature       the whole forward (grouping included) against tests/m2ae_restatement.py in fp32 on the same GPU

Two variants of a pair are warmed up and then alternated ROUNDS times; a figure is CALLS calls inside one host-clock
window that ends in a device synchronise, divided by CALLS; (min, max) over the rounds are printed.  One JSON object.

    python tools/bench_m2ae.py [B] [ROUNDS]
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import m2ae_restatement as R  # noqa: E402
import weights  # noqa: E402
from point_dae_amd import builder  # noqa: E402,F401
from point_dae_amd import point_m2ae as PM  # noqa: E402
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.graph_step import use_created_stream  # noqa: E402
from point_dae_amd.patch_embed import patch_embed_layerwise  # noqa: E402
from point_dae_amd.registry import MODELS  # noqa: E402
from point_dae_amd.synthetic import shapenet_like_clouds  # noqa: E402

CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_svm_pointm2ae.yaml')


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
    return [(round(min(t), 3), round(max(t), 3)) for t in times]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@torch.no_grad()
def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    use_created_stream()
    model = weights.fill_state(MODELS.build(cfg_from_yaml_file(CFG).model), 7).cuda().eval()
    pts = torch.from_numpy(shapenet_like_clouds(B, 2048, seed=3)).cuda()
    out = {'B': B, 'rounds': rounds}
    nbs, cs, idxs = model.group(pts)
    te = model.h_encoder.token_embed[0]
    patches = nbs[0].reshape(B * 512, 16, 3).contiguous()

    def fused():
        return PM.token_embed_points(te, patches)

    def layerwise():
        return patch_embed_layerwise(patches, te.first_conv, te.second_conv)
    out['embed0_fused_vs_layerwise_rel'] = rel(fused(), layerwise())
    out['embed0_fused_ms'], out['embed0_layerwise_ms'] = alternate([fused, layerwise], 5, rounds)
    H = model.h_encoder.num_heads
    for T, D, radius in ((512, 16, 0.32), (255, 32, 0.64), (64, 64, 1.28)):
        qkv = torch.randn(B * T, 3 * H * D, device='cuda')
        cen = torch.rand(B * T, 3, device='cuda') - 0.5
        lens = torch.full((B,), T, dtype=torch.int32, device='cuda')
        out['attn_T%d_D%d_ms' % (T, D)] = alternate(
            [lambda: PM.attention_local(qkv, cen, lens, B, T, H, D ** -0.5, radius)], 50, rounds)[0]
    sd = dict(model.state_dict())

    def new():
        return model(pts)

    def restatement():
        nb, c, ix = model.group(pts)
        return R.forward(nb, c, ix, sd)['feature']
    out['feature_vs_restatement_fp32_rel'] = rel(new(), restatement())
    out['feature_ms'], out['feature_restatement_ms'] = alternate([new, restatement], 3, rounds)
    out['grouping_ms'] = alternate([lambda: model.group(pts)], 5, rounds)[0]
    out['clouds_per_s'] = round(B / (out['feature_ms'][0] * 1e-3), 1)
    out['clouds_per_s_restatement'] = round(B / (out['feature_restatement_ms'][0] * 1e-3), 1)
    out['modelnet40_two_passes_s'] = round((9843 + 2468) / out['clouds_per_s'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
