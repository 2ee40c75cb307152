"""Every distinct product the row-GEMM family computes in one optimisation step of cfg3 (PointCAE_transformer, B = 128,
all visible-token counts the mask ratio can draw), the published variant, cfg2 (Point_CAE_PointNetv2, B = 128), the cfg5
per-GPU shape (N = 2048, G = 128, B = 32: 20 drawn visible-token counts and both ends, 26 and 64), DGCNN
(Point_CAE_DGCNN_FCOnly on the cfg2 YAML, B = 32) and the two ModelNet40 fine-tuning classifiers, ft_transformer
(PointTransformer, T = 65 tokens: trunk products of M = 65 B rows) and ft_dgcnn (DGCNN with the smoothed loss), each at
total_bs = 32: one eager training step (forward, loss, backward) and eval-mode forwards at B = 32 and at B = 4, the
short last batch of ModelNet40's 2468 test clouds.  Recorded at the C boundary (point_dae_amd/_lib.CALL_HOOK) while the
steps run eagerly -> tests/golden/gemm_shapes.json, the shape list of tests/test_gpu_rows3.py.  Run on a GPU:
python tools/dump_gemm_shapes.py"""
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from point_dae_amd import _lib  # noqa: E402

FT_TRANSFORMER = 'cfgs/finetune_modelnet_transferring_features.yaml'
FT_DGCNN = 'cfgs/finetune_modelnet_dgcnn_smooth.yaml'
FT_TEST_COUNT = 2468                 # ModelNet40's test clouds: at total_bs = 32 the last batch holds 4

gemm, wgrad = set(), set()


def hook(name, a):
    if name == 'pdae_rows_gemm':
        gemm.add((a[0], a[1], a[2], int(a[5]), int(a[7])))          # M, N, K, w_kn, epi
    elif name == 'pdae_rows_gemm_bnrelu_stats':                       # a data gradient into relu(bn(X)), [K, N] weight,
        gemm.add((a[0], a[1], a[2], 1, 5, int(a[6] is not None)))    # BatchNorm-backward's sums: epi 5, X listed or not
    elif name == 'pdae_rows_wgrad_listed':
        wgrad.add((a[0], a[1], a[2], int(a[4] is not None), int(a[6] is not None), int(a[7] is not None)))
    elif name == 'pdae_rows_wgrad_multi':
        for m, n, k in zip(list(a[1]), list(a[6]), list(a[7])):
            wgrad.add((m, n, k, 0, 0, 0))
    elif name == 'pdae_rows_wgrad':
        for n, k in zip(list(a[6]), list(a[7])):
            wgrad.add((a[0], n, k, 0, 0, 0))


def main():
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.graph_step import (GraphedClassifierStep, GraphedStaticStep, GraphedTrainStep,
                                          use_created_stream)
    from point_dae_amd.synthetic import shapenet_like_clouds
    device = torch.device('cuda', 0)
    use_created_stream(device)
    out = {}
    for wl in ('cfg3', 'published', 'cfg2', 'cfg5', 'dgcnn'):
        gemm.clear(), wgrad.clear()
        B, N = (32, 2048) if wl == 'cfg5' else ((32, 1024) if wl == 'dgcnn' else (128, 1024))
        x = torch.from_numpy(shapenet_like_clouds(2 * B, N, seed=7)).to(device)
        config = cfg_from_yaml_file(os.path.join(ROOT, {'cfg2': bench.CFG2, 'dgcnn': bench.CFG2,
                                                        'cfg5': bench.CFG5}.get(wl, bench.CFG3)))
        if wl == 'published':
            config.model.NAME = 'PointCAE_transformer_fc_global_folding_local'
        elif wl == 'dgcnn':
            config.model.NAME = 'Point_CAE_DGCNN_FCOnly'
        elif wl == 'cfg5':
            config.npoints, config.model.num_group = N, 128
            random.seed(5), np.random.seed(5), torch.manual_seed(5)       # (39 counts can be drawn: a fixed 20)
        model = FlatDataParallel(builder.model_builder(config.model).to(device), broadcast=False, process_group=None)
        model.world_size = 1
        optimizer, _ = builder.build_opti_sche(model, config)
        model.train()
        model.zero_grad()
        _lib.CALL_HOOK = hook
        if wl in ('cfg2', 'dgcnn'):
            step = GraphedStaticStep(model, optimizer, lambda a, b: a + 0.5 * b, B, N)
            step(x[:B], x[B:])                    # the first calls of a graphed step run eagerly
        else:
            step = GraphedTrainStep(model, optimizer, config, B, N, split=False)
            seen = set()
            for i in range(400):
                step.pts.copy_(x[:B])
                tvis = step._draw()
                if tvis in seen:
                    continue
                seen.add(tvis)
                step._fwd_bwd(tvis)
                model.zero_grad()
                if len(seen) == 20:
                    break
            if wl == 'cfg5':
                G = config.model.num_group
                for tvis in (G - int(0.8 * G), G - int(0.5 * G)):     # the two ends of the mask ratio's range
                    if tvis not in seen:
                        step.pts.copy_(x[:B])
                        seen.add(step._draw(tvis))
                        step._fwd_bwd(tvis)
                        model.zero_grad()
                print(wl, 'visible-token counts', sorted(seen), flush=True)
        _lib.CALL_HOOK = None
        torch.cuda.synchronize()
        out[wl] = {'gemm': sorted(gemm), 'wgrad': sorted(wgrad)}
        print(wl, len(gemm), 'gemm shapes,', len(wgrad), 'wgrad shapes', flush=True)
        del model, optimizer, step
        torch.cuda.empty_cache()
    for wl, cfg in (('ft_transformer', FT_TRANSFORMER), ('ft_dgcnn', FT_DGCNN)):
        gemm.clear(), wgrad.clear()
        config = cfg_from_yaml_file(os.path.join(ROOT, cfg))
        B, N = config.total_bs, config.npoints
        random.seed(5), np.random.seed(5), torch.manual_seed(5)
        x = torch.from_numpy(shapenet_like_clouds(B, N, seed=7)).to(device)
        labels = torch.from_numpy(np.random.default_rng(5).integers(0, config.model.cls_dim, B)).to(device)
        model = FlatDataParallel(builder.model_builder(config.model).to(device), broadcast=False, process_group=None)
        model.world_size = 1
        optimizer, _ = builder.build_opti_sche(model, config)
        model.train()
        model.zero_grad()
        _lib.CALL_HOOK = hook
        step = GraphedClassifierStep(model, optimizer, None, B, N)
        step(x, labels)                           # the first calls of a graphed step run eagerly
        model.module.eval()
        with torch.no_grad():
            for b in (B, FT_TEST_COUNT % B):      # validation: full batches and the test set's short last one
                model.module(x[:b])
        _lib.CALL_HOOK = None
        torch.cuda.synchronize()
        out[wl] = {'gemm': sorted(gemm), 'wgrad': sorted(wgrad)}
        print(wl, len(gemm), 'gemm shapes,', len(wgrad), 'wgrad shapes', flush=True)
        del model, optimizer, step
        torch.cuda.empty_cache()
    with open(os.path.join(ROOT, 'gpurun_out', 'gemm_shapes.json'), 'w') as f:
        json.dump(out, f)


if __name__ == '__main__':
    main()
