"""Few-shot fine-tuning at the paper's largest episode: 10-way 20-shot, 200 training and 200 test clouds of 8192 points
(synthetic), total_bs 32, the config's PointTransformer from scratch.  Four numbers:

    the time of a training epoch (6 steps: batch preparation + the graphed step) under PDAE_FEWSHOT=torch and =hip,
    the time of one validation without and with the kept FPS-to-npoints point sets,

and, beside them, the batch preparation alone (6 batches, no step).  The variants are warmed up (the step's graph is
captured) and then alternated REPS times; a training figure is EPOCHS epochs inside one host-clock window that ends in a
device synchronise, divided by EPOCHS.  One line per window and a RESULT line per variant.

    python tools/bench_fewshot.py [REPS] [EPOCHS] [WAY] [SHOT]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from point_dae_amd import builder, datasets, runner_finetune  # noqa: E402,F401
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.data_parallel import FlatDataParallel  # noqa: E402
from point_dae_amd.finetune_ops import GradNormClip  # noqa: E402
from point_dae_amd.graph_step import GraphedClassifierStep, use_created_stream  # noqa: E402
from point_dae_amd.registry import DATASETS  # noqa: E402

CFG = 'cfgs/fewshot_modelnet_transferring_features.yaml'


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    way = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    shot = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    if not torch.cuda.is_available():
        raise RuntimeError('bench_fewshot needs an MI355X: there is no CPU path')
    use_created_stream()
    config = cfg_from_yaml_file(os.path.join(ROOT, CFG))
    bs = config.total_bs

    def loader(node):
        c = dict(node._base_)
        c.update(dict(node.others))
        c.update(device='cuda', seed=0, bs=bs, way=way, shot=shot, fold=0)
        return DATASETS.build(c)
    train_loader, test_loader = loader(config.dataset.train), loader(config.dataset.test)
    torch.manual_seed(0)
    base_model = builder.model_builder(config.model)
    base_model.load_model_from_ckpt(None, log=lambda *a: None)
    base_model = base_model.cuda()
    model = FlatDataParallel(base_model)
    optimizer, _ = builder.build_opti_sche(model, config)
    model.zero_grad()
    clip = GradNormClip(model.flat_grad, config.grad_norm_clip)
    graphed = GraphedClassifierStep(model, optimizer, clip, bs, config.npoints)
    print('episode %d-way %d-shot: train %s test %s, bs %d, %d steps per epoch' % (
        way, shot, tuple(train_loader.set.shape), tuple(test_loader.set.shape), bs, len(train_loader)), flush=True)

    def train(backend, n_epochs, step=True):
        os.environ['PDAE_FEWSHOT'] = backend
        np.random.seed(1)
        model.train()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n_epochs):
            for _, _, data in train_loader:
                points = runner_finetune.fewshot_train_points(train_loader, data, config.npoints, out=graphed.points)
                if not step:
                    continue
                if points is graphed.points:
                    graphed.step_filled(data[2])
                else:
                    graphed(points, data[2])
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n_epochs

    kept = []

    def val(point_sets):
        os.environ['PDAE_FEWSHOT'] = 'hip'
        logs = []
        torch.cuda.synchronize()
        t = time.perf_counter()
        runner_finetune.validate(base_model, test_loader, 0, config, None, log=logs.append, point_sets=point_sets)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    variants = [('train epoch, torch', lambda: train('torch', epochs)), ('train epoch, hip', lambda: train('hip', epochs)),
                ('batch preparation of an epoch, torch', lambda: train('torch', epochs, False)),
                ('batch preparation of an epoch, hip', lambda: train('hip', epochs, False)),
                ('validation, FPS every time', lambda: val(None)), ('validation, point sets kept', lambda: val(kept))]
    train('hip', 1), train('torch', 1)                       # the eager warm-up steps and the capture
    val(kept)                                                # fills the kept point sets
    for label, fn in variants:
        print('warm-up', label, '%.2f ms' % (fn() * 1e3), flush=True)
    times = {label: [] for label, _ in variants}
    for r in range(reps):
        for label, fn in variants:
            dt = fn()
            times[label].append(dt)
            print('rep %d' % r, label, '%.2f ms' % (dt * 1e3), flush=True)
    for label, v in times.items():
        v = sorted(v)
        print('RESULT', label, 'median %.2f ms' % (v[len(v) // 2] * 1e3), 'min %.2f max %.2f' % (v[0] * 1e3, v[-1] * 1e3),
              flush=True)


if __name__ == '__main__':
    main()
