"""One round of the voted evaluation (runner_finetune.vote_pass, times = 10) per backend on both classifiers at the
configs' sizes: a synthetic test set of COUNT clouds (default 2468, ModelNet40's test split) of the config's N_POINTS points
in batches of total_bs, scratch models in eval().  The variants -- PDAE_VOTE=torch, PDAE_VOTE=hip with FPS every round,
PDAE_VOTE=hip with the FPS cache -- are warmed up once and then alternated REPS times; the time is a host clock around
a pass that ends in a device synchronise.  One line per pass and a RESULT line per variant.

    python tools/bench_vote.py [COUNT] [REPS] [mark]

mark: every variant once more between two marker kernels (pdae_calib_copy), for counting the launches of a pass in a
kernel trace (rocprofv3 --kernel-trace, in a run of its own).
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from point_dae_amd import _lib, builder, datasets, runner_finetune  # noqa: E402,F401
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.registry import DATASETS  # noqa: E402

CFGS = {'DGCNN': 'cfgs/finetune_modelnet_dgcnn_smooth.yaml',
        'PointTransformer': 'cfgs/finetune_modelnet_transferring_features.yaml'}


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 2468
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    mark = len(sys.argv) > 3 and sys.argv[3] == 'mark'
    if not torch.cuda.is_available():
        raise RuntimeError('bench_vote needs an MI355X: there is no CPU path')
    mark_src = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    mark_dst = torch.zeros_like(mark_src)

    def marker():
        _lib.call('pdae_calib_copy', mark_src, 1024, _lib.ptr(mark_src), _lib.ptr(mark_dst))

    for name, path in CFGS.items():
        config = cfg_from_yaml_file(os.path.join(ROOT, path))
        c = dict(config.dataset.test._base_)
        c.update(dict(config.dataset.test.others))
        c.update(npoints=int(c['N_POINTS']), device='cuda', seed=0, rank=0, world=1, count=count, bs=config.total_bs)
        loader = DATASETS.build(c)
        torch.manual_seed(0)
        model = builder.model_builder(config.model)
        model.load_model_from_ckpt(None, log=lambda *a: None)
        model = model.cuda().eval()
        print(name, 'clouds', loader.count, 'points', loader.npoints, 'bs', loader.bs, 'batches', len(loader), flush=True)
        cache = []

        def one(backend, fps_cache):
            os.environ['PDAE_VOTE'] = backend
            np.random.seed(1)
            counter = torch.zeros(1, dtype=torch.int32, device='cuda')
            torch.cuda.synchronize()
            if mark:
                marker()
            t = time.perf_counter()
            with torch.no_grad():
                runner_finetune.vote_pass(model, loader, config, 10, fps_cache, counter)
            if mark:
                marker()
            torch.cuda.synchronize()
            return time.perf_counter() - t, counter.item()

        variants = [('torch', lambda: one('torch', None)), ('hip, FPS every round', lambda: one('hip', None)),
                    ('hip, FPS cached', lambda: one('hip', cache))]
        one('hip', cache)                                    # fills the cache
        for label, fn in variants:
            dt, hits = fn()
            print(name, 'warm-up', label, '%.3f s' % dt, 'hits', hits, flush=True)
        times = {label: [] for label, _ in variants}
        for r in range(1 if mark else reps):
            for label, fn in variants:
                dt, hits = fn()
                times[label].append(dt)
                print(name, 'marked' if mark else 'rep %d' % r, label, '%.3f s' % dt, 'hits', hits, flush=True)
        for label, v in times.items():
            v = sorted(v)
            print(name, 'RESULT', label, 'median %.3f s' % v[len(v) // 2], 'min %.3f max %.3f' % (v[0], v[-1]),
                  '%.0f cloud-votes/s' % (loader.count * 10 / v[len(v) // 2]), flush=True)


if __name__ == '__main__':
    main()
