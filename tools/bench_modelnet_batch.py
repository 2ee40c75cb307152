"""One training-batch preparation of ModelNet40 fine-tuning at the workload's shape: B = 32 clouds of P = 8192 points from
a resident set, aug_type [norm, scale, translate], FPS to 1200 points, npoints 1024.  The set is a synthetic
.dat file in the reference's format that the tool writes itself (into a temporary directory) and datasets.ModelNet reads.
Two variants, fed the same draws:

    chain   the entries a batch takes without pdae_resident_batch: item select, permutation gather,
            pdae_pipeline_norm_affine, FPS, index_select, the two transposing copies around gather_points
            (the loader's __iter__ + runner_finetune.resample)
    hip     resident_ops.fill_batch: one launch into the step's input buffer

The host draws (the epoch's items, the maps, the subset) and the device draw of the shuffle are made outside the timed
window for both; a window is BATCHES preparations between two device synchronisations on the host clock, divided by
BATCHES.  Warm-up first, then the variants alternate REPS times; one line per window and a RESULT line per variant
(median, min, max).

    python tools/bench_modelnet_batch.py [REPS] [BATCHES] [CLOUDS]
"""
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from point_dae_amd import datasets, resident_ops, runner_finetune  # noqa: E402,F401
from point_dae_amd.registry import DATASETS  # noqa: E402
from point_dae_amd.synthetic import labelled_clouds  # noqa: E402

B, P, POINT_ALL, NPOINTS = 32, 8192, 1200, 1024


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    batches = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    clouds = int(sys.argv[3]) if len(sys.argv) > 3 else 8 * B
    if not torch.cuda.is_available():
        raise RuntimeError('bench_modelnet_batch needs an MI355X: there is no CPU path')
    with tempfile.TemporaryDirectory() as root:
        x, y = labelled_clouds(clouds, P, seed=0, classes=3)
        x = np.concatenate([x * 1.7 + 0.3, np.zeros_like(x)], 2).astype(np.float32)        # six channels, un-normalised
        with open(os.path.join(root, 'modelnet40_train_%dpts_fps.dat' % P), 'wb') as f:
            pickle.dump([list(x), [np.array([k], np.int32) for k in y]], f)
        loader = DATASETS.build(dict(NAME='ModelNet', DATA_PATH=root, N_POINTS=P, NUM_CATEGORY=40, USE_NORMALS=False,
                                     subset='train', npoints=P, bs=B, seed=0, device='cuda',
                                     aug_type=['norm', 'scale', 'translate']))
    assert loader.listed and loader.resident
    set_ = loader.set
    draws = [d for _, _, d in loader.iter_draws()][:batches]
    choices = [runner_finetune.subset_indices(NPOINTS, POINT_ALL) for _ in draws]
    print('set %s, %d batches of %d per window' % (tuple(set_.shape), len(draws), B), flush=True)
    out = torch.empty((B, NPOINTS, 3), device='cuda')

    def chain():
        for (item, perm, nmaps, maps, _), choice in zip(draws, choices):
            pts = set_.index_select(0, item.long())
            pts = torch.gather(pts, 1, perm.long().unsqueeze(-1).expand(-1, -1, 3))
            pts = datasets.pipeline_norm_affine(pts, False, (nmaps, maps))
            got = runner_finetune.resample(pts, NPOINTS, choice=choice)
        return got

    def hip():
        for (item, perm, nmaps, maps, _), choice in zip(draws, choices):
            resident_ops.fill_batch(set_, item, perm, nmaps, maps, choice, POINT_ALL, out)
        return out

    def window(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / len(draws)

    # the two variants make the same batch (the last of the window), bit for bit
    assert torch.equal(chain().view(torch.int32), hip().clone().view(torch.int32))
    variants = [('chain', chain), ('hip, one launch', hip)]
    for label, fn in variants:
        for _ in range(2):
            print('warm-up', label, '%.3f ms' % (window(fn) * 1e3), flush=True)
    times = {label: [] for label, _ in variants}
    for r in range(reps):
        for label, fn in variants:
            dt = window(fn)
            times[label].append(dt)
            print('rep %d' % r, label, '%.3f ms' % (dt * 1e3), flush=True)
    for label, v in times.items():
        v = sorted(v)
        print('RESULT', label, 'median %.3f ms' % (v[len(v) // 2] * 1e3), 'min %.3f max %.3f' % (v[0] * 1e3, v[-1] * 1e3),
              flush=True)


if __name__ == '__main__':
    main()
