"""Golden record of the reference's runner-side train transform (datasets/data_transforms.py PointcloudRotate), from the
LIVE reference on the CPU.

Runs only where the reference tree exists (ref_import.REF).  The reference's module imports only numpy and torch and its
PointcloudRotate runs on a CPU tensor, so it is loaded from its file as it lies, read-only, bytecode writing disabled.
np.random is seeded, the class is applied to a (4, 64, 3) cloud, and the seed, the input, the output and the NEXT
np.random.uniform() behind the call are stored: the output pins the maps the product draws
(point_dae_amd/data_transforms.py PointcloudRotate.draw), the next draw pins how many values it consumes and in which
order.  Data only.

    python tests/golden/make_rotate_fixture.py        ->  tests/golden/rotate_transform_b4.npz
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import as R  # noqa: E402

SEED, B, N = 20, 4, 64


def main():
    if not R.available():
        raise SystemExit('reference tree not found at %s' % R.REF)
    spec = importlib.util.spec_from_file_location('ref_data_transforms', os.path.join(R.REF, 'datasets', 'data_transforms.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    # a cloud of its own generator (np.random stays untouched until the seed below): unit-scale coordinates, one cloud
    # scaled to O(100), one exact zero and one negative zero among them
    x = np.random.default_rng(7).uniform(-1.0, 1.0, (B, N, 3)).astype(np.float32)
    x[1] *= 100.0
    x[2, 0, 0], x[2, 1, 2] = 0.0, -0.0
    np.random.seed(SEED)
    out = ref.PointcloudRotate()(torch.from_numpy(x.copy()))
    nxt = np.random.uniform()
    path = os.path.join(HERE, 'rotate_transform_b4.npz')
    np.savez(path, seed=np.int64(SEED), input=x, output=out.numpy().astype(np.float32), next_uniform=np.float64(nxt))
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
