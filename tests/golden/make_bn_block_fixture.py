"""Record the head block's training-mode results, bn_block_train.npz: Dropout(ReLU / LeakyReLU(BatchNorm1d(y))) in
training mode, forward and backward, for seeded inputs (B=8, N=260: two blocks of columns, the second partly filled).

Run on the GPU at the commit whose bits are to be kept -- the file in the tree was written by the commit before the
block learnt the frozen-BatchNorm mode (its kernels were not yet templated on the BatchNorm mode); the test
test_gpu_protocols.py::test_training_mode_block_keeps_the_recorded_bits holds every later build to it.  Uses only
arguments the block had then.

    python tests/golden/make_bn_block_fixture.py [OUT.npz]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B, N, P, SLOPE = 8, 260, 0.5, 0.2


def inputs():
    g = torch.Generator().manual_seed(11)
    return dict(y=torch.randn(B, N, generator=g) * 2 + 0.3, u=torch.rand(B, N, generator=g),
                d=torch.randn(B, N, generator=g), gamma=1 + 0.2 * torch.randn(N, generator=g),
                beta=0.1 * torch.randn(N, generator=g))


def run(slope, **kw):
    """{out, dy, dgamma, dbeta, running_mean, running_var} of the block on the GPU; kw: further arguments of the block"""
    from point_dae_amd import finetune_ops as F
    t = inputs()
    bn = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        bn.weight.copy_(t['gamma']), bn.bias.copy_(t['beta'])
    bn = bn.cuda().train()
    y = t['y'].cuda().requires_grad_()
    if slope is None:
        out = F.bn_relu_dropout(y, bn, P, u=t['u'].cuda(), **kw)
    else:
        out = F.bn_lrelu_dropout(y, bn, P, slope, u=t['u'].cuda(), **kw)
    out.backward(t['d'].cuda())
    assert int(bn.num_batches_tracked) == 1
    return dict(out=out.detach(), dy=y.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
                running_var=bn.running_var)


if __name__ == '__main__':
    rec = {}
    for key, slope in (('relu', None), ('lrelu', SLOPE)):
        rec.update({'%s/%s' % (key, k): v.cpu().numpy() for k, v in run(slope).items()})
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'bn_block_train.npz')
    np.savez_compressed(path, **rec)
    print('wrote', path, sorted(rec))
