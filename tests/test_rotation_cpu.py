"""The SO(3) rotation-robustness fine-tuning protocol without a GPU: the --so3_rotation flag, the three configurations, the
host draws of the runner-side transforms against the live-reference fixture (tests/golden/rotate_transform_b4.npz,
make_rotate_fixture.py) and against a re-enactment with np.random, and validate_rotation's ten passes on stubs."""
import os

import numpy as np
import pytest
import torch

from point_dae_amd import data_transforms, parser, runner_finetune
from point_dae_amd.config import get_config
from point_dae_amd.datasets import _AUGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rotate_transform_b4.npz')
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_rotation_%s_officialmodelnet.yaml')
U = 2.0 ** -24


def map_bound(x, A, t=None):
    """4 u (|x||A0j| + |y||A1j| + |z||A2j| + |tj|), fp64: the gamma_4 bound of the four-term fp32 sum
    ((x A0j + y A1j) + z A2j) + tj (at most four roundings touch any term), with or without fma contraction."""
    x, A = x.double().abs(), A.double().abs()
    mag = torch.einsum('bni,bij->bnj', x, A)
    if t is not None:
        mag = mag + t.double().abs()[:, None, :]
    return 4 * U * mag


def test_parser_knows_so3_rotation(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    base = ['--config', CFG % 'z2so3', '--scratch_model']
    assert parser.get_args(base).so3_rotation is False
    assert parser.get_args(base + ['--so3_rotation']).so3_rotation is True


@pytest.mark.parametrize('tag,train,test', [('z2z', 'rotate_z', 'rotate_z'), ('z2so3', 'rotate_z', 'rotate'),
                                            ('so32so3', 'rotate', 'rotate')])
def test_rotation_configs_load(tag, train, test):
    class Args:
        config, resume, local_rank, experiment_path = CFG % tag, False, 0, None
    config = get_config(Args)
    assert config.model.NAME == 'DGCNN' and config.model.smoothloss is True and config.model.cls_dim == 40
    assert config.npoints == 1024 and config.total_bs == 32
    want = {'train': train, 'val': test, 'test': test}
    for subset, item in want.items():
        node = config.dataset[subset]
        assert list(node.others.aug_type) == ['clean', item]
        assert all(a in _AUGS for a in node.others.aug_type)
        assert node._base_.NAME == 'ModelNet' and node._base_.NUM_CATEGORY == 40
        assert node.others.subset == ('train' if subset == 'train' else 'test')


def test_rotate_draw_reproduces_the_reference():
    fx = np.load(GOLDEN)
    x, want = torch.from_numpy(fx['input']), torch.from_numpy(fx['output'])
    np.random.seed(int(fx['seed']))
    A, t = data_transforms.PointcloudRotate().draw(x.shape[0])
    nxt = np.random.uniform()
    assert t is None and A.dtype == torch.float32 and tuple(A.shape) == (x.shape[0], 3, 3)
    got = torch.einsum('bni,bij->bnj', x.double(), A.double())
    # the reference's own fp32 matmul sums three terms: it stays within the same bound of the exact product
    err, bound = (got - want.double()).abs(), map_bound(x, A)
    print('rotate draw: max err / bound = %.3f' % (err / bound.clamp_min(1e-300)).max().item())
    assert (err <= bound).all()
    assert nxt == float(fx['next_uniform'])             # B uniforms consumed, nothing else


def test_scale_and_translate_draw_is_the_reference_order():
    B = 5
    tr = data_transforms.PointcloudScaleAndTranslate()
    assert (tr.scale_low, tr.scale_high, tr.translate_range) == (2. / 3., 3. / 2., 0.2)
    np.random.seed(31)
    A, t = tr.draw(B)
    nxt = np.random.uniform()
    np.random.seed(31)
    for i in range(B):                                  # data_transforms.py:28-32: scale first, then the shift, per cloud
        xyz1 = np.random.uniform(low=2. / 3., high=3. / 2., size=[3])
        xyz2 = np.random.uniform(low=-0.2, high=0.2, size=[3])
        assert torch.equal(A[i], torch.diag(torch.from_numpy(xyz1).float()))
        assert torch.equal(t[i], torch.from_numpy(xyz2).float())
    assert nxt == np.random.uniform()
    d = torch.diagonal(A, dim1=1, dim2=2)
    assert ((d >= 2. / 3.) & (d <= 3. / 2.)).all() and (t.abs() <= 0.2).all()
    custom = data_transforms.PointcloudScaleAndTranslate(scale_low=0.9, scale_high=1.1, translate_range=0.0)
    A, t = custom.draw(3)
    d = torch.diagonal(A, dim1=1, dim2=2)
    assert ((d >= 0.9) & (d <= 1.1)).all() and (t == 0).all()


class _StubLoader:
    """Three batches (the last one short) of labelled 'clouds'; the labels change with every pass, so the per-pass
    accuracies differ."""

    def __init__(self):
        self.iterations = 0
        g = torch.Generator().manual_seed(3)
        self.x = torch.rand(10, 8, 3, generator=g)

    def labels(self, k):
        return (torch.arange(10) * (k + 1)) % 3

    def __iter__(self):
        k = self.iterations
        self.iterations += 1
        y = self.labels(k)
        for i in range(0, 10, 4):
            yield 'ModelNet', i, (self.x[i:i + 4], y[i:i + 4])


class _StubModel(torch.nn.Module):
    """logits = a fixed function of the points."""

    def forward(self, pts):
        s = (pts.sum((1, 2)) * 7).long() % 3
        return torch.nn.functional.one_hot(s, 3).float()


def test_validate_rotation_averages_ten_passes(monkeypatch):
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    monkeypatch.setattr(runner_finetune, 'fps', lambda pts, n: (None, pts[:, :n]))
    loader, model = _StubLoader(), _StubModel().train()
    lines = []

    class Config:
        npoints = 8
    metric = runner_finetune.validate_rotation(model, loader, 4, Config, log=lines.append)
    assert loader.iterations == 10 and not model.training
    pred = model(loader.x).argmax(-1)
    accs = [(pred == loader.labels(k)).sum() / float(10) * 100. for k in range(10)]
    assert len({float(a) for a in accs}) > 1           # the passes differ, so a mean over one pass would show
    want = torch.Tensor(accs).mean()
    assert want.dtype == torch.float32
    assert metric.acc == float(want)
    assert lines == ['[Validation] EPOCH: 4  acc = %.4f' % want]
    metric = runner_finetune.validate_rotation(model, loader, 0, Config, log=lines.append, passes=3)
    accs = [(pred == loader.labels(k)).sum() / float(10) * 100. for k in (10, 11, 12)]
    assert loader.iterations == 13 and metric.acc == float(torch.Tensor(accs).mean())
