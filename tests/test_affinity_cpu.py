"""The task-affinity protocol (--task_affinity), CPU side: the flag and its dispatch, the new configuration, the probe's
learning-rate schedule against CosineAnnealingLR, the taxonomy-rank labels of a listed ShapeNetClass set, the shared
host-side draws, and the label checks that raise before the native library is touched."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, 'cfgs', 'finetune_shapenet_task_affinity_dgcnn.yaml')


def test_parser_accepts_task_affinity(tmp_path, monkeypatch):
    from point_dae_amd import parser
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    assert parser.get_args(['--config', CFG]).task_affinity is False
    assert parser.get_args(['--config', CFG, '--task_affinity']).task_affinity is True


@pytest.mark.parametrize('flags,taken', [(['--scratch_model', '--task_affinity'], 'task_affinity'),
                                         (['--finetune_model', '--task_affinity'], 'task_affinity'),
                                         (['--scratch_model', '--task_affinity', '--so3_rotation'], 'task_affinity'),
                                         (['--scratch_model', '--task_affinity', '--svm_classification'], 'svm_classification'),
                                         (['--scratch_model'], 'run_net')])
def test_main_dispatches_to_task_affinity(tmp_path, monkeypatch, flags, taken):
    """main.py:101-109 of the reference: --svm_classification is looked at first, then --task_affinity, then
    --so3_rotation."""
    from point_dae_amd import main, runner_finetune
    calls = []
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    for name in ('run_net', 'run_net_rotation', 'svm_classification', 'task_affinity'):
        monkeypatch.setattr(runner_finetune, name, lambda args, config, name=name: calls.append(name))
    main.main(['--config', CFG, *flags])
    assert calls == [taken]


def test_main_refuses_the_distributed_launcher(tmp_path, monkeypatch):
    from point_dae_amd import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    with pytest.raises(ValueError, match='one process'):
        main.main(['--config', CFG, '--scratch_model', '--task_affinity', '--launcher', 'pytorch'])


def test_new_config():
    from point_dae_amd.config import cfg_from_yaml_file
    import yaml
    cfg = cfg_from_yaml_file(CFG)
    assert cfg.model.NAME == 'DGCNN_feat' and cfg.total_bs == 64 and cfg.npoints == 1024
    for split, subset in (('train', 'train'), ('val', 'test'), ('test', 'test')):
        others = cfg.dataset[split].others
        assert others.subset == subset and others.npoints == 1024
        assert list(others.aug_type) == ['norm'] and list(others.corrupt_type) == ['clean']
        assert cfg.dataset[split]._base_.NAME == 'ShapeNetClass'
    with open(os.path.join(ROOT, 'cfgs', 'dataset_configs', 'ShapeNet-55_task_affinity.yaml')) as f:
        base = yaml.safe_load(f)
    assert base == {'NAME': 'ShapeNetClass', 'DATA_PATH': 'data/ShapeNet55-34/ShapeNet-55-subset-task-affinity',
                    'N_POINTS': 1024, 'PC_PATH': 'data/ShapeNet55-34/shapenet_pc_masksurf_with_normal'}


def test_schedule_is_cosine_annealing():
    """The closed form against CosineAnnealingLR(T_max=300) stepped once per epoch, over the 300 epochs: 1e-15 relative."""
    from point_dae_amd import affinity_ops
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=0.05)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=300)
    want = []
    for _ in range(300):
        want.append(opt.param_groups[0]['lr'])
        opt.step()
        sch.step()
    got = affinity_ops.cosine_lrs(1e-3, 300, 300)
    assert len(got) == 300 and got[0] == 1e-3
    worst = max(abs(g - w) / w for g, w in zip(got, want))
    print('cosine_lrs vs CosineAnnealingLR: %.3e relative' % worst)
    assert worst <= 1e-15
    import math
    direct = [1e-3 * (1.0 + math.cos(math.pi * e / 300)) / 2.0 for e in range(300)]
    print('the closed form evaluated directly: %.3e absolute, %.3e relative' % (
        max(abs(d - w) for d, w in zip(direct, want)), max(abs(d - w) / w for d, w in zip(direct, want))))
    assert max(abs(d - w) for d, w in zip(direct, want)) <= 1e-18
    assert 0 < got[-1] < 1e-7                            # the last epoch still trains, at lr (1 + cos(299 pi / 300)) / 2


def _listed(tmp_path, train, test):
    data = tmp_path / 'lists'
    data.mkdir()
    (data / 'train.txt').write_text(''.join(line + '\n' for line in train))
    (data / 'test.txt').write_text(''.join(line + '\n' for line in test))
    return data


def test_taxonomy_rank_labels(tmp_path):
    """Ids with gaps, out of order, and a class (03001627) that only test.txt holds: the label is the rank among the
    sorted distinct ids of both lists."""
    from point_dae_amd import datasets
    train = ['04379243-aa.npy', '02691156-b-c.npy', '04379243-dd.npy', '02958343-e.npy']
    test = ['03001627-f.npy', '02691156-g.npy']
    data = _listed(tmp_path, train, test)
    ranks = datasets.taxonomy_ranks(str(data))
    assert ranks == {'02691156': 0, '02958343': 1, '03001627': 2, '04379243': 3}
    assert [ranks[line.split('-')[0]] for line in train] == [3, 0, 3, 1]
    assert [ranks[line.split('-')[0]] for line in test] == [2, 0]
    assert issubclass(datasets.ShapeNetClass, datasets.ShapeNet)


@pytest.mark.parametrize('item', ['dropout_global', 'dropout_global_p5', 'dropout_patch_pointmae', 'Drop-Patch'])
def test_forward_side_corruptions_are_refused(item):
    from point_dae_amd import datasets
    with pytest.raises(NotImplementedError, match='forward'):
        datasets.ShapeNetClass(dict(corrupt_type=[item], device='cpu'))
    datasets.ShapeNetClass(dict(corrupt_type=['clean', 'affine_r3'], device='cpu'))


def test_out_of_range_labels_raise_before_the_library_is_touched(monkeypatch):
    from point_dae_amd import _lib, affinity_ops

    def no_library():
        raise AssertionError('the native library was touched')
    monkeypatch.setattr(_lib, 'lib', no_library)
    X = torch.zeros(70, 8)
    good = np.arange(70) % 5
    for bad in (np.where(np.arange(70) == 69, 5, good), np.where(np.arange(70) == 3, -1, good)):
        with pytest.raises(ValueError, match='train label outside'):
            affinity_ops.train_linear_probe(X, bad, 5)
        with pytest.raises(ValueError, match='test label outside'):
            affinity_ops.evaluate(torch.zeros(5, 8), torch.zeros(5), X, torch.from_numpy(bad))
        with pytest.raises(ValueError, match='train label outside'):
            affinity_ops.task_affinity_loss(X, bad, X, good)
    # num_class is max(test labels) + 1: a train label above every test label is out of range
    with pytest.raises(ValueError, match='train label outside 0 .. 3'):
        affinity_ops.task_affinity_loss(X, good, X, good % 4)
    with pytest.raises(ValueError, match='69 train labels for 70'):
        affinity_ops.train_linear_probe(X, good[:69], 5)
    # and with good labels there is no CPU path
    with pytest.raises(RuntimeError, match='GPU'):
        affinity_ops.train_linear_probe(X, good, 5)
    with pytest.raises(RuntimeError, match='GPU'):
        affinity_ops.evaluate(torch.zeros(5, 8), torch.zeros(5), X, good)


def test_shared_draws_follow_the_reference_order():
    """The init is nn.Linear(D, K) on the CPU under the current seed, then one randperm per epoch: what the reference's
    loop consumes from the default host generator, in its order."""
    from point_dae_amd import affinity_ops
    torch.manual_seed(7)
    lin = torch.nn.Linear(12, 5)
    want = [torch.randperm(100) for _ in range(3)]
    torch.manual_seed(7)
    W0, b0, perms = affinity_ops._draws(12, 5, 100, 3, None, None)
    assert torch.equal(W0, lin.weight.detach()) and torch.equal(b0, lin.bias.detach())
    assert perms.shape == (3, 100) and all(torch.equal(perms[e], want[e]) for e in range(3))
    # overrides: used as given, and a row that is no permutation is refused
    W1, b1, p1 = affinity_ops._draws(12, 5, 4, 2, (np.ones((5, 12)), np.zeros(5)), [[3, 2, 1, 0], [0, 1, 2, 3]])
    assert W1.dtype == torch.float32 and float(W1.sum()) == 60.0 and p1.tolist() == [[3, 2, 1, 0], [0, 1, 2, 3]]
    with pytest.raises(ValueError, match='permutation'):
        affinity_ops._draws(12, 5, 4, 1, None, [[0, 1, 1, 3]])


def test_backend_selection(monkeypatch):
    from point_dae_amd import affinity_ops
    monkeypatch.delenv('PDAE_AFFINITY', raising=False)
    assert affinity_ops.backend() == 'hip'
    monkeypatch.setenv('PDAE_AFFINITY', 'torch')
    assert affinity_ops.backend() == 'torch'
    monkeypatch.setenv('PDAE_AFFINITY', 'sklearn')
    with pytest.raises(ValueError, match='PDAE_AFFINITY'):
        affinity_ops.backend()


def test_new_abi_symbols_are_bound():
    from point_dae_amd import _lib
    names = set(_lib.exported_symbols())
    with open(os.path.join(ROOT, 'include', 'pdae.h')) as f:
        header = f.read()
    for n in ('pdae_linear_probe_train', 'pdae_linear_probe_eval', 'pdae_linear_probe_supported',
              'pdae_linear_probe_workspace'):
        assert n in names and n + '(' in header, n
    assert '#define PDAE_PROBE_MAX_CLASSES 64' in header
