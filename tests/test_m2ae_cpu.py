"""Point-M2AE as the linear-SVM feature extractor (point_dae_amd/point_m2ae.py), the checks that need no GPU.

tests/golden/m2ae_svmfeat_{a,b,c}.npz hold the LIVE reference's outputs (make_m2ae_encoder_fixtures.py): the fp32 feature
of models/Point_M2AE.py Point_M2AE_SVMFeature on seeded clouds with weights.fill_state(model, 7), and the feature of the
same modules run in fp64.  (i) validates the yardstick of tests/test_gpu_m2ae.py -- tests/m2ae_restatement.py -- against
them; (ii) to (v) are the host side of the model: layout, checkpoint loading, the refusals, the config."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import m2ae_restatement as R  # noqa: E402
import weights  # noqa: E402

CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_svm_pointm2ae.yaml')
#           num_groups, group_sizes, T_pad per level, visible per level
FIXTURES = {'a': ([72, 40, 8], [16, 8, 4], [72, 29, 8], [[72, 67, 72], [29, 27, 29], [8, 8, 8]]),
            'b': ([136, 72, 16], [16, 8, 4], [133, 56, 16], [[131, 133], [56, 51], [16, 16]]),
            'c': ([512, 256, 64], [16, 8, 8], [512, 255, 64], [[512, 512], [252, 255], [64, 64]])}


def build_model(num_groups=None, group_sizes=None, name=None):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    cfg = cfg_from_yaml_file(CFG).model
    if num_groups is not None:
        cfg.num_groups, cfg.group_sizes = list(num_groups), list(group_sizes)
    if name is not None:
        cfg.NAME = name
    return MODELS.build(cfg)


def fixture(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'm2ae_svmfeat_%s.npz' % name))


@pytest.mark.parametrize('name', list(FIXTURES))
def test_restatement_in_fp64_reproduces_the_live_reference(oracle_ops, name):
    """(i) the framework-op restatement, fed the oracle's grouping of the fixture's clouds, against the reference's fp64
    features: 1e-9 of the largest entry (both are fp64 evaluations of one formula in different op orders)."""
    num_groups, group_sizes, t_pads, visible = FIXTURES[name]
    f = fixture(name)
    nb, c, idx = oracle_ops.m2ae_hierarchy(f['pts'], num_groups, group_sizes)
    model = weights.fill_state(build_model(num_groups, group_sizes), 7)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    out = R.forward([torch.from_numpy(t).double() for t in nb], [torch.from_numpy(t).double() for t in c],
                    [torch.from_numpy(t) for t in idx], sd)
    for i, lv in enumerate(out['levels']):
        assert lv['T_pad'] == t_pads[i] == int(f['T_pad%d' % i])
        assert lv['lens'].tolist() == visible[i] == f['len%d' % i].tolist()
        want = f['rows%d_sample' % i]
        got = lv['rows'][::7].numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), i
    want = f['feature64']
    err = np.abs(out['feature'].numpy() - want).max() / np.abs(want).max()
    print('%s: restatement fp64 vs reference fp64 %.2e; reference fp32 vs fp64 %.2e' % (name, err, float(f['dist'])))
    assert err <= 1e-9
    assert 1e-8 < float(f['dist']) < 2e-6           # the stored fp32 feature is an fp32 evaluation of the same thing


def test_state_dict_layout_equals_the_reference():
    """(ii)"""
    with open(os.path.join(ROOT, 'tests', 'golden', 'm2ae_svmfeat_layout.json')) as fh:
        layout = json.load(fh)
    model = build_model()
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == layout['state_dict']
    assert len(sd) == 237
    assert sum(p.numel() for p in model.parameters()) == layout['parameters'] == 12654976


def test_pretraining_checkpoint_loads_with_its_prefixes(tmp_path):
    """(iii) a checkpoint saved under 'base_model' with 'module.' prefixes, the encoder partly under 'MAE_encoder.', and
    decoder keys the feature extractor has no use for."""
    src = weights.fill_state(build_model([72, 40, 8], [16, 8, 4]), 3)
    sd = {}
    for k, v in src.state_dict().items():
        sd['module.' + ('MAE_encoder.' + k if 'encoder_blocks.1' in k else k)] = v.clone()
    extras = {'module.h_decoder.0.blocks.0.norm1.weight': torch.ones(384), 'module.mask_token': torch.zeros(1, 384)}
    sd.update(extras)
    path = str(tmp_path / 'ckpt.pth')
    torch.save({'base_model': sd, 'epoch': 3}, path)
    model = build_model([72, 40, 8], [16, 8, 4])
    lines = []
    inc = model.load_model_from_ckpt(path, log=lines.append)
    assert list(inc.missing_keys) == []
    assert sorted(inc.unexpected_keys) == sorted(k[len('module.'):] for k in extras)
    for k, v in model.state_dict().items():
        assert torch.equal(v, src.state_dict()[k]), k
    text = '\n'.join(lines)
    assert 'unexpected_keys' in text and 'h_decoder.0.blocks.0.norm1.weight' in text and 'missing_keys' not in text
    lines = []
    assert build_model().load_model_from_ckpt(None, log=lines.append) is None and 'scratch' in lines[0]


def test_forward_refuses_the_cpu_and_training_mode():
    """(iv)"""
    model = build_model([72, 40, 8], [16, 8, 4])
    pts = torch.rand(2, 300, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        model.eval()(pts)
    with pytest.raises(NotImplementedError, match='evaluation mode only'):
        model.train()(pts)


def test_config_parses_and_model_name_overrides_it(tmp_path, monkeypatch):
    """(v) the yaml names the model directly; --model_name still replaces it (main.py:64-65)."""
    from point_dae_amd import parser
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401
    cfg = cfg_from_yaml_file(CFG)
    m = cfg.model
    assert m.NAME == 'Point_M2AE_SVMFeature' and 'Point_M2AE_SVMFeature' in MODELS
    assert (m.num_groups, m.group_sizes, m.encoder_dims, m.encoder_depths) == ([512, 256, 64], [16, 8, 8], [96, 192, 384], [5, 5, 5])
    assert m.local_radius == [0.32, 0.64, 1.28] and m.num_heads == 6
    assert cfg.npoints == 2048 and cfg.total_bs == 128 and cfg.dataset.train.others.npoints == 2048
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    args = parser.get_args(['--config', CFG, '--finetune_model', '--svm_classification', '--model_name',
                            'Point_M2AE_SVMFeature'])
    assert args.svm_classification and args.model_name == 'Point_M2AE_SVMFeature'
    m.NAME = 'Point_M2AE'                            # what the reference's file says; it relies on --model_name
    with pytest.raises(KeyError):
        MODELS.build(m)
    if args.model_name != 'none':
        m.NAME = args.model_name
    assert type(MODELS.build(m)).__name__ == 'Point_M2AE_SVMFeature'
