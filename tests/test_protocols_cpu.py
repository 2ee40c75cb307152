"""The frozen-encoder protocols (optimizer.part only_new / diff_lr) without a GPU: the linear-protocol model's layout,
the AdamW groups, set_bn_eval's reach and the three new configs, against tests/golden/protocol_layout.json (taken from
the live reference by tests/golden/make_protocol_fixtures.py)."""
import json
import os

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS_CFG = {'PointTransformer': 'finetune_modelnet_non_linear_classification.yaml',
              'PointTransformerLinearClassification': 'finetune_modelnet_linear_classification.yaml',
              'DGCNN': 'finetune_modelnet_dgcnn_smooth.yaml'}


def _layout():
    with open(os.path.join(ROOT, 'tests', 'golden', 'protocol_layout.json')) as f:
        return json.load(f)


def _build(name):
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', MODELS_CFG[name]))
    cfg.model.NAME = name
    return builder.model_builder(cfg.model), cfg


def test_registry_builds_the_linear_classifier_with_the_reference_layout(tmp_path):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_transformer import PointCAE_transformer
    from point_dae_amd.point_transformer import PointTransformer, PointTransformerLinearClassification
    fx = _layout()
    model, _ = _build('PointTransformerLinearClassification')
    assert type(model) is PointTransformerLinearClassification
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == fx['state_dict']
    assert len(model.cls_head_finetune) == 1 and isinstance(model.cls_head_finetune[0], torch.nn.Linear)
    # the trunk is shared with PointTransformer, not copied
    assert PointTransformerLinearClassification.trunk is PointTransformer.trunk
    pre = PointCAE_transformer(cfg_from_yaml_file(os.path.join(ROOT, fx['pretrain_config'])).model)
    path = str(tmp_path / 'ckpt-last.pth')
    torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, path)
    inc = model.load_model_from_ckpt(path, log=lambda *_: None)
    assert sorted(inc.missing_keys) == fx['missing_keys']
    assert sorted(inc.unexpected_keys) == fx['unexpected_keys']


@pytest.mark.parametrize('part', ['only_new', 'diff_lr'])
@pytest.mark.parametrize('name', sorted(MODELS_CFG))
def test_parameter_groups_equal_the_reference(name, part):
    from point_dae_amd import builder
    model, cfg = _build(name)
    want = _layout()['groups'][name][part]
    kw = cfg.optimizer.kwargs
    groups = builder.add_weight_decay(model, kw.weight_decay, part=part, lr=kw.lr)
    name_of = {id(p): n for n, p in model.named_parameters()}
    assert len(groups) == len(want) == (4 if part == 'diff_lr' else 2)
    for g, w in zip(groups, want):
        assert [name_of[id(p)] for p in g['params']] == w['names']
        assert g['weight_decay'] == w['weight_decay']
        assert g.get('lr', kw.lr) == pytest.approx(w['lr'], rel=1e-12)
    if part == 'only_new' and name != 'DGCNN':
        assert 'cls_token' in want[0]['names'] and 'cls_pos' in want[1]['names']       # cls_pos IS decayed


@pytest.mark.parametrize('name', sorted(MODELS_CFG))
def test_set_bn_eval_freezes_the_reference_modules(name):
    from point_dae_amd.runner_finetune import set_bn_eval, set_train_mode
    fx = _layout()
    model, _ = _build(name)
    set_train_mode(model, 'only_new')
    bns = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
    assert sorted(n for n, m in bns.items() if not m.training) == sorted(fx['bn_eval'][name])
    assert sorted(n for n, m in bns.items() if m.training) == sorted(fx['bn_train'][name])
    # everything that is not a frozen BatchNorm stays in training mode (Dropout, DropPath, the model itself)
    assert all(m.training for n, m in model.named_modules() if n not in fx['bn_eval'][name])
    set_train_mode(model, 'all')
    assert all(m.training for m in model.modules())
    model.eval().apply(set_bn_eval)
    assert not any(m.training for m in model.modules())


@pytest.mark.parametrize('name', ['finetune_modelnet_linear_classification.yaml',
                                  'finetune_modelnet_non_linear_classification.yaml',
                                  'finetune_modelnet_transferring_features_diff_lr.yaml'])
def test_new_config_equals_the_reference_values(name):
    from point_dae_amd.config import cfg_from_yaml_file
    want = _layout()['configs'][name]['values']
    with open(os.path.join(ROOT, 'cfgs', name)) as f:
        assert yaml.safe_load(f) == want
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', name))
    assert cfg.optimizer.part == want['optimizer']['part'] and cfg.model.NAME == want['model']['NAME']
    assert cfg.optimizer.kwargs.lr == want['optimizer']['kwargs']['lr']


def test_segment_runs_merge_adjacent_spans():
    from point_dae_amd.optim import _runs
    assert _runs([(0, 4), (4, 6), (12, 0), (16, 8), (24, 1)]) == [(0, 10), (16, 9)]


def test_runner_refuses_dgcnn_only_new_before_touching_the_gpu():
    model, _ = _build('DGCNN')
    assert 'bn4' in model.only_new_unsupported and 'training-mode' in model.only_new_unsupported
    assert _build('PointTransformer')[0].only_new_unsupported is None
