"""Fine-tuning classifier (PointTransformer), CPU side: the state_dict layout and the pretraining-checkpoint remap
against the live-reference fixture (tests/golden/finetune_layout.json), the CLI flags, the new ABI symbols, and
no CPU path."""
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features.yaml')


def _layout():
    with open(os.path.join(HERE, 'golden', 'finetune_layout.json')) as f:
        return json.load(f)


def _model_cfg():
    from point_dae_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(CFG).model


def test_model_state_dict_matches_reference_layout():
    from point_dae_amd.builder import model_builder
    model = model_builder(_model_cfg())
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == _layout()['state_dict']


def test_pretrain_checkpoint_remap_reports_reference_keys(tmp_path):
    from point_dae_amd.builder import model_builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_transformer import PointCAE_transformer
    lay = _layout()
    pre = PointCAE_transformer(cfg_from_yaml_file(os.path.join(ROOT, lay['pretrain_config'])).model)
    path = tmp_path / 'ckpt-last.pth'
    torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, str(path))
    model = model_builder(_model_cfg())
    lines = []
    inc = model.load_model_from_ckpt(str(path), log=lines.append)
    assert sorted(inc.missing_keys) == lay['missing_keys']
    assert sorted(inc.unexpected_keys) == lay['unexpected_keys']
    assert lines[0] == 'missing_keys' and 'unexpected_keys' in lines
    assert lines[-1].startswith('[Transformer] Successful Loading the ckpt from')
    # the encoder weights did arrive
    sd = pre.state_dict()
    assert torch.equal(model.blocks.blocks[3].mlp.fc1.weight, sd['MAE_encoder.blocks.blocks.3.mlp.fc1.weight'])
    assert torch.equal(model.encoder.second_conv[0].weight, sd['MAE_encoder.encoder.second_conv.0.weight'])


def test_from_scratch_init_follows_reference():
    from point_dae_amd.builder import model_builder
    model = model_builder(_model_cfg())
    lines = []
    assert model.load_model_from_ckpt(None, log=lines.append) is None
    assert lines == ['Training from scratch!!!']
    assert float(model.cls_head_finetune[0].bias.abs().max()) == 0.0
    assert float(model.blocks.blocks[0].mlp.fc1.weight.std()) < 0.03


def test_too_many_tokens_raises_at_construction():
    from point_dae_amd.point_transformer import PointTransformer
    cfg = _model_cfg()
    cfg.num_group = 128                       # the ScanObjectNN configurations: T = 129
    with pytest.raises(NotImplementedError, match='tokens'):
        PointTransformer(cfg)


def test_forward_raises_off_gpu():
    from point_dae_amd.point_transformer import PointTransformer
    cfg = _model_cfg()
    cfg.depth = 1
    with pytest.raises(RuntimeError, match='GPU'):
        PointTransformer(cfg)(torch.zeros(2, 1024, 3))


def test_parser_accepts_finetune_flags(tmp_path, monkeypatch):
    from point_dae_amd import parser
    monkeypatch.chdir(tmp_path)
    a = parser.get_args(['--config', CFG, '--finetune_model', '--ckpts', 'x.pth'])
    assert a.finetune_model and not a.scratch_model and a.ckpts == 'x.pth'
    b = parser.get_args(['--config', CFG, '--scratch_model'])
    assert b.scratch_model and not b.finetune_model
    c = parser.get_args(['--config', CFG])
    assert not c.finetune_model and not c.scratch_model


def test_new_abi_symbols_are_bound():
    from point_dae_amd import _lib
    names = set(_lib.exported_symbols())
    for n in ('pdae_prepend_token', 'pdae_prepend_token_grad', 'pdae_cls_max_concat', 'pdae_cls_max_concat_grad',
              'pdae_bn_relu_dropout', 'pdae_bn_relu_dropout_grad', 'pdae_softmax_xent', 'pdae_softmax_xent_grad',
              'pdae_grad_norm_clip', 'pdae_grad_norm_parts', 'pdae_adamw_step_gscale'):
        assert n in names, n
    with open(os.path.join(ROOT, 'include', 'pdae.h')) as f:
        header = f.read()
    assert 'pdae_adamw_step_gscale(' in header and 'pdae_grad_norm_clip(' in header


def test_finetune_config_keeps_reference_values():
    from point_dae_amd.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(CFG)
    assert cfg.grad_norm_clip == 10 and cfg.total_bs == 32 and cfg.npoints == 1024
    assert cfg.model.cls_dim == 40 and cfg.model.num_group == 64
    assert list(cfg.dataset.train.others.aug_type) == ['norm', 'scale', 'translate']
    assert list(cfg.dataset.val.others.aug_type) == ['norm']
    assert cfg.dataset.train._base_.NAME == 'ModelNet' and cfg.dataset.train._base_.NUM_CATEGORY == 40


@pytest.mark.parametrize('bs', [32, 5])
def test_modelnet_train_subset_drops_the_short_last_batch(bs):
    """The reference's train loader is built with drop_last (tools/builder.py): 2 bs + 1 clouds give 2 full batches and
    len() 2; the test subset keeps every cloud (3 batches, the last one of 1)."""
    from point_dae_amd.datasets import ModelNet
    count = 2 * bs + 1
    train = ModelNet(dict(subset='train', count=count, bs=bs, npoints=64, device='cpu', aug_type=['clean']))
    sizes = [data[0].shape[0] for _, _, data in train]
    assert sizes == [bs, bs] and len(train) == 2
    assert all(data[1].shape[0] == bs for _, _, data in train)
    test = ModelNet(dict(subset='test', count=count, bs=bs, npoints=64, device='cpu', aug_type=['clean']))
    sizes = [data[0].shape[0] for _, _, data in test]
    assert sizes == [bs, bs, 1] and len(test) == 3
    assert sum(sizes) == count
