"""DGCNN classifier (dgcnn_cls.DGCNN), CPU side: the state_dict layout and the Point_CAE_DGCNN_FCOnly checkpoint remap
against the live-reference fixture (tests/golden/dgcnn_cls_layout.json), the scratch init, the configuration, the new
ABI symbols, and no CPU path."""
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_dgcnn_smooth.yaml')


def _layout():
    with open(os.path.join(HERE, 'golden', 'dgcnn_cls_layout.json')) as f:
        return json.load(f)


def _model_cfg():
    from point_dae_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(CFG).model


def _model():
    from point_dae_amd.builder import model_builder
    return model_builder(_model_cfg())


def test_state_dict_matches_reference_layout():
    got = [[k, list(v.shape)] for k, v in _model().state_dict().items()]
    assert got == _layout()['state_dict']


def test_autoencoder_checkpoint_remap_reports_reference_keys(tmp_path):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_dgcnn import Point_CAE_DGCNN_FCOnly
    lay = _layout()
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, lay['pretrain_config'])).model
    pre_cfg.NAME = lay['pretrain_model']
    torch.manual_seed(1)
    pre = Point_CAE_DGCNN_FCOnly(pre_cfg)
    path = tmp_path / 'ckpt-last.pth'
    torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, str(path))
    model = _model()
    lines = []
    inc = model.load_model_from_ckpt(str(path), log=lines.append)
    assert sorted(inc.missing_keys) == lay['missing_keys']
    assert sorted(inc.unexpected_keys) == lay['unexpected_keys']
    assert all(k.startswith('cls_head_finetune.') for k in inc.missing_keys)
    assert all(k.startswith('recfc.') for k in inc.unexpected_keys)
    assert lines[0] == 'missing_keys' and 'unexpected_keys' in lines
    assert lines[-1].startswith('[Transformer] Successful Loading the ckpt from')
    sd = pre.state_dict()
    for k in ('dgcnn_encoder.conv1.0.weight', 'dgcnn_encoder.conv5.0.weight', 'dgcnn_encoder.bn5.running_var',
              'dgcnn_encoder.conv3.1.weight'):
        assert torch.equal(model.state_dict()[k], sd[k]), k


def test_scratch_init_touches_linear_and_conv1d_only():
    model = _model()
    torch.manual_seed(0)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    lines = []
    assert model.load_model_from_ckpt(None, log=lines.append) is None
    assert lines == ['Training from scratch!!!']
    after = model.state_dict()
    enc, head = model.dgcnn_encoder, model.cls_head_finetune
    # Linear layers and conv5's Conv1d: trunc-normal(std 0.02) weights (timm's absolute cut-offs +-2), zero biases
    for lin in (head[0], head[3], head[7]):
        assert 0.015 < float(lin.weight.detach().std()) < 0.025
        assert float(lin.bias.detach().abs().max()) == 0.0
    w5 = enc.conv5[0].weight
    assert not torch.equal(w5, before['dgcnn_encoder.conv5.0.weight'])
    assert 0.015 < float(w5.detach().std()) < 0.025
    # the Conv2d layers and every BatchNorm keep torch's default init
    for k in before:
        if k.startswith('dgcnn_encoder.conv5.0.') or k.startswith(('cls_head_finetune.0.', 'cls_head_finetune.3.',
                                                                   'cls_head_finetune.7.')):
            continue
        assert torch.equal(after[k], before[k]), k


def test_config_parses_to_reference_values():
    from point_dae_amd.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(CFG)
    assert cfg.optimizer.type == 'AdamW' and cfg.optimizer.part == 'all'
    assert cfg.optimizer.kwargs.lr == 0.0005 and cfg.optimizer.kwargs.weight_decay == 0.05
    assert cfg.scheduler.type == 'CosLR'
    assert cfg.scheduler.kwargs.epochs == 200 and cfg.scheduler.kwargs.initial_epochs == 10
    assert cfg.max_epoch == 200 and cfg.npoints == 1024 and cfg.total_bs == 32 and cfg.grad_norm_clip == 10
    assert cfg.step_per_update == 1
    assert cfg.model.NAME == 'DGCNN' and cfg.model.smoothloss is True and cfg.model.cls_dim == 40
    # the Transformer keys the reference's file carries parse and are not used
    assert cfg.model.trans_dim == 384 and cfg.model.num_group == 128
    assert list(cfg.dataset.train.others.aug_type) == ['norm', 'scale', 'translate']
    assert cfg.dataset.train.others.subset == 'train' and cfg.dataset.train.others.npoints == 1024
    for split in ('val', 'test'):
        assert list(cfg.dataset[split].others.aug_type) == ['norm']
        assert cfg.dataset[split].others.subset == 'test'
    assert cfg.dataset.train._base_.NAME == 'ModelNet' and cfg.dataset.train._base_.NUM_CATEGORY == 40
    model = _model()
    assert model.smoothing and model.cls_dim == 40


def test_new_abi_symbols_are_bound():
    from point_dae_amd import _lib
    names = set(_lib.exported_symbols())
    new = ('pdae_bn_lrelu_dropout', 'pdae_bn_lrelu_dropout_grad', 'pdae_softmax_xent_smooth',
           'pdae_softmax_xent_smooth_grad')
    for n in new:
        assert n in names, n
    with open(os.path.join(ROOT, 'include', 'pdae.h')) as f:
        header = f.read()
    for n in new:
        assert n + '(' in header, n


def test_forward_and_ops_raise_off_gpu():
    from point_dae_amd import finetune_ops as F
    model = _model()
    with pytest.raises(RuntimeError, match='GPU'):
        model(torch.zeros(2, 1024, 3))
    with pytest.raises(RuntimeError, match='GPU'):
        F.bn_lrelu_dropout(torch.zeros(4, 8), torch.nn.BatchNorm1d(8), 0.5, 0.2)
    with pytest.raises(RuntimeError, match='GPU'):
        F.softmax_xent_smooth(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), 0.3)


def test_too_many_classes_raise_at_construction():
    from point_dae_amd.dgcnn_cls import DGCNN
    cfg = _model_cfg()
    cfg.cls_dim = 65
    with pytest.raises(NotImplementedError, match='classes'):
        DGCNN(cfg)
