"""DGCNN part segmentation (point_dae_amd/dgcnn_partseg.py, main.py --part_seg with
cfgs/segmentation_shapenetpart_dgcnn.yaml), the checks that need no GPU.

tests/golden/dgcnn_partseg_{a,b}.npz and dgcnn_partseg_layout.json hold the LIVE reference's outputs
(make_dgcnn_partseg_fixtures.py): its DGCNN segmentation model's fp64 logits on a seeded subset of the points, the three
graphs they rest on, the state_dict layout, and what the reference's own load_model_from_ckpt reports for a checkpoint
with the keys of its Point_CAE_DGCNN_PartSeg."""
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
import dgcnn_partseg_restatement as R  # noqa: E402
import weights  # noqa: E402

CONFIG = 'cfgs/segmentation_shapenetpart_dgcnn.yaml'
SEEDS = {'a': 11, 'b': 12}
PIN = 1e-5
GAP_FACTOR = 8.0


def layout():
    with open(os.path.join(ROOT, 'tests', 'golden', 'dgcnn_partseg_layout.json')) as fh:
        return json.load(fh)


def fixture(which):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'dgcnn_partseg_%s.npz' % which))


def build_model(**changes):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    cfg = cfg_from_yaml_file(os.path.join(ROOT, CONFIG)).model
    for k, v in changes.items():
        cfg[k] = v
    return MODELS.build(cfg)


def state64(model):
    return {k: (v.double().cpu() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}


@pytest.mark.parametrize('which', ['a', 'b'])
def test_restatement_in_fp64_reproduces_the_live_reference(which):
    """The fp64 restatement, fed the recorded graphs, against the reference's fp64 logits: 1e-10 of the largest entry."""
    f = fixture(which)
    assert int(f['seed']) == SEEDS[which]
    model = weights.fill_state(build_model(), int(f['seed']))
    graphs = torch.from_numpy(f['graphs'].astype(np.int64))
    assert graphs.shape == (3, 2, 512, 20) and f['graphs'].dtype == np.int16
    got = R.forward(torch.from_numpy(f['pts']).double(), torch.from_numpy(f['cls']), state64(model), graphs)
    sub = torch.from_numpy(f['sub_idx']).long()
    logits = torch.gather(got['logits'], 1, sub.unsqueeze(-1).expand(-1, -1, 50)).numpy()
    want = f['logits64']
    err = np.abs(logits - want).max() / np.abs(want).max()
    print('%s: restatement fp64 vs reference fp64 %.2e; reference fp32 vs fp64 %.2e' % (which, err, float(f['dist'])))
    assert want.shape == (2, 256, 50) and err <= 1e-10
    assert np.array_equal(got['logits'].argmax(-1).numpy(), f['argmax64'])
    assert abs(float(np.abs(got['logits'].numpy()).max()) - float(f['scale64'])) <= 1e-10 * float(f['scale64'])
    # the fixture's own conditions, as its maker asserted them
    assert float(f['dist']) <= 1e-6
    assert float((f['margin64'] < 100 * PIN * float(f['scale64'])).mean()) <= 0.01
    assert f['gap64'].shape == (3, 2, 512) and f['pd_err'].shape == (3,)
    for l in range(3):
        assert float((f['gap64'][l] < GAP_FACTOR * f['pd_err'][l]).mean()) <= 0.02
    # the recorded graphs are the k largest of the reference's distance expression on the restatement's features
    feats = (torch.from_numpy(f['pts']).double(), got['x1'], got['x2'])
    for l in range(3):
        pd = R.knn_distance(feats[l])
        top = pd.topk(21, dim=-1)[0]
        assert np.allclose((top[..., 19] - top[..., 20]).numpy(), f['gap64'][l], rtol=0, atol=1e-9)
        own = pd.topk(20, dim=-1)[1].sort(-1)[0]
        clear = torch.from_numpy(f['gap64'][l] >= GAP_FACTOR * f['pd_err'][l])
        assert torch.equal(own[clear], graphs[l].sort(-1)[0][clear])


def test_state_dict_layout_equals_the_reference():
    lay = layout()
    model = build_model()
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == lay['state_dict']
    assert sum(p.numel() for p in model.parameters()) == lay['parameters']
    # both key sets of every BatchNorm, as point_cae_dgcnn.dgcnn_encoder carries them
    for i in range(1, 7):
        assert 'dgcnn_encoder.bn%d.weight' % i in sd and 'dgcnn_encoder.conv%d.1.weight' % i in sd
        assert sd['dgcnn_encoder.bn%d.weight' % i].data_ptr() == sd['dgcnn_encoder.conv%d.1.weight' % i].data_ptr()
    for i in range(7, 11):
        assert sd['bn%d.running_var' % i].data_ptr() == sd['conv%d.1.running_var' % i].data_ptr()
    assert tuple(sd['conv8.0.weight'].shape) == (256, 1280, 1) and tuple(sd['conv11.weight'].shape) == (50, 128, 1)
    assert not any('bias' in k for k in sd if k.endswith(('.0.bias', 'conv11.bias')))


def test_reference_segmentation_checkpoints_load_strictly(tmp_path):
    src = weights.fill_state(build_model(), 5)
    want = src.state_dict()
    path = str(tmp_path / 'best_model.pth')
    for prefix in ('', 'module.'):
        torch.save({'epoch': 3, 'model_state_dict': {prefix + k: v for k, v in want.items()}}, path)
        model = build_model()
        assert model.load_segmentation_checkpoint(path, log=lambda s: None) == []
        assert all(torch.equal(v, want[k]) for k, v in model.state_dict().items())
    short = {k: v for k, v in want.items() if k != 'conv11.weight'}
    torch.save({'model_state_dict': short}, path)
    with pytest.raises(RuntimeError, match='conv11'):
        build_model().load_segmentation_checkpoint(path, log=lambda s: None)
    extra = dict(want)
    extra['convs3_cls.weight'] = torch.zeros(1)                       # (there is no renaming: the Transformer's names are foreign)
    torch.save({'model_state_dict': extra}, path)
    with pytest.raises(RuntimeError, match='convs3_cls'):
        build_model().load_segmentation_checkpoint(path, log=lambda s: None)
    torch.save({'base_model': want}, path)
    with pytest.raises(RuntimeError, match='model_state_dict'):
        build_model().load_segmentation_checkpoint(path, log=lambda s: None)


def test_pretraining_checkpoint_reports_the_recorded_keys(tmp_path):
    lay = layout()
    gen = torch.Generator().manual_seed(3)
    pre = {'module.' + k: torch.randn(shape, generator=gen) if len(shape) else torch.zeros((), dtype=torch.long)
           for k, shape in lay['pretrain_state_dict']}
    path = str(tmp_path / 'ckpt-last.pth')
    torch.save({'base_model': pre}, path)
    model, lines = build_model(), []
    inc = model.load_model_from_ckpt(path, log=lines.append)
    assert sorted(inc.missing_keys) == lay['missing_keys'] and len(lay['missing_keys']) > 0
    assert not any(k.startswith('dgcnn_encoder.') for k in inc.missing_keys)       # the head, and only the head
    assert sorted(inc.unexpected_keys) == lay['unexpected_keys'] and len(lay['unexpected_keys']) > 0
    assert all(k.startswith('folding') for k in inc.unexpected_keys)                # the decoder, and only the decoder
    assert torch.equal(model.state_dict()['dgcnn_encoder.conv6.0.weight'], pre['module.dgcnn_encoder.conv6.0.weight'])
    text = '\n'.join(lines)
    assert 'missing_keys' in text and 'unexpected_keys' in text


def test_model_refusals():
    model = build_model()
    with pytest.raises(RuntimeError, match='GPU'):
        model.eval()(torch.rand(2, 64, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(NotImplementedError, match='training is not built'):
        model.train()(torch.rand(2, 64, 3), torch.zeros(2, dtype=torch.long))
    from point_dae_amd.dgcnn_partseg import DGCNNPartSeg
    import inspect
    assert list(inspect.signature(DGCNNPartSeg.forward).parameters)[1:] == ['pts', 'cls_label', 'seg', 'counts', 'capture',
                                                                            'graphs']


def test_one_hot_label_is_refused(monkeypatch):
    """The label is the (B,) category id; the check sits in front of any kernel (is_cuda is stubbed to reach it)."""
    model = build_model().eval()
    pts = torch.rand(2, 64, 3)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    with pytest.raises(ValueError, match='not a one-hot'):
        model(pts, torch.zeros(2, 16))
    with pytest.raises(ValueError, match='not a one-hot'):
        model(pts, torch.zeros(3, dtype=torch.long))


def test_backend_switch(monkeypatch):
    from point_dae_amd import dgcnn_partseg
    monkeypatch.delenv('PDAE_PARTSEG', raising=False)
    assert dgcnn_partseg.mode() == dgcnn_partseg.DEFAULT_MODE and dgcnn_partseg.DEFAULT_MODE in ('hip', 'layers')
    assert build_model().partseg_mode() == dgcnn_partseg.DEFAULT_MODE
    for m in ('hip', 'layers'):
        monkeypatch.setenv('PDAE_PARTSEG', m)
        assert dgcnn_partseg.mode() == m
    monkeypatch.setenv('PDAE_PARTSEG', 'eager')
    with pytest.raises(ValueError, match='PDAE_PARTSEG'):
        dgcnn_partseg.mode()


def test_header_declares_the_new_entries():
    from point_dae_amd import _lib
    names = _lib.exported_symbols()
    for name in ('pdae_edge2_eval_supported', 'pdae_edge2_eval_forward', 'pdae_partseg_cloud_bias_lrelu',
                 'pdae_partseg_logits_tail'):
        assert name in names


def test_config_values(monkeypatch):
    from point_dae_amd.config import cfg_from_yaml_file
    monkeypatch.chdir(ROOT)
    cfg = cfg_from_yaml_file(os.path.join(ROOT, CONFIG))
    assert (cfg.npoints, cfg.total_bs, cfg.model.NAME, cfg.model.cls_dim, cfg.model.num_categories) == \
        (2048, 16, 'DGCNNPartSeg', 50, 16)
    assert cfg.dataset.test._base_.NAME == 'ShapeNetPart' and cfg.dataset.test.others.subset == 'test'
    assert cfg.dataset.test.others.npoints == 2048
    assert cfg.dataset.test._base_.DATA_PATH == 'data/shapenetcore_partanno_segmentation_benchmark_v0_normal'
    tr = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs/segmentation_shapenetpart_transformer.yaml'))
    assert cfg.dataset == tr.dataset                                   # the Transformer's config with another model


def test_main_routes_part_seg_test_to_the_runner(tmp_path, monkeypatch):
    from point_dae_amd import main, parser, runner_finetune
    monkeypatch.chdir(ROOT)
    monkeypatch.setenv('LOCAL_RANK', '0')
    cfg = os.path.join(ROOT, CONFIG)
    with pytest.raises(NotImplementedError, match='part-segmentation training is not built'):
        main.main(['--config', cfg, '--part_seg', '--scratch_model'])
    with pytest.raises(ValueError, match='ckpts'):
        parser.get_args(['--config', cfg, '--part_seg', '--test'])
    seen = {}

    def fake(args, config):
        seen['model'] = config.model.NAME
        seen['bs'] = config.total_bs
    monkeypatch.setattr(runner_finetune, 'part_seg_test', fake)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    main.main(['--config', cfg, '--part_seg', '--test', '--scratch_model', '--exp_name', 'ci_dgcnn_partseg', '--root_folder',
               os.path.relpath(str(tmp_path / 'exp'), ROOT)])
    assert seen == {'model': 'DGCNNPartSeg', 'bs': 16}
