"""Part segmentation (point_dae_amd/part_seg.py, partseg_ops.py, datasets.ShapeNetPart, main.py --part_seg), the checks
that need no GPU.

tests/golden/partseg_{a,b}.npz and partseg_layout.json hold the LIVE reference's outputs (make_partseg_fixtures.py): its
segmentation model's fp64 log-probabilities on a seeded subset of the points, the geometric decisions they rest on, the
state_dict layout, and what the reference's own load_model_from_ckpt reports for a pretraining checkpoint of this
repository.  tests/golden/shapenetpart_mini/ is a synthetic root in the dataset's file format (two categories, five
shapes of 40 to 60 points)."""
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
import partseg_restatement as R  # noqa: E402
import weights  # noqa: E402

CONFIG = 'cfgs/segmentation_shapenetpart_transformer.yaml'
SEEDS = {'a': 3, 'b': 7}
MINI = os.path.join(ROOT, 'tests', 'golden', 'shapenetpart_mini')


def layout():
    with open(os.path.join(ROOT, 'tests', 'golden', 'partseg_layout.json')) as fh:
        return json.load(fh)


def fixture(which):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'partseg_%s.npz' % which))


def build_model(**changes):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    cfg = cfg_from_yaml_file(os.path.join(ROOT, CONFIG)).model
    for k, v in changes.items():
        cfg[k] = v
    return MODELS.build(cfg)


@pytest.mark.parametrize('which', ['a', 'b'])
def test_restatement_in_fp64_reproduces_the_live_reference(which):
    """The fp64 restatement, fed the recorded FPS / kNN indices, against the reference's fp64 log-probabilities: 1e-12 of
    the largest entry (the reference's matmul-form distance moves d by ~1e-16; the printed figure shows what that does)."""
    f = fixture(which)
    assert int(f['seed']) == SEEDS[which]
    model = weights.fill_state(build_model(), int(f['seed']))
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    got = R.forward(torch.from_numpy(f['pts']).double(), torch.from_numpy(f['cls']), sd, torch.from_numpy(f['fps_idx']),
                    torch.from_numpy(f['knn_idx']))
    assert torch.equal(got['three_idx'], torch.from_numpy(f['three_idx']).long())
    assert R.third_fourth_gap(torch.from_numpy(f['pts']), got['center']) >= 1e-6
    sub = torch.from_numpy(f['sub_idx']).long()
    logp = torch.gather(got['logp'], 1, sub.unsqueeze(-1).expand(-1, -1, 50)).numpy()
    want = f['logp64']
    err = np.abs(logp - want).max() / np.abs(want).max()
    print('%s: restatement fp64 vs reference fp64 %.2e; reference fp32 vs fp64 %.2e' % (which, err, float(f['dist'])))
    assert want.shape == (2, 256, 50) and err <= 1e-12
    assert np.array_equal(got['logp'].argmax(-1).numpy(), f['argmax64'])
    assert float(f['dist']) <= 1e-6
    assert float((f['margin64'] < 100 * 1e-5 * float(f['scale64'])).mean()) <= 0.01


def test_state_dict_layout_equals_the_reference():
    lay = layout()
    model = build_model()
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == lay['state_dict']
    assert len(sd) == 192 and sum(p.numel() for p in model.parameters()) == lay['parameters'] == 27063730
    assert not any(k.startswith(('cls_token', 'cls_pos', 'cls_head_finetune')) for k in sd)


def test_reference_checkpoints_load_under_both_layouts(tmp_path):
    src = weights.fill_state(build_model(), 5)
    want = src.state_dict()
    path = str(tmp_path / 'best_model.pth')
    torch.save({'epoch': 3, 'model_state_dict': want}, path)
    model = build_model()
    assert model.load_segmentation_checkpoint(path, log=lambda s: None) == []
    assert all(torch.equal(v, want[k]) for k, v in model.state_dict().items())
    old = {k.replace('_cls', ''): v for k, v in want.items()}
    assert sum(k not in want for k in old) == 36                      # every head entry carries the suffix
    torch.save({'model_state_dict': old}, path)
    model, lines = build_model(), []
    renamed = model.load_segmentation_checkpoint(path, log=lines.append)
    assert sorted(renamed) == sorted(k for k in want if '_cls' in k) and len(renamed) == 36
    assert all(torch.equal(v, want[k]) for k, v in model.state_dict().items())
    assert any('renamed' in ln for ln in lines)
    del old['convs3.weight']
    torch.save({'model_state_dict': old}, path)
    with pytest.raises(RuntimeError, match='convs3'):
        build_model().load_segmentation_checkpoint(path, log=lambda s: None)
    torch.save({'base_model': want}, path)
    with pytest.raises(RuntimeError, match='model_state_dict'):
        build_model().load_segmentation_checkpoint(path, log=lambda s: None)


def test_pretraining_checkpoint_reports_the_recorded_keys(tmp_path):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    lay = layout()
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, lay['pretrain_config'])).model
    pre_cfg.NAME = lay['pretrain_model']
    build_model()                                                      # (registers the models)
    pre = weights.fill_state(MODELS.build(pre_cfg), 3)
    path = str(tmp_path / 'ckpt-last.pth')
    torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, path)
    model, lines = build_model(), []
    inc = model.load_model_from_ckpt(path, log=lines.append)
    assert sorted(inc.missing_keys) == lay['missing_keys'] and len(lay['missing_keys']) == 31
    assert all('_cls' in k for k in inc.missing_keys)                   # the head, and only the head
    assert sorted(inc.unexpected_keys) == lay['unexpected_keys'] and len(lay['unexpected_keys']) > 0
    text = '\n'.join(lines)
    assert 'missing_keys' in text and 'unexpected_keys' in text


def test_model_refusals():
    model = build_model()
    with pytest.raises(RuntimeError, match='GPU'):
        model.eval()(torch.rand(2, 64, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(NotImplementedError, match='training is not built'):
        model.train()(torch.rand(2, 64, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(NotImplementedError, match='three nearest'):
        build_model(num_group=2)
    with pytest.raises(NotImplementedError, match='at most 128'):
        build_model(num_group=129)


def test_backend_switch(monkeypatch):
    from point_dae_amd import partseg_ops
    monkeypatch.delenv('PDAE_PARTSEG', raising=False)
    assert partseg_ops.mode() == 'hip'
    monkeypatch.setenv('PDAE_PARTSEG', 'layers')
    assert partseg_ops.mode() == 'layers'
    monkeypatch.setenv('PDAE_PARTSEG', 'eager')
    with pytest.raises(ValueError, match='PDAE_PARTSEG'):
        partseg_ops.mode()


def test_seg_classes_table():
    from point_dae_amd import partseg_ops
    labels = sorted(l for ls in partseg_ops.SEG_CLASSES.values() for l in ls)
    assert labels == list(range(50)) and len(partseg_ops.SEG_CLASSES) == 16
    assert all(ls == list(range(ls[0], ls[-1] + 1)) for ls in partseg_ops.SEG_CLASSES.values())
    assert partseg_ops.SEG_CLASSES['Laptop'] == [28, 29] and partseg_ops.SEG_CLASSES['Motorbike'] == [30, 31, 32, 33, 34, 35]
    cat_of, lo, hi = partseg_ops.label_tables()
    assert partseg_ops.CATEGORIES[cat_of[33]] == 'Motorbike' and (lo[cat_of[33]], hi[cat_of[33]]) == (30, 35)


# ---- the dataset reader ----------------------------------------------------------------------------------------------
def _mini(split, **kw):
    from point_dae_amd import datasets
    cfg = dict(DATA_PATH=MINI, subset=split, npoints=32, bs=2, device='cpu', seed=0)
    cfg.update(kw)
    return datasets.ShapeNetPart(cfg)


def test_dataset_reader_on_the_mini_root():
    from point_dae_amd import datasets, partseg_ops
    names = {'trainval': ['a1', 'c3', 'e5'], 'train': ['a1', 'e5'], 'val': ['c3'], 'test': ['b2', 'd4']}
    for split, want in names.items():
        d = _mini(split)
        assert d.listed and MINI in d.source
        assert [os.path.basename(p)[:-4] for p in d.paths] == want, split       # category by category, names sorted
        assert [c for c, _ in d.categories] == ['Laptop', 'Motorbike']
        assert d.cls.tolist() == [0 if n in ('a1', 'b2', 'c3') else 1 for n in want]
        assert d.offsets[-1] == d.points.shape[0] == d.seg.shape[0] and len(d.offsets) == len(want) + 1
    with pytest.raises(ValueError, match='unknown split'):
        _mini('all')
    d = _mini('test')
    raw = np.loadtxt(os.path.join(MINI, '03642806', 'b2.txt')).astype(np.float32)
    assert 40 <= len(raw) <= 60 and d.offsets[1] == len(raw)
    want = datasets.pc_normalize(raw[:, 0:3])
    assert np.array_equal(d.points[:len(raw)].numpy(), want)                       # columns 0:3, normalised once
    assert abs(float(np.sqrt((want ** 2).sum(1)).max()) - 1.0) < 1e-6 and np.abs(want.mean(0)).max() < 1e-6
    assert np.array_equal(d.seg[:len(raw)].numpy(), raw[:, -1].astype(np.int32))   # the last column
    batches = list(d)
    assert len(batches) == len(d) == 1
    _, _, (pts, cls, seg) = batches[0]
    assert pts.shape == (2, 32, 3) and cls.tolist() == [0, 1] and seg.shape == (2, 32) and seg.dtype == torch.int32
    for i, cat in enumerate(('Laptop', 'Motorbike')):
        parts = partseg_ops.SEG_CLASSES[cat]
        assert set(seg[i].tolist()) <= set(parts)
        assert int(seg[i, 0]) in parts                                             # seg[:, 0] identifies the category
        rows = d.points[d.offsets[i]:d.offsets[i + 1]]
        assert all(bool((rows == p).all(1).any()) for p in pts[i])                 # resampled with replacement from the shape
    again = list(_mini('test'))[0][2]
    assert torch.equal(again[0], pts) and torch.equal(again[2], seg)               # the host generator is seeded
    assert len(_mini('trainval', bs=2)) == 2                                        # the short last batch is kept


def test_synthetic_stand_in():
    from point_dae_amd import datasets, partseg_ops
    d = datasets.ShapeNetPart(dict(DATA_PATH='data/nowhere', subset='test', npoints=64, bs=8, device='cpu', count=16))
    assert not d.listed and d.source.startswith('synthetic stand-in (no data/nowhere')
    assert sorted(d.cls.tolist()) == list(range(16))
    _, lo, hi = partseg_ops.label_tables()
    for _, _, (pts, cls, seg) in d:
        assert pts.shape == (8, 64, 3) and float(pts.norm(dim=-1).max()) <= 1.0 + 1e-6
        for i in range(8):
            k = int(cls[i])
            assert lo[k] <= int(seg[i].min()) and int(seg[i].max()) <= hi[k]
            assert lo[k] <= int(seg[i, 0]) <= hi[k]


# ---- the metric ------------------------------------------------------------------------------------------------------
def test_metric_on_a_hand_worked_case():
    """Three shapes of six points.  Shape 0 (Laptop, parts 28-29): truth all 28, prediction all 28 -> part 28 IoU 6/6,
    part 29 in neither: 1.0; shape IoU 1.  Shape 1 (Laptop): truth all 28, prediction 28 28 28 29 29 29 -> part 28 3/6,
    part 29 predicted but absent from the truth: 0/3 = 0; shape IoU 0.25.  Shape 2 (Motorbike, 30-35): truth
    30 30 31 31 32 32, prediction 30 31 31 31 32 33 -> 30: 1/2, 31: 2/3, 32: 1/2, 33: 0/1, 34 and 35 in neither: 1.0;
    shape IoU (0.5 + 2/3 + 0.5 + 0 + 1 + 1) / 6 = 11/18."""
    classes = {'Laptop': [28, 29], 'Motorbike': [30, 31, 32, 33, 34, 35]}
    seg = np.array([[28] * 6, [28] * 6, [30, 30, 31, 31, 32, 32]])
    pred = np.array([[28] * 6, [28, 28, 28, 29, 29, 29], [30, 31, 31, 31, 32, 33]])
    m = R.metric(pred, seg, classes)
    assert m['accuracy'] == 13 / 18
    assert m['category_iou']['Laptop'] == 0.625 and abs(m['category_iou']['Motorbike'] - 11 / 18) < 1e-15
    assert abs(m['class_avg_iou'] - (0.625 + 11 / 18) / 2) < 1e-15
    assert abs(m['inctance_avg_iou'] - (1 + 0.25 + 11 / 18) / 3) < 1e-15
    c = m['counts']
    assert c['part_seen'][28:33].tolist() == [12, 0, 2, 2, 2] and c['part_correct'][28:33].tolist() == [9, 0, 1, 2, 1]
    assert c['shape_correct'].tolist() == [6, 3, 4]
    assert c['shape_iu'][1, :, 28:30].tolist() == [[3, 0], [6, 3]]
    assert c['shape_iu'][2, :, 30:36].tolist() == [[1, 2, 1, 0, 0, 0], [2, 3, 2, 1, 0, 0]]
    assert np.isnan(m['class_avg_accuracy'])                 # labels never seen divide 0 by 0, as in the reference
    # the product's host side forms the same numbers from the same counts
    from point_dae_amd import partseg_ops
    cat_of, _, _ = partseg_ops.label_tables()
    got = partseg_ops.metrics(dict(shape_iu=c['shape_iu'], shape_correct=c['shape_correct'], shape_cat=cat_of[seg[:, 0]],
                                   part_seen=c['part_seen'], part_correct=c['part_correct'], points=18))
    assert got['accuracy'] == m['accuracy'] and abs(got['inctance_avg_iou'] - m['inctance_avg_iou']) < 1e-15
    assert got['category_iou']['Laptop'] == 0.625 and abs(got['category_iou']['Motorbike'] - 11 / 18) < 1e-15
    assert np.isnan(got['category_iou']['Table']) and np.isnan(got['class_avg_accuracy'])


# ---- the command line ------------------------------------------------------------------------------------------------
def test_main_routing(tmp_path, monkeypatch):
    from point_dae_amd import main, parser
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    cfg = os.path.join(ROOT, CONFIG)
    with pytest.raises(NotImplementedError, match='part-segmentation training is not built'):
        main.main(['--config', cfg, '--part_seg', '--scratch_model'])
    with pytest.raises(NotImplementedError, match='one process'):
        main.main(['--config', cfg, '--part_seg', '--test', '--scratch_model', '--launcher', 'pytorch'])
    with pytest.raises(ValueError, match='ckpts'):
        parser.get_args(['--config', cfg, '--part_seg', '--test'])
    args = parser.get_args(['--config', cfg, '--part_seg', '--test', '--scratch_model'])
    assert args.part_seg and args.test and args.ckpts is None
    assert not parser.get_args(['--config', cfg]).part_seg


def test_config_values(monkeypatch):
    from point_dae_amd.config import cfg_from_yaml_file
    monkeypatch.chdir(ROOT)
    cfg = cfg_from_yaml_file(os.path.join(ROOT, CONFIG))
    assert (cfg.npoints, cfg.total_bs, cfg.model.cls_dim, cfg.model.num_categories) == (2048, 16, 50, 16)
    assert (cfg.model.trans_dim, cfg.model.depth, cfg.model.num_heads, cfg.model.group_size, cfg.model.num_group) == \
        (384, 12, 6, 32, 128)
    assert cfg.dataset.test._base_.NAME == 'ShapeNetPart' and cfg.dataset.test.others.subset == 'test'
    assert cfg.dataset.test._base_.DATA_PATH == 'data/shapenetcore_partanno_segmentation_benchmark_v0_normal'
