"""The linear-SVM evaluation protocol (--svm_classification, DGCNN_feat), CPU side: the flag and its dispatch, the new
configuration and DGCNN_feat's layout against the live-reference fixture (tests/golden/dgcnn_feat_layout.json, written by
tests/golden/make_svm_fixtures.py), the checkpoint remap, no CPU path, and the host class layout of svm_ops against
sklearn's own SVC."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG_NAME = 'finetune_modelnet_svm_dgcnn.yaml'
CFG = os.path.join(ROOT, 'cfgs', CFG_NAME)


def _layout():
    with open(os.path.join(HERE, 'golden', 'dgcnn_feat_layout.json')) as f:
        return json.load(f)


def _model():
    from point_dae_amd.builder import model_builder
    from point_dae_amd.config import cfg_from_yaml_file
    return model_builder(cfg_from_yaml_file(CFG).model)


def test_parser_accepts_svm_classification(tmp_path, monkeypatch):
    from point_dae_amd import parser
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    assert parser.get_args(['--config', CFG]).svm_classification is False
    assert parser.get_args(['--config', CFG, '--svm_classification']).svm_classification is True


@pytest.mark.parametrize('flags,taken', [(['--scratch_model', '--svm_classification'], 'svm_classification'),
                                         (['--finetune_model', '--svm_classification'], 'svm_classification'),
                                         (['--scratch_model', '--svm_classification', '--so3_rotation'], 'svm_classification'),
                                         (['--scratch_model'], 'run_net')])
def test_main_dispatches_to_svm_classification(tmp_path, monkeypatch, flags, taken):
    """main.py:101-109 of the reference: under --finetune_model / --scratch_model the flag is looked at first."""
    from point_dae_amd import main, runner_finetune
    calls = []
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    for name in ('run_net', 'run_net_rotation', 'svm_classification'):
        monkeypatch.setattr(runner_finetune, name, lambda args, config, name=name: calls.append(name), raising=False)
    main.main(['--config', CFG, *flags])
    assert calls == [taken]


def test_main_refuses_the_distributed_launcher(tmp_path, monkeypatch):
    from point_dae_amd import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    with pytest.raises(ValueError, match='one process'):
        main.main(['--config', CFG, '--scratch_model', '--svm_classification', '--launcher', 'pytorch'])


def test_new_config_equals_the_reference_values():
    from point_dae_amd.config import cfg_from_yaml_file
    entry = _layout()['configs'][CFG_NAME]
    want = entry['values']
    with open(CFG) as f:
        assert yaml.safe_load(f) == want
    assert entry['changes'] == {'model.NAME': 'DGCNN_feat'}
    cfg = cfg_from_yaml_file(CFG)
    assert cfg.model.NAME == 'DGCNN_feat' and cfg.model.smoothloss is True and cfg.model.cls_dim == 40
    assert cfg.npoints == 1024 and cfg.total_bs == 32
    for split in ('train', 'val', 'test'):
        assert list(cfg.dataset[split].others.aug_type) == ['norm']
        assert cfg.dataset[split].others.npoints == 1024
    assert cfg.dataset.train.others.subset == 'train' and cfg.dataset.val.others.subset == 'test'


def test_state_dict_matches_reference_layout():
    model = _model()
    assert type(model).__name__ == 'DGCNN_feat'
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == _layout()['state_dict']
    assert all(k.startswith('dgcnn_encoder.') for k, _ in got)
    assert [n for n, _ in model.named_children()] == ['dgcnn_encoder']


def test_autoencoder_checkpoint_loads_with_only_recfc_unexpected(tmp_path):
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
    assert list(inc.missing_keys) == [] == lay['missing_keys']
    assert sorted(inc.unexpected_keys) == lay['unexpected_keys']
    assert inc.unexpected_keys and all(k.startswith('recfc.') for k in inc.unexpected_keys)
    assert 'missing_keys' not in lines and 'unexpected_keys' in lines
    sd = pre.state_dict()
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_helpers_are_the_classifiers():
    """get_loss_acc / load_model_from_ckpt are inherited, not copied."""
    from point_dae_amd.classifier import Classifier
    from point_dae_amd.dgcnn_cls import DGCNN, DGCNN_feat
    assert issubclass(DGCNN_feat, DGCNN)
    assert DGCNN_feat.get_loss_acc is Classifier.get_loss_acc
    assert DGCNN_feat.load_model_from_ckpt is Classifier.load_model_from_ckpt
    model = _model()
    assert model.smooth_eps == 0.3
    lines = []
    assert model.load_model_from_ckpt(None, log=lines.append) is None
    assert lines == ['Training from scratch!!!']


def test_forward_and_solver_raise_off_gpu():
    from point_dae_amd import svm_ops
    with pytest.raises(RuntimeError, match='GPU'):
        _model()(torch.zeros(2, 256, 3))
    with pytest.raises(RuntimeError, match='GPU'):
        svm_ops.fit_predict_ovo(torch.zeros(8, 4), np.arange(8) % 2, torch.zeros(3, 4))


def test_new_abi_symbols_are_bound():
    from point_dae_amd import _lib
    names = set(_lib.exported_symbols())
    with open(os.path.join(ROOT, 'include', 'pdae.h')) as f:
        header = f.read()
    for n in ('pdae_svm_ovo_train', 'pdae_svm_ovo_predict', 'pdae_svm_ovo_supported'):
        assert n in names and n + '(' in header, n


def test_backend_selection(monkeypatch):
    from point_dae_amd import svm_ops
    monkeypatch.delenv('PDAE_SVM', raising=False)
    assert svm_ops.backend() == 'hip'
    monkeypatch.setenv('PDAE_SVM', 'sklearn')
    assert svm_ops.backend() == 'sklearn'
    monkeypatch.setenv('PDAE_SVM', 'libsvm')
    with pytest.raises(ValueError, match='PDAE_SVM'):
        svm_ops.backend()
    assert svm_ops.SVM_CS == (0.001, 0.01, 0.1, 1, 10, 100)


def test_class_layout_is_sklearns():
    """Labels with gaps in the ids and unequal class sizes: the classes, the class-ordered samples, the pair order and the
    dual_coef_ row rule of svm_ops reproduce what sklearn's SVC holds after a fit -- its ovo decision values rebuilt from
    dual_coef_ through class_layout / pairs / coef_row equal its own."""
    from sklearn.svm import SVC
    from point_dae_amd import svm_ops
    rng = np.random.default_rng(3)
    ids, sizes = np.array([7, 2, 11, 30]), [9, 4, 13, 6]
    y = rng.permutation(np.repeat(ids, sizes))
    means = rng.standard_normal((31, 6))
    X = means[y] + 0.7 * rng.standard_normal((len(y), 6))
    Xt = rng.standard_normal((10, 6))
    classes, order, class_ptr = svm_ops.class_layout(y)
    K = len(classes)
    assert classes.tolist() == [2, 7, 11, 30] and class_ptr.tolist() == [0, 4, 13, 26, 32]
    for k in range(K):                                   # class order, each class in input order (a stable sort)
        members = order[class_ptr[k]:class_ptr[k + 1]]
        assert (y[members] == classes[k]).all() and (np.diff(members) > 0).all()
    assert svm_ops.pairs(K) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    clf = SVC(C=1.0, kernel='linear', decision_function_shape='ovo').fit(X, y)
    assert clf.classes_.tolist() == classes.tolist()
    # dual_coef_ over ALL samples in class order (zeros at the non-support vectors), as the kernels write it
    pos_of = {int(s): i for i, s in enumerate(order)}
    coef = np.zeros((K - 1, len(y)))
    cols = [pos_of[int(s)] for s in clf.support_]
    assert cols == sorted(cols)                          # libsvm's support vectors come in the same order
    coef[:, cols] = clf.dual_coef_
    gram = Xt @ X[order].T
    dec = np.zeros((len(Xt), K * (K - 1) // 2))
    for k, (p, q) in enumerate(svm_ops.pairs(K)):
        sp, sq = slice(class_ptr[p], class_ptr[p + 1]), slice(class_ptr[q], class_ptr[q + 1])
        dec[:, k] = (gram[:, sp] @ coef[svm_ops.coef_row(p, q), sp] + gram[:, sq] @ coef[svm_ops.coef_row(q, p), sq]
                     + clf.intercept_[k])
    want = clf.decision_function(Xt)
    assert np.abs(dec - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    assert (classes[svm_ops.vote(want, K)] == clf.predict(Xt)).all()


def test_vote_breaks_ties_towards_the_first_class():
    from point_dae_amd import svm_ops
    # three classes, each with one vote; a decision value of exactly 0 votes for the pair's second class
    dec = np.array([[1.0, -1.0, 1.0], [0.0, 0.0, 0.0], [-1.0, 1.0, -1.0]])
    assert svm_ops.vote(dec, 3).tolist() == [0, 2, 0]
