"""The linear-SVM evaluation protocol on the GPU: the one-vs-one solver and predictor of csrc/svm.hip (svm_ops) against
sklearn's SVC on the host -- what the reference calls --, DGCNN_feat against the auto-encoder's feature path, and the
protocol end to end through main.

Tolerances.  Per case (setting, C) the test itself measures what libsvm's stopping tolerance leaves open:
e_ref = max |SVC(tol=1e-3).decision_function - SVC(tol=1e-7).decision_function| over the test rows and pairs.  The
kernels stop at the same violation (eps = 1e-3) on another working-set sequence and on an fp32 Gram matrix, and must stay
within 4 e_ref of the tight solution (an fp64 first-order SMO on the CPU measured at most 1.25 e_ref on these inputs; the
factor 4 is the margin over that for the sequence and the Gram's precision; on the MI355X the largest ratio seen is 1.28).  A predicted label may differ from tight
sklearn's only on a row that has a pairwise tight decision value within 4 e_ref of zero, and on at most 5 % of the rows.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import proc_util  # noqa: E402

pytestmark = pytest.mark.gpu

CS = (0.001, 0.01, 0.1, 1, 10, 100)
FACTOR = 4.0
# K, D, train size of class 0 (class k has 3 k more), mean scale
SETTINGS = {'k5_d64': (5, 64, 40, 0.25), 'k7_d256': (7, 256, 37, 0.12), 'k4_d1024': (4, 1024, 61, 0.06)}
M_TEST = 150


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gaussian_classes(sizes, D, scale, seed, m=M_TEST, ids=None):
    """Gaussian classes (unit variance) around random means of the given scale, fp32, the samples shuffled.
    -> Xtr, ytr, Xte, yte; class k carries the label ids[k] (default 3 k + 1: ids with gaps)."""
    rng = np.random.default_rng(seed)
    K = len(sizes)
    ids = np.arange(K) * 3 + 1 if ids is None else np.asarray(ids)
    means = rng.standard_normal((K, D)) * scale
    ctr = rng.permutation(np.repeat(np.arange(K), sizes))
    cte = rng.integers(0, K, m)
    Xtr = (means[ctr] + rng.standard_normal((len(ctr), D))).astype(np.float32)
    Xte = (means[cte] + rng.standard_normal((m, D))).astype(np.float32)
    return Xtr, ids[ctr], Xte, ids[cte]


def sklearn_dec(Xtr, ytr, Xte, C, tol):
    """-> (decision values (m, P) with dec > 0 voting for the pair's FIRST class, predictions) of the reference's call."""
    from sklearn.svm import SVC
    clf = SVC(C=C, kernel='linear', tol=tol, decision_function_shape='ovo').fit(Xtr.astype(np.float64), ytr)
    dec = clf.decision_function(Xte.astype(np.float64))
    if dec.ndim == 1:                   # two classes: sklearn flips the sign (positive = classes_[1]) and drops the axis
        dec = -dec[:, None]
    return dec, clf.predict(Xte.astype(np.float64))


class Reference:
    """The sklearn side of one data set, computed once: per C the tight decision values / predictions and e_ref."""

    def __init__(self, data, Cs=CS):
        self.data, self.Cs = data, Cs
        Xtr, ytr, Xte, _ = data
        self.tight, self.pred, self.e_ref = [], [], []
        for C in Cs:
            loose, _ = sklearn_dec(Xtr, ytr, Xte, C, 1e-3)
            tight, pred = sklearn_dec(Xtr, ytr, Xte, C, 1e-7)
            self.tight.append(tight)
            self.pred.append(pred)
            self.e_ref.append(float(np.abs(loose - tight).max()))


_refs = {}


def reference(name):
    if name not in _refs:
        if name in SETTINGS:
            K, D, base, scale = SETTINGS[name]
            _refs[name] = Reference(gaussian_classes([base + 3 * k for k in range(K)], D, scale, seed=100 + K))
        elif name == 'big_pair':        # more members than the workgroup has threads (and than 1024): 700 + 650
            _refs[name] = Reference(gaussian_classes([700, 650], 64, 0.25, seed=11, ids=[5, 2]), Cs=(0.001, 0.01, 0.1, 1))
        elif name == 'single_sample':   # a class of one sample: its two pairs have a lone member on one side
            _refs[name] = Reference(gaussian_classes([30, 1, 45], 32, 0.4, seed=12))
    return _refs[name]


def solve(ref, **kw):
    from point_dae_amd import svm_ops
    Xtr, ytr, Xte, _ = ref.data
    pred, dec, status = svm_ops.fit_predict_ovo(_dev(Xtr), ytr, _dev(Xte), ref.Cs, **kw)
    torch.cuda.synchronize()
    return pred, dec.cpu().numpy(), status


def check_against_sklearn(name):
    """The decision-value and prediction checks of the module docstring for every C of a data set -> the largest ratio
    |dec - tight| / e_ref seen."""
    from point_dae_amd import svm_ops
    ref = reference(name)
    pred, dec, status = solve(ref)
    classes = status['classes']
    K = len(classes)
    assert dec.shape == (len(ref.Cs), M_TEST, K * (K - 1) // 2) and pred.shape == (len(ref.Cs), M_TEST)
    assert not status['capped'].any() and (status['gap'] < 1e-3).all()
    worst, failures = 0.0, []
    for i, C in enumerate(ref.Cs):
        err = float(np.abs(dec[i] - ref.tight[i]).max())
        bound = FACTOR * ref.e_ref[i]
        ratio = err / ref.e_ref[i]
        worst = max(worst, ratio)
        print('%s C=%g: e_ref %.3e, |dec - tight| %.3e (ratio %.2f), iterations max %d median %d' % (
            name, C, ref.e_ref[i], err, ratio, status['iters'][i].max(), np.median(status['iters'][i])))
        if not err <= bound:
            failures.append('C=%g: |dec - tight| %.3e > %g e_ref = %.3e' % (C, err, FACTOR, bound))
        # the vote and its tie rule, exactly, on the kernels' own decision values
        assert (pred[i] == classes[svm_ops.vote(dec[i], K)]).all(), 'C=%g: pred is not the vote of dec' % C
        differ = np.nonzero(pred[i] != ref.pred[i])[0]
        print('%s C=%g: %d of %d predictions differ from tight sklearn' % (name, C, len(differ), M_TEST))
        for r in differ:
            if not np.abs(ref.tight[i][r]).min() <= bound:
                failures.append('C=%g: row %d differs without a decision value within %.3e of zero' % (C, r, bound))
        if len(differ) > 0.05 * M_TEST:
            failures.append('C=%g: %d of %d rows differ (more than 5 %%)' % (C, len(differ), M_TEST))
    assert not failures, failures
    return worst


@pytest.mark.parametrize('name', list(SETTINGS))
def test_decisions_and_predictions_match_sklearn(name):
    check_against_sklearn(name)


def test_pair_larger_than_the_workgroup():
    check_against_sklearn('big_pair')


def test_class_with_a_single_sample():
    check_against_sklearn('single_sample')


def test_same_call_twice_gives_the_same_bits():
    ref = reference('k5_d64')
    _, dec_a, st_a = solve(ref)
    coef_a, rho_a = st_a['coef'].clone(), st_a['rho'].clone()
    _, dec_b, st_b = solve(ref)
    assert torch.equal(coef_a, st_b['coef']) and torch.equal(rho_a, st_b['rho'])
    assert np.array_equal(dec_a, dec_b) and np.array_equal(st_a['iters'], st_b['iters'])
    # (the dual constraints the coefficients must satisfy: 0 <= |coef| <= C, y^T alpha = 0 per pair up to rounding)
    for i, C in enumerate(ref.Cs):
        c = coef_a[i].cpu().numpy()
        assert np.abs(c).max() <= C


def test_pair_above_the_member_cap_is_refused_before_any_launch(monkeypatch):
    from point_dae_amd import _lib, svm_ops
    rng = np.random.default_rng(0)
    X = rng.standard_normal((2049 + 8, 8)).astype(np.float32)
    y = np.repeat([0, 1, 2], [1025, 1024, 8])
    seen = []
    Xd, Xt = _dev(X), _dev(X[:4])
    monkeypatch.setattr(_lib, 'CALL_HOOK', lambda name, args: seen.append(name))
    with pytest.raises(RuntimeError, match='status -3.*2048'):
        svm_ops.fit_predict_ovo(Xd, y, Xt, CS)
    assert seen == []
    for bad in (dict(max_iter=0), dict(Cs=CS + (1e3, 1e4, 1e5))):          # neither runs: a negative status each
        kw = dict(Cs=CS, max_iter=100)
        kw.update(bad)
        with pytest.raises(RuntimeError, match='status -1'):
            svm_ops.fit_predict_ovo(Xd[:64], y[1000:1064], Xt, kw['Cs'], max_iter=kw['max_iter'])
    assert seen == []


def test_iteration_cap_raises_and_names_the_pair():
    from point_dae_amd import svm_ops
    Xtr, ytr, Xte, _ = reference('k5_d64').data
    with pytest.raises(RuntimeError, match=r'max_iter = 1 on the class pair \(1, 4\) at C = 0.001'):
        svm_ops.fit_predict_ovo(_dev(Xtr), ytr, _dev(Xte), CS, max_iter=1)


# ---- the model ------------------------------------------------------------------------------------------------------------
def _models():
    from point_dae_amd.builder import model_builder
    from point_dae_amd.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'pretrain_PointCAE_clean.yaml')).model
    cfg.NAME = 'Point_CAE_DGCNN_FCOnly'
    torch.manual_seed(5)
    pre = model_builder(cfg).cuda()
    feat = model_builder(cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'finetune_modelnet_svm_dgcnn.yaml')).model)
    inc = feat.load_state_dict(pre.state_dict(), strict=False)
    assert not inc.missing_keys and all(k.startswith('recfc.') for k in inc.unexpected_keys)
    return pre.eval(), feat.cuda().eval()


def test_dgcnn_feat_is_the_autoencoders_feature_path():
    from conftest import make_clouds
    pre, feat = _models()
    # running estimates away from their initial (0, 1), so that eval mode is told apart from batch statistics
    with torch.no_grad():
        for mod in feat.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    pre.load_state_dict(feat.state_dict(), strict=False)
    pts = _dev(make_clouds(3, 2, 256, 'shapes'))
    before = {k: v.clone() for k, v in feat.state_dict().items()}
    with torch.no_grad():
        want = pre(pts, pts, return_feat=True)
        got = feat(pts)
        again = feat(pts)
    assert got.shape == (2, 1024) and torch.equal(got, want) and torch.equal(again, got)
    for k, v in feat.state_dict().items():
        assert torch.equal(v, before[k]), k


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _run_main(tmp_path, env=None):
    cmd = [sys.executable, '-m', 'point_dae_amd.main', '--config', 'cfgs/finetune_modelnet_svm_dgcnn.yaml', '--scratch_model',
           '--svm_classification', '--total_bs', '16', '--steps_per_epoch', '3', '--exp_name', 'ci', '--root_folder',
           os.path.relpath(str(tmp_path / 'exp'), ROOT)]
    return proc_util.run(cmd, 300, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


def _protocol_lines(out):
    """-> ([(c, max_acc)] of the six 'c max_acc' lines, the accuracy of the final line)."""
    rows = []
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 2 and parts[0] in ('0.001', '0.01', '0.1', '1', '10', '100'):
            rows.append((parts[0], float(parts[1])))
    final = [line for line in out.splitlines() if line.startswith('[Validation] EPOCH: ')]
    assert len(final) == 1, out[-2000:]
    assert final[0].startswith('[Validation] EPOCH: 100  acc = ')
    return rows, float(final[0].split('acc = ')[1])


def test_protocol_end_to_end(tmp_path, monkeypatch, capsys):
    """main --svm_classification from scratch on the synthetic ModelNet: 3 train batches of 16, the 256 test clouds; the
    accuracy equals svm_ops' on the same seeded features computed here; PDAE_SVM=sklearn prints the same lines."""
    from point_dae_amd import main as pmain
    from point_dae_amd import svm_ops
    r = _run_main(tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Training from scratch' in r.stdout and 'SVM backend: hip' in r.stdout
    assert '(48, 1024)' in r.stdout and '(256, 1024)' in r.stdout
    rows, final = _protocol_lines(r.stdout)
    assert [c for c, _ in rows] == ['0.001', '0.01', '0.1', '1', '10', '100']
    accs = [a for _, a in rows]
    assert all(b >= a for a, b in zip(accs, accs[1:])) and 0.0 <= accs[-1] <= 1.0
    assert abs(final - accs[-1]) < 5e-5

    # the same command in this process (main seeds every generator from --seed, so the features are the child's), with the
    # features it hands to the classifier kept
    seen = {}
    orig = svm_ops.accuracies

    def capture(tr_f, tr_l, te_f, te_l, Cs=svm_ops.SVM_CS):
        seen.update(tr_f=tr_f, tr_l=tr_l, te_f=te_f, te_l=te_l)
        return orig(tr_f, tr_l, te_f, te_l, Cs)
    monkeypatch.setattr(svm_ops, 'accuracies', capture)
    monkeypatch.chdir(ROOT)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.delenv('PDAE_SVM', raising=False)
    capsys.readouterr()
    pmain.main(['--config', 'cfgs/finetune_modelnet_svm_dgcnn.yaml', '--scratch_model', '--svm_classification', '--total_bs',
                '16', '--steps_per_epoch', '3', '--exp_name', 'ci2', '--root_folder', os.path.relpath(str(tmp_path / 'exp'), ROOT)])
    rows_here, final_here = _protocol_lines(capsys.readouterr().out)
    assert rows_here == rows and final_here == final
    assert tuple(seen['tr_f'].shape) == (48, 1024) and seen['tr_f'].is_cuda and tuple(seen['te_f'].shape) == (256, 1024)
    pred, _, _ = svm_ops.fit_predict_ovo(seen['tr_f'], seen['tr_l'], seen['te_f'], svm_ops.SVM_CS)
    te_l = seen['te_l'].cpu().numpy()
    best = max(float(np.mean(p == te_l)) for p in pred)
    assert accs[-1] == best and abs(final - best) < 5e-5

    r2 = _run_main(tmp_path, env={'PDAE_SVM': 'sklearn'})
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert 'SVM backend: sklearn' in r2.stdout
    rows2, final2 = _protocol_lines(r2.stdout)
    assert [c for c, _ in rows2] == [c for c, _ in rows] and 0.0 <= final2 <= 1.0
