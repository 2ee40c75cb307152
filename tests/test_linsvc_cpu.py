"""CPU side of the device LinearSVC (point_dae_amd/linsvc_ops.py): the backend switch, the label layout, the objective the
kernels minimise (pinned against sklearn's own optimum) and the stopping rule."""
import numpy as np
import pytest
import torch

import linsvc_cases as cases


def test_backend_switch(monkeypatch):
    from point_dae_amd import linsvc_ops
    monkeypatch.delenv('PDAE_LINSVC', raising=False)
    assert linsvc_ops.backend() == 'sklearn'             # tests/test_gpu_probe.py pins validate() to the host fit to 1e-12
    monkeypatch.setenv('PDAE_LINSVC', 'hip')
    assert linsvc_ops.backend() == 'hip'
    monkeypatch.setenv('PDAE_LINSVC', 'sklearn')
    assert linsvc_ops.backend() == 'sklearn'
    monkeypatch.setenv('PDAE_LINSVC', 'liblinear')
    with pytest.raises(ValueError, match='PDAE_LINSVC'):
        linsvc_ops.backend()


def test_label_layout_is_np_unique():
    from point_dae_amd import linsvc_ops
    labels = np.array([7, -2, 7, 30, -2, 11, 30, 30])
    classes, index = linsvc_ops.label_layout(labels)
    assert classes.tolist() == [-2, 7, 11, 30] and np.array_equal(classes, np.unique(labels))
    assert index.dtype == np.int32 and np.array_equal(classes[index], labels)
    Y = linsvc_ops.targets(index, len(classes))
    assert Y.shape == (8, 4) and set(np.unique(Y)) == {-1.0, 1.0}
    for k, c in enumerate(classes):
        assert np.array_equal(Y[:, k] > 0, labels == c)
    # as sklearn orders its machines
    from sklearn.svm import LinearSVC
    x = np.random.default_rng(0).standard_normal((8, 3))
    assert np.array_equal(LinearSVC().fit(x, labels).classes_, classes)
    # two classes: one machine, the second class positive (sklearn's coef_ has one row)
    classes2, index2 = linsvc_ops.label_layout(labels[:5] == 7)
    assert linsvc_ops.columns(2) == (1, 1) and linsvc_ops.columns(3) == (3, 0)
    Y2 = linsvc_ops.targets(index2, 2)
    assert Y2.shape == (5, 1) and np.array_equal(Y2[:, 0] > 0, labels[:5] == 7)
    assert LinearSVC().fit(x[:5], labels[:5] == 7).coef_.shape == (1, 3)


@pytest.mark.parametrize('name', ['small', 'd_gt_n'])
def test_objective_is_the_one_sklearn_minimises(name):
    """Intercept regularised, C multiplies the sum, squared hinge: at sklearn's [coef_, intercept_] the fp64 gradient of
    that objective vanishes to what sklearn's own tol = 1e-10 leaves (bound 1e-6 |g(0)|, loose)."""
    from point_dae_amd import linsvc_ops
    xtr, ytr, _, _ = cases.features(name)
    classes, index = linsvc_ops.label_layout(ytr)
    Y = linsvc_ops.targets(index, len(classes))
    W = cases.w_ref(name)
    _, g = cases.objective(W, xtr, Y)
    _, g0 = cases.objective(np.zeros_like(W), xtr, Y)
    ratio = np.sqrt((g * g).sum(0)) / np.sqrt((g0 * g0).sum(0))
    print(name, 'max |g| / |g(0)| at the sklearn optimum', ratio.max())
    assert ratio.max() <= 1e-6
    if name != 'small':
        return
    # and with the intercept left out of the regulariser it is a different function: that gradient does not vanish there
    # (where the intercepts are not small: |b| ~ 0.4 on this shape)
    g_free = g.copy()
    g_free[-1] -= W[-1]
    assert (np.sqrt((g_free * g_free).sum(0)) / np.sqrt((g0 * g0).sum(0))).max() > 1e-5


def test_stored_optimum_of_the_wide_shape():
    """tests/golden/linsvc_ref_d.npz is the optimum of the features the generator gives today."""
    from point_dae_amd import linsvc_ops
    xtr, ytr, _, _ = cases.features('wide')
    classes, index = linsvc_ops.label_layout(ytr)
    Y = linsvc_ops.targets(index, len(classes))
    W = cases.w_ref('wide')
    assert W.shape == (385, 40)
    _, g = cases.objective(W, xtr, Y)
    _, g0 = cases.objective(np.zeros_like(W), xtr, Y)
    assert (np.sqrt((g * g).sum(0)) / np.sqrt((g0 * g0).sum(0))).max() <= 1e-6


def test_stopping_rule_is_liblinears():
    from point_dae_amd import linsvc_ops
    _, index = linsvc_ops.label_layout([0] * 2 + [1] * 10 + [2] * 28)
    eps = linsvc_ops.stopping_eps(index, 3, tol=1e-4)
    assert np.allclose(eps, 1e-4 * np.array([2, 10, 12]) / 40.0, rtol=1e-15)
    assert np.allclose(linsvc_ops.stopping_eps(index, 3, tol=1e-8), 1e-4 * eps, rtol=1e-12)
    _, index2 = linsvc_ops.label_layout([5] * 3 + [9] * 7)
    assert np.allclose(linsvc_ops.stopping_eps(index2, 2), [1e-4 * 3 / 10.0], rtol=1e-15)


@pytest.mark.parametrize('name', sorted(cases.SHAPES))
def test_reference_fit_keeps_the_excluded_share(name):
    """The condition of the GPU tests' prediction check: LinearSVC()'s own fit leaves at most 2 % of the test rows with
    their two best decision values closer than delta."""
    _, excluded = cases.default_fit(name)
    print(name, 'excluded share', excluded.mean())
    assert excluded.mean() <= cases.EXCLUDED_CAP


def test_fit_predict_needs_the_gpu():
    from point_dae_amd import linsvc_ops
    x = torch.rand(12, 5)
    with pytest.raises(RuntimeError, match='GPU'):
        linsvc_ops.fit_predict(x, np.arange(12) % 3, x)


def test_supported_refuses_before_any_launch():
    from point_dae_amd import _lib
    handle = _lib.lib()
    assert handle.pdae_linsvc_supported(100, 10, 8, 40) == 0
    for args, word in (((100, 10, 8, 1), 'greater than one'), ((100, 10, 8, 65), 'PDAE_LINSVC_MAX_CLASSES'),
                       ((0, 10, 8, 3), 'empty'), ((100, 0, 8, 3), 'empty'), ((100, 10, 0, 3), 'empty')):
        assert handle.pdae_linsvc_supported(*args) == -3
        assert word in handle.pdae_last_error().decode()
