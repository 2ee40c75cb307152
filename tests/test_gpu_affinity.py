"""The task-affinity protocol on the GPU: the fused linear probe of csrc/affinity.hip (affinity_ops) against the
reference's loop -- torch.nn.Linear, torch.optim.AdamW, CosineAnnealingLR on the CPU --, its evaluation against fp64,
datasets.ShapeNetClass, and the protocol end to end through main.

Tolerances.  Per setting the reference loop is run once in fp64 and once in fp32 from the same fp32 init and the same
permutations; e_ref is the fp32 run's distance from the fp64 run, taken two ways: the relative L2 of W, and the largest
absolute difference of the logits on 150 test rows evaluated in fp64.  The kernel does the same fp32 arithmetic in another
summation order, so its W, b must lie within FACTOR e_ref of the fp64 run on both measures.  If e_ref (relative L2) is not
below 1e-5 the data is too ill-conditioned to say anything and the test fails instead of passing.  FACTOR = 4, the margin
test_gpu_svm.py takes in the same situation; the ratios measured on the MI355X are in test_trajectory's docstring.

The one-step and step-counter tests compare with the steps written out in fp64 numpy (np_probe, which equals the fp64
torch loop to 1e-17); their tolerances are derived from the fp32 format in their docstrings.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import proc_util  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
M_TEST = 150
LR, WD, T_MAX, B1, B2, EPS = 1e-3, 0.05, 300, 0.9, 0.999, 1e-8
EPS32 = 2.0 ** -23
# n, D, K, epochs, mean scale
SETTINGS = {'n200_d72_k5': (200, 72, 5, 4, 0.25),           # three batches and a dropped tail of 8; D no multiple of a slice
            'n130_d1024_k55': (130, 1024, 55, 2, 0.06),     # the protocol's own widths
            'n64_d768_k40': (64, 768, 40, 3, 0.1),          # exactly one batch per epoch
            'n200_d72_k5_full': (200, 72, 5, 300, 0.25)}    # the whole schedule down to its last learning rate: 900 steps


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gaussian_data(n, D, K, scale, seed, m=M_TEST, epochs=1):
    """Gaussian classes (unit variance) around random means of the given scale, fp32 -> dict of Xtr, ytr, Xte, yte, the fp32
    init (W0, b0) of nn.Linear(D, K) under the seed and one permutation per epoch."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((K, D)) * scale
    ctr, cte = rng.integers(0, K, n), rng.integers(0, K, m)
    Xtr = (means[ctr] + rng.standard_normal((n, D))).astype(np.float32)
    Xte = (means[cte] + rng.standard_normal((m, D))).astype(np.float32)
    torch.manual_seed(seed)
    lin = torch.nn.Linear(D, K)
    perms = np.stack([rng.permutation(n) for _ in range(epochs)], 0) if epochs else np.zeros((0, n), np.int64)
    return dict(Xtr=Xtr, ytr=ctr.astype(np.int64), Xte=Xte, yte=cte.astype(np.int64), W0=lin.weight.detach().numpy().copy(),
                b0=lin.bias.detach().numpy().copy(), perms=perms, K=K, epochs=epochs)


def torch_loop(d, dtype):
    """The reference's loop (tools/runner_finetune.py:1203-1242) on the CPU in `dtype` -> (W, b) as fp64 numpy."""
    X, y = torch.from_numpy(d['Xtr']).to(dtype), torch.from_numpy(d['ytr'])
    net = torch.nn.Linear(X.shape[1], d['K']).to(dtype)
    with torch.no_grad():
        net.weight.copy_(torch.from_numpy(d['W0']))
        net.bias.copy_(torch.from_numpy(d['b0']))
    criterion = torch.nn.CrossEntropyLoss()
    optimizer = torch.optim.AdamW(net.parameters(), lr=LR, weight_decay=WD)
    schedule = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=T_MAX)
    for epoch in range(d['epochs']):
        r = torch.from_numpy(d['perms'][epoch])
        feats, labels = X[r], y[r]
        for i in range(X.shape[0] // 64):
            optimizer.zero_grad()
            loss = criterion(net(feats[i * 64:(i + 1) * 64]), labels[i * 64:(i + 1) * 64])
            loss.backward()
            optimizer.step()
        schedule.step()
    return net.weight.detach().double().numpy(), net.bias.detach().double().numpy()


def distances(d, W, b, W64, b64):
    """(relative L2 of W, max |logit difference| on the test rows in fp64) of (W, b) from the fp64 run."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    Xte = d['Xte'].astype(np.float64)
    return (float(np.linalg.norm(W - W64) / np.linalg.norm(W64)),
            float(np.abs((Xte @ W.T + b) - (Xte @ W64.T + b64)).max()))


_refs = {}


def reference(name):
    """The data of a setting with the fp64 run and e_ref, computed once."""
    if name not in _refs:
        n, D, K, epochs, scale = SETTINGS[name]
        d = gaussian_data(n, D, K, scale, seed=300 + K + epochs, epochs=epochs)
        d['W64'], d['b64'] = torch_loop(d, torch.float64)
        W32, b32 = torch_loop(d, torch.float32)
        d['e_ref'] = distances(d, W32, b32, d['W64'], d['b64'])
        _refs[name] = d
    return _refs[name]


def train(d, **kw):
    from point_dae_amd import affinity_ops
    args = dict(epochs=d['epochs'], init=(d['W0'], d['b0']), perms=d['perms'])
    args.update(kw)
    W, b = affinity_ops.train_linear_probe(_dev(args.pop('X', d['Xtr'])), args.pop('y', d['ytr']), d['K'], **args)
    torch.cuda.synchronize()
    return W, b


def np_probe(d, epochs, restart_t=False):
    """The probe's steps in fp64 numpy, written out: softmax cross-entropy gradient, then AdamW with the decoupled decay
    first and the bias corrections of the global step t (restart_t: t starts again at 1 in every epoch, which is NOT
    what the reference does).  One batch per epoch is all the callers need: rows perms[e][:64]."""
    from point_dae_amd import affinity_ops
    X, y = d['Xtr'].astype(np.float64), d['ytr']
    W, b = d['W0'].astype(np.float64), d['b0'].astype(np.float64)
    mW, vW, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)
    lrs = affinity_ops.cosine_lrs(LR, T_MAX, epochs)
    t = 0
    for e in range(epochs):
        rows = d['perms'][e][:64]
        t = 1 if restart_t else t + 1
        z = X[rows] @ W.T + b
        p = np.exp(z - z.max(1, keepdims=True))
        g = p / p.sum(1, keepdims=True)
        g[np.arange(64), y[rows]] -= 1.0
        g /= 64.0
        grads = (g.T @ X[rows], g.sum(0))
        out = []
        for par, m, v, gr in ((W, mW, vW, grads[0]), (b, mb, vb, grads[1])):
            par = par * (1.0 - lrs[e] * WD)
            m[...] = B1 * m + (1 - B1) * gr
            v[...] = B2 * v + (1 - B2) * gr * gr
            out.append(par - lrs[e] / (1 - B1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - B2 ** t) + EPS))
        W, b = out
    return W, b, grads


# ---- 1. the trajectory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SETTINGS))
def test_trajectory(name):
    """The kernel's W, b against the fp64 reference loop, within FACTOR times the fp32 reference loop's own distance.

    Measured on the MI355X, ratio of the kernel's distance to e_ref (relative L2 of W / test logits):
    n200_d72_k5 0.99 / 1.01, n130_d1024_k55 1.42 / 2.47, n64_d768_k40 1.08 / 1.08, n200_d72_k5_full 1.06 / 1.07.
    The one ratio above 2 (logits, n130_d1024_k55: kernel 1.07e-6 against e_ref 4.31e-7) is the reference's own spread,
    not an excess of the kernel: that setting is four steps at D = 1024, so e_ref is a single draw of the rounding of
    1024-term dot products, and it depends on the order in which the host's BLAS adds them -- the same fp32 reference loop
    gave 1.18e-6 on the logits on another host's CPU (2.7 times the value above, with the same fp64 run), against which
    the kernel's ratio is 0.91.  FACTOR stays at 4."""
    d = reference(name)
    e_w, e_z = d['e_ref']
    print('%s: e_ref relative L2 of W %.3e, logits %.3e' % (name, e_w, e_z))
    assert e_w < 1e-5, 'the fp32 reference loop is %.3e from the fp64 one: the data is too ill-conditioned' % e_w
    W, b = train(d)
    k_w, k_z = distances(d, W.cpu().numpy(), b.cpu().numpy(), d['W64'], d['b64'])
    print('%s: kernel relative L2 of W %.3e (ratio %.2f), logits %.3e (ratio %.2f)' % (name, k_w, k_w / e_w, k_z, k_z / e_z))
    assert k_w <= FACTOR * e_w and k_z <= FACTOR * e_z


# ---- 2. one step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [8, 1024])
def test_one_step_is_the_closed_form(D):
    """n = 64, one epoch, K = 3: against one AdamW step written out in fp64.  The order of decay and update, the bias
    corrections at t = 1 (m / (1 - b1) = g, sqrt(v / (1 - b2)) = |g|: every entry moves by lr g / (|g| + eps) plus the
    decay) and the bias row.

    Tolerance per entry: 2 eps32 max|W0| for the two roundings of the parameter itself (decay, subtraction) + 2e-9 for the
    update term (lr = 1e-3 times ~10 roundings of 6e-8, and its sensitivity lr eps dg / (|g| + eps)^2 to the fp32 error
    dg ~ 2e-7 of a gradient entry, which is below 2e-10 once |g| >= 1e-4).  Entries with a smaller |g| -- the step is
    then steep in g -- are only required to move by at most lr (1 + 1e-3) beside the decay."""
    d = gaussian_data(64, D, 3, 0.5, seed=40 + D)
    W64, b64, (gW, gb) = np_probe(d, 1)
    W, b = train(d, epochs=1)
    W, b = W.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    tol = 2 * EPS32 * max(np.abs(d['W0']).max(), np.abs(d['b0']).max()) + 2e-9
    for got, want, g, p0 in ((W, W64, gW, d['W0']), (b, b64, gb, d['b0'])):
        firm = np.abs(g) >= 1e-4
        assert firm.mean() > 0.9
        print('D=%d: max |kernel - fp64| %.3e on %d firm entries (tolerance %.3e)' % (D, np.abs(got - want)[firm].max(), firm.sum(), tol))
        assert np.abs(got - want)[firm].max() <= tol
        assert (np.abs(got - p0.astype(np.float64) * (1 - LR * WD)) <= LR * (1 + 1e-3) + tol).all()
        # (and the step is there at all: a firm entry moves by lr to 1e-4 relative)
        moved = np.abs(got - p0.astype(np.float64) * (1 - LR * WD))[firm]
        assert np.abs(moved - LR).max() <= 1e-4 * LR + tol


# ---- 3. the step counter runs on across the epochs -----------------------------------------------------------------------
def test_step_counter_continues_across_epochs():
    """Two epochs of one batch each equal the fp64 steps with t = 1, 2 (tolerance: two steps of test_one_step's, the
    second step's m / sqrt(v) being as benign as the first's), and a run that restarts t at every epoch is far away."""
    d = gaussian_data(64, 40, 4, 0.5, seed=77, epochs=2)
    W64, b64, _ = np_probe(d, 2)
    Wr, br, _ = np_probe(d, 2, restart_t=True)
    W, b = train(d)
    W, b = W.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    tol = 2 * (2 * EPS32 * max(np.abs(d['W0']).max(), np.abs(d['b0']).max()) + 2e-9)
    err = max(np.abs(W - W64).max(), np.abs(b - b64).max())
    apart = max(np.abs(Wr - W64).max(), np.abs(br - b64).max())
    print('continuing t: max |kernel - fp64| %.3e (tolerance %.3e); restarted t lies %.3e away' % (err, tol, apart))
    assert apart > 100 * tol
    assert err <= tol


# ---- 4. - 6. permutations, determinism, nothing to train -----------------------------------------------------------------
def test_rows_are_gathered_through_the_permutation():
    """An explicit permutation (the same in both epochs) against X physically shuffled with identity permutations."""
    d = gaussian_data(200, 72, 5, 0.25, seed=5, epochs=2)
    p = d['perms'][0]
    assert not np.array_equal(p, np.arange(200))
    W_a, b_a = train(d, perms=np.stack([p, p]))
    W_b, b_b = train(d, X=d['Xtr'][p], y=d['ytr'][p], perms=np.stack([np.arange(200)] * 2))
    assert torch.equal(W_a, W_b) and torch.equal(b_a, b_b)
    W_c, _ = train(d, perms=np.stack([np.arange(200)] * 2))
    assert not torch.equal(W_a, W_c)


def test_same_call_twice_gives_the_same_bits():
    d = reference('n130_d1024_k55')
    W_a, b_a = train(d)
    W_b, b_b = train(d)
    assert torch.equal(W_a, W_b) and torch.equal(b_a, b_b)
    assert not torch.equal(W_a.cpu(), torch.from_numpy(d['W0']))


def test_nothing_to_train(monkeypatch):
    from point_dae_amd import _lib
    d = gaussian_data(63, 72, 5, 0.25, seed=6, epochs=3)
    seen = []
    monkeypatch.setattr(_lib, 'CALL_HOOK', lambda name, args: seen.append(name))
    W, b = train(d)
    assert torch.equal(W.cpu(), torch.from_numpy(d['W0'])) and torch.equal(b.cpu(), torch.from_numpy(d['b0']))
    d2 = gaussian_data(128, 72, 5, 0.25, seed=6, epochs=0)
    W, b = train(d2, perms=None)
    assert torch.equal(W.cpu(), torch.from_numpy(d2['W0'])) and torch.equal(b.cpu(), torch.from_numpy(d2['b0']))
    assert seen == []


# ---- 7. evaluation ----------------------------------------------------------------------------------------------------------
def test_eval_against_fp64():
    """m = 150 (two full batches of the reference's 64 and a short one), K = 55, D = 1024: the mean cross-entropy to 1e-6
    relative, the correct count on the rows whose two largest fp64 logits are more than 1e-5 apart (the others, at most
    2 % of the rows, may go either way)."""
    from point_dae_amd import affinity_ops
    d = gaussian_data(64, 1024, 55, 0.06, seed=9)
    rng = np.random.default_rng(9)
    W = (d['W0'] + 0.05 * rng.standard_normal(d['W0'].shape)).astype(np.float32)     # (a probe that separates the classes a bit)
    b = d['b0']
    z = d['Xte'].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    lse = z.max(1) + np.log(np.exp(z - z.max(1, keepdims=True)).sum(1))
    want_loss = float((lse - z[np.arange(M_TEST), d['yte']]).mean())
    top2 = np.sort(z, 1)[:, -2:]
    close = (top2[:, 1] - top2[:, 0]) <= 1e-5
    assert close.sum() <= 0.02 * M_TEST
    sure = int(((z.argmax(1) == d['yte']) & ~close).sum())
    acc, loss, logits = affinity_ops.evaluate(_dev(W), _dev(b), _dev(d['Xte']), d['yte'], return_logits=True)
    print('eval: loss %.9f, fp64 %.9f (relative %.3e); correct %d, fp64 %d on the %d rows with a clear winner' % (
        loss, want_loss, abs(loss - want_loss) / want_loss, round(acc * M_TEST), sure, M_TEST - close.sum()))
    assert abs(loss - want_loss) <= 1e-6 * want_loss
    assert sure <= round(acc * M_TEST) <= sure + int(close.sum())
    assert 0 < sure < M_TEST                             # (the count says something: neither nothing nor everything is right)
    assert np.abs(logits.cpu().numpy() - z).max() <= 1e-4
    assert affinity_ops.evaluate(_dev(W), _dev(b), _dev(d['Xte']), d['yte']) == (acc, loss)


def test_eval_tie_goes_to_the_lower_class():
    from point_dae_amd import affinity_ops
    rng = np.random.default_rng(1)
    K, D, m = 6, 16, 9
    W = (0.1 * rng.standard_normal((K, D))).astype(np.float32)
    W[4] = W[2] = rng.standard_normal(D).astype(np.float32)
    b = np.zeros(K, np.float32)
    X = (3.0 * W[2] + 0.1 * rng.standard_normal((m, D))).astype(np.float32)
    acc_lo, loss_lo, logits = affinity_ops.evaluate(_dev(W), _dev(b), _dev(X), np.full(m, 2), return_logits=True)
    z = logits.cpu().numpy()
    assert np.array_equal(z[:, 2], z[:, 4]) and (z[:, 2] > np.delete(z, [2, 4], 1).max(1)).all()
    acc_hi, loss_hi = affinity_ops.evaluate(_dev(W), _dev(b), _dev(X), np.full(m, 4))
    assert acc_lo == 1.0 and acc_hi == 0.0 and loss_lo == loss_hi


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch):
    from point_dae_amd import _lib, affinity_ops
    X = _dev(np.zeros((128, 8), np.float32))
    seen = []
    monkeypatch.setattr(_lib, 'CALL_HOOK', lambda name, args: seen.append(name))
    with pytest.raises(RuntimeError, match='status -1.*greater than one'):
        affinity_ops.train_linear_probe(X, np.zeros(128, np.int64), 1)
    with pytest.raises(RuntimeError, match='status -3.*64'):
        affinity_ops.train_linear_probe(X, np.arange(128) % 65, 65)
    with pytest.raises(ValueError, match='train label outside 0 .. 4'):
        affinity_ops.train_linear_probe(X, np.where(np.arange(128) == 100, 5, 0), 5)
    W, b = _dev(np.zeros((5, 8), np.float32)), _dev(np.zeros(5, np.float32))
    with pytest.raises(ValueError, match='test label outside 0 .. 4'):
        affinity_ops.evaluate(W, b, X, np.where(np.arange(128) == 100, 5, 0))
    with pytest.raises(RuntimeError, match='status -3'):
        affinity_ops.evaluate(_dev(np.zeros((65, 8), np.float32)), _dev(np.zeros(65, np.float32)), X, np.zeros(128, np.int64))
    assert seen == []
    # the C entries refuse the same by themselves (a negative status, nothing launched)
    handle = _lib.lib()
    for bad in ((128, 8, 8, 1), (128, 0, 8, 5), (128, 8, 7, 5), (-1, 8, 8, 5)):
        assert handle.pdae_linear_probe_supported(*bad) == -1, bad
    assert handle.pdae_linear_probe_supported(128, 8, 8, 65) == -3
    assert handle.pdae_linear_probe_supported(0, 8, 8, 64) == 0


# ---- 9. the labelled loader -------------------------------------------------------------------------------------------------
def _listed_set(tmp_path):
    pc, lists = tmp_path / 'pc', tmp_path / 'lists'
    pc.mkdir()
    lists.mkdir()
    rng = np.random.default_rng(0)
    names = ['04379243-a.npy', '02691156-b.npy', '04379243-c.npy', '03001627-d.npy', '02691156-e.npy', '03001627-f.npy']
    for i, name in enumerate(names):
        np.save(str(pc / name), (rng.standard_normal((1100, 6)) * (1 + i)).astype(np.float32))    # xyz + normals
    (lists / 'train.txt').write_text('\n'.join(names) + '\n')
    (lists / 'test.txt').write_text('\n'.join(names[1:]) + '\n')
    return dict(PC_PATH=str(pc), DATA_PATH=str(lists), N_POINTS=1024, npoints=1024, bs=4, aug_type=['norm'],
                corrupt_type=['clean'], device='cuda', seed=0)


def test_shapenet_class_loader(tmp_path):
    from point_dae_amd import datasets
    cfg = _listed_set(tmp_path)
    want = {'02691156': 0, '03001627': 1, '04379243': 2}
    train = list(datasets.ShapeNetClass(dict(cfg, subset='train')))
    assert len(train) == 1                                # 6 clouds in batches of 4: the short batch is dropped
    tax, model_id, (points, labels) = train[0]
    assert (tax, model_id) == ('04379243', 'a') and points.shape == (4, 1024, 3) and points.is_cuda
    assert labels.tolist() == [2, 0, 2, 1] and labels.dtype == torch.int64
    assert torch.isfinite(points).all() and float(points.norm(dim=2).max()) <= 1.0 + 1e-5      # 'norm': the unit sphere
    test = list(datasets.ShapeNetClass(dict(cfg, subset='test')))
    assert [tuple(t[2][0].shape) for t in test] == [(4, 1024, 3), (1, 1024, 3)]                 # 5 clouds: the short batch stays
    assert torch.cat([t[2][1] for t in test]).tolist() == [want[n] for n in ('02691156', '04379243', '03001627', '02691156', '03001627')]
    moved = list(datasets.ShapeNetClass(dict(cfg, subset='test', corrupt_type=['affine_r3'])))
    assert moved[0][2][0].shape == (4, 1024, 3) and torch.isfinite(moved[0][2][0]).all()
    with pytest.raises(NotImplementedError, match='forward'):
        datasets.ShapeNetClass(dict(cfg, subset='train', corrupt_type=['dropout_global']))
    # without files: labelled synthetic clouds, `count` of them
    syn = datasets.ShapeNetClass(dict(N_POINTS=1024, npoints=1024, bs=8, count=20, classes=3, subset='train', device='cuda'))
    batches = list(syn)
    assert len(syn) == 2 == len(batches) and batches[0][2][0].shape == (8, 1024, 3)
    assert set(torch.cat([t[2][1] for t in batches]).tolist()) <= {0, 1, 2}


# ---- 10. end to end ---------------------------------------------------------------------------------------------------------
def _run_main(tmp_path, env=None):
    cmd = [sys.executable, '-m', 'point_dae_amd.main', '--config', 'cfgs/finetune_shapenet_task_affinity_dgcnn.yaml',
           '--scratch_model', '--task_affinity', '--total_bs', '64', '--steps_per_epoch', '2', '--exp_name', 'ci',
           '--root_folder', os.path.relpath(str(tmp_path / 'exp'), ROOT)]
    return proc_util.run(cmd, 300, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


def _protocol_line(out):
    lines = re.findall(r'^\[Validation\] Acc: \d\.\d{4}  loss = \d+\.\d{4}$', out, flags=re.M)
    assert len(lines) == 1, out[-2000:]
    acc, loss = re.match(r'\[Validation\] Acc: (\S+)  loss = (\S+)', lines[0]).groups()
    return float(acc), float(loss)


def test_protocol_end_to_end(tmp_path):
    """main --task_affinity from scratch on the synthetic set: 2 train batches of 64 (so 2 steps per epoch, 600 in all), the
    256 test clouds.  With PDAE_AFFINITY=torch and the same seed the printed loss agrees to 1e-4 absolute (the simple one
    of the two bounds the protocol's issue offers; the line prints four decimals, so one unit of the last place is let
    through on top)."""
    r = _run_main(tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Training from scratch' in r.stdout and 'Affinity backend: hip' in r.stdout
    assert '(128, 1024)' in r.stdout and '(256, 1024)' in r.stdout
    acc, loss = _protocol_line(r.stdout)
    assert 0.0 <= acc <= 1.0 and loss > 0.0
    r2 = _run_main(tmp_path, env={'PDAE_AFFINITY': 'torch'})
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert 'Affinity backend: torch' in r2.stdout
    acc2, loss2 = _protocol_line(r2.stdout)
    print('hip: acc %.4f loss %.4f; torch: acc %.4f loss %.4f' % (acc, loss, acc2, loss2))
    assert abs(loss - loss2) <= 1e-4 + 1.0001e-4
