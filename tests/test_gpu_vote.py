"""The voted evaluation on the GPU: csrc/vote.hip's two kernels (pdae_vote_resample bit for bit against pdae_resample_affine
per vote; pdae_vote_reduce against fp64 and its host twin), the two backends of vote_ops against each other on both
classifiers, the FPS cache, and main --test end to end.

gap_tol.  The hip backend runs the V B clouds of a batch as one forward, the torch backend as V forwards of B clouds; a
cloud's logits may depend on the batch it runs in (the row GEMMs plan their split by the row count).  FORWARD_DIFF is that
dependence MEASURED on the code before this feature: the largest |base_model(cat of the V point sets) - the V separate
base_model(points_k)| over the batches of this module's loader (count 5, bs 2, P 1300, npoints 1024, V 3, seed SEED) on
an MI355X, per model.  Two clouds' predictions are compared only when the torch backend's top-2 gap exceeds
gap_tol = 2 FORWARD_DIFF + the reduce bound (v + 1) 2^-24 max|logits|; the seed is such that every cloud does.
Measured (seeds 0 - 3): FORWARD_DIFF = 0.0 for both models, so gap_tol is the reduce bound alone: 2.3e-9 (DGCNN,
max|logits| 9.6e-3) and 3.5e-8 (PointTransformer, 0.145) against smallest top-2 gaps of 4.0e-4 and 2.6e-4 at seed 0; the
two backends' mean logits differed by 4.7e-10 and 7.5e-9.
"""
import contextlib
import os
import types

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {'DGCNN': os.path.join(ROOT, 'cfgs', 'finetune_modelnet_dgcnn_smooth.yaml'),
        'PointTransformer': os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features.yaml')}
U = 2.0 ** -24
SEED, TIMES = 0, 3
# measured on the parent commit's code (see the module docstring); 0.0: one forward of the cat equals the separate
# forwards bit for bit, and the comparison of the two backends' predictions is exact up to the reduce bound
FORWARD_DIFF = {'DGCNN': 0.0, 'PointTransformer': 0.0}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- pdae_vote_resample ------------------------------------------------------------------------------------------------

SIZES = {'one_block': dict(V=3, B=3, P=70, point_all=40, npoints=33),
         'two_chunks_and_tail': dict(V=3, B=3, P=400, point_all=320, npoints=300)}


def _case(V, B, P, point_all, npoints, C, seed):
    """raw (B,P,C) with one cloud of O(100) coordinates; fps_idx (B,point_all) distinct rows per cloud; choice (V,npoints)
    distinct FPS columns per vote; the first chosen point of vote 0 of every cloud is (-0, 0, -0); A (V,B,3,3), t (V,B,3)."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand(B, P, C, generator=g) * 2 - 1
    raw[1] *= 100.0
    fps_idx = torch.stack([torch.randperm(P, generator=g)[:point_all] for _ in range(B)]).to(torch.int32)
    choice = torch.stack([torch.randperm(point_all, generator=g)[:npoints] for _ in range(V)]).to(torch.int32)
    for b in range(B):
        row = int(fps_idx[b, int(choice[0, 0])])
        raw[b, row, 0], raw[b, row, 1], raw[b, row, 2] = -0.0, 0.0, -0.0
    A, t = torch.randn(V, B, 3, 3, generator=g), torch.randn(V, B, 3, generator=g)
    return raw.cuda(), fps_idx.cuda(), choice.cuda(), A.cuda(), t.cuda()


def _per_vote(raw, fps_idx, choice, A, t):
    from point_dae_amd.data_transforms import resample_affine
    return torch.stack([resample_affine(raw, fps_idx, choice[k].contiguous(), None if A is None else A[k].contiguous(),
                                        None if t is None else t[k].contiguous()) for k in range(choice.shape[0])])


@pytest.mark.parametrize('C', [3, 6])
@pytest.mark.parametrize('use', ['A+t', 'A', 'none'])
@pytest.mark.parametrize('size', sorted(SIZES))
def test_vote_resample_equals_resample_affine_per_vote_bit_for_bit(size, use, C):
    from point_dae_amd import vote_ops
    raw, fps_idx, choice, A, t = _case(C=C, seed=3 + C, **SIZES[size])
    A, t = (A if 'A' in use else None), (t if 't' in use else None)
    got = vote_ops.vote_resample(raw, fps_idx, choice, A, t)
    s = SIZES[size]
    assert tuple(got.shape) == (s['V'], s['B'], s['npoints'], 3)
    assert torch.equal(_bits(got), _bits(_per_vote(raw, fps_idx, choice, A, t)))
    if use == 'none':                                       # moved, not computed on: the signed zeros survive
        want = raw[torch.arange(s['B'])[:, None], fps_idx.long()[:, choice[0].long()], :3]
        assert torch.equal(_bits(got[0]), _bits(want))
        assert torch.equal(_bits(got[0, :, 0]), _bits(torch.tensor([-0.0, 0.0, -0.0], device='cuda').expand(s['B'], 3)))


@pytest.mark.parametrize('which', ['choice', 'fps_idx'])
@pytest.mark.parametrize('bad', [-1, 'size'])
def test_vote_resample_does_not_follow_an_index_outside_its_array(which, bad):
    from point_dae_amd import vote_ops
    s = SIZES['two_chunks_and_tail']
    raw, fps_idx, choice, A, t = _case(C=3, seed=8, **s)
    nan = torch.zeros(s['V'], s['B'], s['npoints'], dtype=torch.bool, device='cuda')
    if which == 'choice':                                   # vote 1, column 290 (the second chunk): every cloud's point
        choice[1, 290] = s['point_all'] if bad == 'size' else bad
        nan[1, :, 290] = True
    else:                                                   # cloud 2's FPS column that vote 2 reads at n = 7
        col = int(choice[2, 7])
        fps_idx[2, col] = s['P'] if bad == 'size' else bad
        nan[:, 2] = choice.long() == col
        assert nan[2, 2, 7] and nan.sum() <= s['V']
    got = vote_ops.vote_resample(raw, fps_idx, choice, A, t)
    assert torch.equal(torch.isnan(got).all(-1), nan) and torch.equal(torch.isnan(got).any(-1), nan)


def test_vote_resample_refuses_bad_arguments_before_launching():
    from point_dae_amd import _lib, vote_ops
    s = SIZES['one_block']
    raw, fps_idx, choice, A, t = _case(C=3, seed=9, **s)
    out = torch.full((s['V'], s['B'], s['npoints'], 3), 777.0, device='cuda')
    with pytest.raises(RuntimeError, match=r'pdae_vote_resample failed.*c >= 3'):
        vote_ops.vote_resample(raw[:, :, :2].contiguous(), fps_idx, choice, A, t, out=out)
    many = (torch.arange(s['V'] * 41, dtype=torch.int32).cuda() % 40).view(s['V'], 41)       # 41 columns of 40 FPS points
    with pytest.raises(RuntimeError, match=r'pdae_vote_resample failed.*npoints > point_all'):
        vote_ops.vote_resample(raw, fps_idx, many, out=torch.full((s['V'], s['B'], 41, 3), 777.0, device='cuda'))
    p = _lib.ptr
    ok = [s['V'], s['B'], s['P'], 3, s['point_all'], s['npoints'], p(raw), p(fps_idx), p(choice), p(A), p(t), p(out)]
    for pos in range(6):                                    # every size, zero and negative
        for v in (0, -1):
            with pytest.raises(RuntimeError, match=r'status -1.*(positive|c >= 3)'):
                _lib.call('pdae_vote_resample', raw, *(ok[:pos] + [v] + ok[pos + 1:]))
    for pos in (6, 7, 8, 11):                               # every required pointer (A and t may be null)
        with pytest.raises(RuntimeError, match=r'status -1.*null pointer'):
            _lib.call('pdae_vote_resample', raw, *(ok[:pos] + [None] + ok[pos + 1:]))
    with pytest.raises(RuntimeError, match=r'status -3.*one launch'):       # a grid of 2^31 blocks
        _lib.call('pdae_vote_resample', raw, *([1 << 16, 1 << 15] + ok[2:]))
    with pytest.raises(ValueError, match='out'):
        vote_ops.vote_resample(raw, fps_idx, choice, A, t, out=out[:2])
    torch.cuda.synchronize()
    assert (out == 777.0).all()                             # nothing was launched


# ---- pdae_vote_reduce --------------------------------------------------------------------------------------------------

def _counter():
    return torch.zeros(1, dtype=torch.int32, device='cuda')


@pytest.mark.parametrize('V,B,K', [(10, 5, 40), (1, 1, 2), (3, 70, 15)])
def test_vote_reduce_mean_pred_and_count(V, B, K):
    from point_dae_amd import vote_ops
    g = torch.Generator().manual_seed(V * 100 + K)
    logits = torch.randn(V, B, K, generator=g) * 3
    labels = torch.randint(0, K, (B,), generator=g)
    mean64 = logits.double().mean(0)
    labels[::2] = mean64.argmax(-1)[::2]                    # half of the rows are hits
    correct = _counter()
    pred, mean = vote_ops.vote_reduce(logits.cuda(), labels.cuda(), correct)
    err, bound = (mean.cpu().double() - mean64).abs().max().item(), (V + 1) * U * logits.abs().max().item()
    print('vote_reduce (%d,%d,%d): |mean - fp64 mean| %.3e, bound %.3e' % (V, B, K, err, bound))
    assert err <= bound
    _, want = vote_ops.reduce_host(mean.cpu().numpy()[None])
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), want)
    assert correct.item() == int((want == labels.numpy()).sum()) >= (B + 1) // 2
    # the mean itself: the host twin's ordered fp32 sum, then one division
    assert torch.equal(_bits(mean.cpu()), _bits(torch.from_numpy(vote_ops.reduce_host(logits.numpy())[0])))
    pred2, none = vote_ops.vote_reduce(logits.cuda(), labels.cuda(), _counter(), want_mean=False)
    assert none is None and torch.equal(pred2, pred)


def test_vote_reduce_ties_go_to_the_lowest_class():
    from point_dae_amd import vote_ops
    g = torch.Generator().manual_seed(1)
    logits = torch.randint(-2, 3, (3, 70, 15), generator=g).float()      # integer sums: exact, and many rows tie at the top
    logits[:, 0] = 0.0                                                     # a row that ties everywhere: class 0
    logits[:, 1, 3], logits[:, 1, 9] = 50.0, 50.0                          # 3 and 9 tie: 3
    s = logits.sum(0)
    assert ((s == s.max(-1, keepdim=True).values).sum(-1) > 1).sum() >= 10
    pred, mean = vote_ops.vote_reduce(logits.cuda(), torch.zeros(70, dtype=torch.int64).cuda(), _counter())
    _, want = vote_ops.reduce_host(logits.numpy())
    assert np.array_equal(pred.cpu().numpy(), want) and want[0] == 0 and want[1] == 3
    assert np.array_equal(want, (s / 3).numpy().argmax(-1))               # numpy's argmax: the first of equals


def test_vote_reduce_nan_rows_foreign_labels_and_accumulation():
    from point_dae_amd import vote_ops
    V, B, K = 3, 9, 15
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(V, B, K, generator=g)
    top = logits.double().mean(0).argmax(-1)
    assert (torch.sort(logits.double().mean(0), -1).values[:, -1] - torch.sort(logits.double().mean(0), -1).values[:, -2]
            > 1e-3).all()                                   # no near tie: fp32 and fp64 agree on the argmax
    labels = top.clone()
    logits[1, 4, 14] = float('nan')                         # row 4: one NaN in one vote (the last class)
    labels[5], labels[6] = K, -1                            # labels outside 0 .. K-1
    labels[7] = (top[7] + 1) % K                            # a plain miss
    correct = _counter()
    pred, mean = vote_ops.vote_reduce(logits.cuda(), labels.cuda(), correct)
    want = top.clone()
    want[4] = -1
    assert torch.equal(pred.cpu(), want) and torch.isnan(mean[4, 14]) and not torch.isnan(mean[4, :14]).any()
    assert correct.item() == 5                              # rows 0 .. 3 and 8
    labels[4] = -1                                          # a label of -1 against the NaN row's -1: still no hit
    vote_ops.vote_reduce(logits.cuda(), labels.cuda(), correct)
    assert correct.item() == 10                             # two launches on one counter accumulate
    with pytest.raises(RuntimeError, match=r'status -3.*classes'):
        vote_ops.vote_reduce(torch.zeros(2, 3, 65, device='cuda'), torch.zeros(3, dtype=torch.int64, device='cuda'), correct)
    with pytest.raises(ValueError, match='one int32 counter'):
        vote_ops.vote_reduce(logits.cuda(), labels.cuda(), torch.zeros(2, dtype=torch.int32, device='cuda'))
    assert correct.item() == 10


# ---- the two backends ----------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _backend(name):
    old = os.environ.get('PDAE_VOTE')
    os.environ['PDAE_VOTE'] = name
    try:
        yield
    finally:
        if old is None:
            del os.environ['PDAE_VOTE']
        else:
            os.environ['PDAE_VOTE'] = old


def _loader():
    """The synthetic ModelNet test subset: 5 clouds of 1300 points in batches of 2 (the last batch has one cloud)."""
    from point_dae_amd import datasets  # noqa: F401
    from point_dae_amd.registry import DATASETS
    return DATASETS.build(dict(NAME='ModelNet', subset='test', npoints=1300, count=5, bs=2, device='cuda', seed=0,
                               NUM_CATEGORY=40, aug_type=['norm']))


def _scratch_model(name):
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    config = cfg_from_yaml_file(CFGS[name])
    torch.manual_seed(0)
    model = builder.model_builder(config.model)
    model.load_model_from_ckpt(None, log=lambda *a: None)
    return config, model.cuda().eval()


def _vote_pass(setup, backend, fps_cache=None):
    """-> (pred, label, mean logits, hits, the next np.random.random() behind the pass)."""
    from point_dae_amd import runner_finetune
    config, model, loader = setup
    with _backend(backend), torch.no_grad():
        np.random.seed(SEED)
        pred, label, mean, correct = runner_finetune.vote_pass(model, loader, config, TIMES, fps_cache)
    return pred.cpu(), label.cpu(), mean.cpu(), correct.item(), np.random.random()


@pytest.fixture(scope='module', params=sorted(CFGS))
def setup(request):
    config, model = _scratch_model(request.param)
    s = (config, model, _loader())
    seen = []                                               # max |logits| of every forward of the torch pass (one per vote)
    hook = model.register_forward_hook(lambda m, inp, out: seen.append(out.detach().abs().max()))
    torch_pass = _vote_pass(s, 'torch')
    hook.remove()
    assert len(seen) == 3 * TIMES
    return types.SimpleNamespace(name=request.param, s=s, torch_pass=torch_pass, max_logit=max(v.item() for v in seen))


def test_backends_agree_on_every_cloud(setup):
    from point_dae_amd import runner_finetune
    pred_t, label, mean_t, hits_t, next_t = setup.torch_pass
    assert tuple(mean_t.shape) == (5, 40) and pred_t.shape == (5,)
    reduce_bound = (TIMES + 1) * U * setup.max_logit
    gap_tol = 2 * FORWARD_DIFF[setup.name] + reduce_bound
    top2 = torch.sort(mean_t, -1).values
    gap = top2[:, -1] - top2[:, -2]
    print('%s: top-2 gaps %s, gap_tol %.3e' % (setup.name, ['%.3e' % v for v in gap.tolist()], gap_tol))
    decided = gap > gap_tol
    assert (~decided).float().mean().item() == 0.0          # the excluded share: this seed leaves no cloud under gap_tol
    pred_h, label_h, mean_h, hits_h, next_h = _vote_pass(setup.s, 'hip')
    assert next_h == next_t                                 # the same draws, the same number of them
    assert torch.equal(label_h, label)
    assert torch.equal(pred_h[decided], pred_t[decided])
    diff = (mean_h - mean_t).abs().max().item()
    print('%s: |mean logits hip - torch| %.3e' % (setup.name, diff))
    assert diff <= gap_tol
    assert hits_h == int((pred_h == label).sum()) and hits_t == int((pred_t == label).sum())
    # test_vote: the same pass as a percentage (fp32, as the reference divides)
    config, model, loader = setup.s
    with _backend('hip'):
        np.random.seed(SEED)
        acc = runner_finetune.test_vote(model, loader, config, None, times=TIMES)
    assert acc == float(np.float32(hits_h) / np.float32(5) * np.float32(100.))


def test_second_pass_reuses_the_fps_cache(setup, monkeypatch):
    from point_dae_amd import runner_finetune
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    cache = []
    first = _vote_pass(setup.s, 'hip', cache)
    assert len(cache) == 3 and [tuple(c.shape) for c in cache] == [(2, 1200), (2, 1200), (1, 1200)]
    for c, (_, _, data) in zip(cache, setup.s[2]):
        assert c.dtype == torch.int32 and torch.equal(c, furthest_point_sample(data[0].contiguous(), 1200))
    kept = [c.clone() for c in cache]

    def no_fps(*a, **k):
        raise AssertionError('FPS ran although the cache holds the batch')
    monkeypatch.setattr(runner_finetune, 'furthest_point_sample', no_fps)
    second = _vote_pass(setup.s, 'hip', cache)
    monkeypatch.undo()
    assert len(cache) == 3 and all(torch.equal(a, b) for a, b in zip(cache, kept))
    plain = _vote_pass(setup.s, 'hip', None)
    for other in (second, plain):                           # the same draws consumed, the same bits out
        assert other[4] == first[4] and other[3] == first[3]
        assert torch.equal(other[0], first[0]) and torch.equal(_bits(other[2]), _bits(first[2]))


def test_voting_refuses_npoints_outside_the_table(setup):
    from point_dae_amd import runner_finetune
    from point_dae_amd.config import AttrDict
    config, model, loader = setup.s
    with pytest.raises(NotImplementedError, match='2048'):
        runner_finetune.test_vote(model, loader, AttrDict(npoints=2048), None, times=1)


# ---- main --test -----------------------------------------------------------------------------------------------------------

def test_main_test_votes_a_saved_checkpoint(tmp_path, monkeypatch, capsys):
    """Nothing is trained: the scratch DGCNN is saved through builder.save_checkpoint and main --test evaluates it on five
    synthetic test clouds: '[TEST] acc', two voting rounds, and their maximum."""
    from point_dae_amd import builder, main
    from point_dae_amd.svm_probe import Acc_Metric
    raw = yaml.safe_load(open(CFGS['DGCNN']))
    base = dict(NAME='ModelNet', DATA_PATH='unused', N_POINTS=1300, NUM_CATEGORY=40, USE_NORMALS=False)
    for subset in ('train', 'val', 'test'):
        raw['dataset'][subset] = dict(_base_=dict(base), others=dict(raw['dataset'][subset]['others'], count=5))
    raw['total_bs'] = 2
    cfg = tmp_path / 'vote.yaml'
    yaml.safe_dump(raw, open(cfg, 'w'))
    _, model = _scratch_model('DGCNN')
    args = types.SimpleNamespace(experiment_path=str(tmp_path / 'saved'), local_rank=0)
    builder.save_checkpoint(model, torch.optim.AdamW(model.parameters()), 0, Acc_Metric(0.), Acc_Metric(0.), 'ckpt-best', args)
    ckpt = tmp_path / 'saved' / 'ckpt-best.pth'
    assert ckpt.exists()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.delenv('PDAE_VOTE', raising=False)
    capsys.readouterr()
    main.main(['--config', str(cfg), '--test', '--ckpts', str(ckpt), '--vote_rounds', '2'])
    out = capsys.readouterr().out
    assert out.count('[TEST] acc = ') == 1 and out.count('[TEST_VOTE_time ') == 2 and out.count('[TEST_VOTE] acc = ') == 1
    assert '[TEST_VOTE_time 1]' in out and '[TEST_VOTE_time 2]' in out and 'Vote backend: hip' in out
    rounds = [float(line.split('acc = ')[1].split(',')[0]) for line in out.splitlines() if '[TEST_VOTE_time ' in line]
    best = [float(line.split('best acc = ')[1]) for line in out.splitlines() if '[TEST_VOTE_time ' in line]
    final = float(out.split('[TEST_VOTE] acc = ')[1].split()[0])
    assert all(0.0 <= a <= 100.0 and round(a / 20.0, 3) == round(a / 20.0) for a in rounds)      # hits of five clouds
    assert best == [rounds[0], max(rounds)] and final == max(rounds)
    assert out.index('[TEST] acc') < out.index('[TEST_VOTE]\n') < out.index('[TEST_VOTE_time 1]') < out.index('[TEST_VOTE] acc')


def test_validate_vote_logs_and_returns_the_metric(setup):
    from point_dae_amd import runner_finetune
    config, model, loader = setup.s
    lines = []
    with _backend('hip'):
        np.random.seed(SEED)
        metric = runner_finetune.validate_vote(model, loader, 7, config, None, log=lines.append, times=TIMES)
        np.random.seed(SEED)
        acc = runner_finetune.test_vote(model, loader, config, None, times=TIMES)
    assert metric.acc == acc and metric.state_dict() == {'acc': acc}
    assert lines[-1] == '[Validation_vote] EPOCH: 7  acc_vote = %.4f' % acc


_VOTE_CHILD = """
import sys
from point_dae_amd import main, runner_finetune
from point_dae_amd.svm_probe import Acc_Metric

def high(base_model, test_loader, epoch, config, args=None, log=print):
    log('[Validation] EPOCH: %d  acc = 95.0000' % epoch)
    return Acc_Metric(95.0)

runner_finetune.run_net = lambda args, config: runner_finetune._run(args, config, print, 20, validate_fn=high)
main.main(sys.argv[1:])
"""


def test_vote_flag_runs_one_voted_validation_behind_a_high_plain_one(tmp_path):
    """run_net --vote in a child process whose plain validation is replaced by one that reports 95 %: the branch of
    runner_finetune.py:254-262 calls validate_vote and saves ckpt-best_vote beside ckpt-best and ckpt-last."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import proc_util
    raw = yaml.safe_load(open(CFGS['DGCNN']))
    base = dict(NAME='ModelNet', DATA_PATH='unused', N_POINTS=1300, NUM_CATEGORY=40, USE_NORMALS=False)
    for subset in ('train', 'val', 'test'):
        raw['dataset'][subset] = dict(_base_=dict(base), others=dict(raw['dataset'][subset]['others'], count=5))
    cfg = tmp_path / 'vote.yaml'
    yaml.safe_dump(raw, open(cfg, 'w'))
    cmd = [sys.executable, '-c', _VOTE_CHILD, '--config', str(cfg), '--scratch_model', '--vote', '--max_epoch', '0',
           '--steps_per_epoch', '2', '--total_bs', '4', '--exp_name', 'v']
    r = proc_util.run(cmd, 300, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert out.count('[Validation] EPOCH: 0') == 1 and out.count('[Validation_vote] EPOCH: 0  acc_vote = ') == 1
    acc = float(out.split('acc_vote = ')[1].split()[0])
    assert 0.0 <= acc <= 100.0
    for name in ('ckpt-best', 'ckpt-last'):
        assert list(tmp_path.glob('experiments/*/*/v/%s.pth' % name)), name
    saved = list(tmp_path.glob('experiments/*/*/v/ckpt-best_vote.pth'))
    # the voted best starts at 0, as the reference's: a voted accuracy of 0 (a model of two steps may miss all five clouds)
    # is no improvement and saves nothing
    assert bool(saved) == (acc > 0.0)
    if saved:
        best_vote = torch.load(str(saved[0]), map_location='cpu')
        assert best_vote['metrics'] == {'acc': 95.0} and abs(best_vote['best_metrics']['acc'] - acc) < 1e-3
