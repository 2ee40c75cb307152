"""The PointNet++ classifier PointNetv2 (point_dae_amd/point_cae_pointnetv2.py) and its fine-tuning loop on the GPU.

  * the live-reference fixture tests/golden/pointnetv2_cls_b2.npz (B = 2, N = 1024): the kernels' FPS and ball-query indices
    equal the recorded ones; evaluation-mode logits, and training-mode logits, loss and every parameter gradient, under
    both PDAE_SA_FIRST settings.  Bounds: FACTOR times the reference's OWN fp32-against-fp64 distance, which the fixture
    records (at B = 2 the head's BatchNorm1d layers normalise over two rows, which amplifies rounding: 7e-4 on the logits,
    1.9e-2 on the worst gradient tensor, see tests/golden/make_pointnetv2_cls_fixtures.py), and the split form within
    FACTOR of the grouped form's error;
  * run_net on the synthetic ModelNet stand-in: the step is one hipGraph replay, a second replay changes the parameters,
    the checkpoints are written, --test votes one round on ckpt-best, a reloaded checkpoint reproduces the logits;
  * a few-shot episode epoch, optimizer.part diff_lr, and PDAE_DETERMINISTIC=1 run to run.
"""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import weights  # noqa: E402
from test_pointnetv2_cls_cpu import CFG, ZERO_GRAD, build_model, fixture, grad_entry  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
EVAL_PIN = 1e-5            # the bound tests/test_gpu_svmfeat.py sets for the same fused encoder against the same reference
MODES = ('grouped', 'split')


def _rel(got, want):
    got, want = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float((got - want).abs().max() / want.abs().max())


def _filled(f, monkeypatch, mode):
    monkeypatch.setenv('PDAE_SA_FIRST', mode)
    model = weights.fill_state(build_model(), int(f['seed']))
    assert model.sa_first == mode
    for m in model.cls_head_finetune:
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0                                 # as the generator set the reference's
    return model.cuda()


def _check_geometry(cap, f):
    for lvl in range(2):
        assert torch.equal(cap['fps_idx'][lvl].cpu(), torch.from_numpy(f['fps_idx%d' % lvl])), lvl
        assert torch.equal(cap['ball_idx'][lvl].cpu(), torch.from_numpy(f['ball_idx%d' % lvl])), lvl


def test_evaluation_logits_on_the_live_reference_fixture(monkeypatch):
    from point_dae_amd import _lib
    f = fixture()
    outs = {}
    for mode in MODES:
        model = _filled(f, monkeypatch, mode).eval()
        calls, cap = [], {}
        monkeypatch.setattr(_lib, 'CALL_HOOK', lambda name, args: calls.append(name))
        with torch.no_grad():
            logits = model(torch.from_numpy(f['pts']).cuda(), capture=cap)
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, 'CALL_HOOK', None)
        _check_geometry(cap, f)
        assert calls.count('pdae_sa_eval_forward') == 2 and 'pdae_sa_first_forward' not in calls   # the fused levels
        err = _rel(logits, f['eval_logits64'])
        print('PDAE_SA_FIRST=%s evaluation logits vs reference fp64 %.3e (reference fp32 %.2e)' % (mode, err, float(f['eval_dist'])))
        assert logits.shape == (2, 40) and err <= EVAL_PIN
        outs[mode] = logits
    assert torch.equal(outs['grouped'], outs['split'])                 # the switch does not reach evaluation mode


def test_training_logits_loss_and_gradients_on_the_live_reference_fixture(monkeypatch):
    """Both forms on the recorded geometry.  The grouped run's max-pool winners are injected into the split run
    (sa_mlp.ARG_HOOK), so that a near-tie which rounding resolves the other way does not decide a gradient comparison."""
    from point_dae_amd import _lib, sa_mlp
    f = fixture()
    pts, labels = torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['labels']).cuda()
    errs, winners = {}, []
    was = _lib.deterministic()
    _lib.set_deterministic(True)                     # ordered reductions: the figures below are the same on every run
    try:
        for mode in MODES:
            model = _filled(f, monkeypatch, mode).train()
            calls, cap, seen = [], {}, []

            def hook(arg):
                seen.append(arg.clone())
                return arg if mode == 'grouped' else winners[len(seen) - 1]
            monkeypatch.setattr(_lib, 'CALL_HOOK', lambda name, args: calls.append(name))
            sa_mlp.ARG_HOOK = hook
            try:
                logits = model(pts, capture=cap)
                loss, _ = model.get_loss_acc(logits, labels)
                loss.backward()
            finally:
                sa_mlp.ARG_HOOK = None
                monkeypatch.setattr(_lib, 'CALL_HOOK', None)
            torch.cuda.synchronize()
            _check_geometry(cap, f)
            assert len(seen) == 3
            if mode == 'grouped':
                winners = seen
                assert 'pdae_sa_first_forward' not in calls and calls.count('pdae_sa_group_rows') == 2
            else:
                assert cap['first'] == ['split', 'split']
                assert calls.count('pdae_sa_first_forward') == 2 and calls.count('pdae_sa_first_backward') == 2
                assert 'pdae_sa_group_rows' not in calls and 'pdae_sa_group_rows_grad' not in calls
                print('winners the split form chose differently: %s' % [int((a != b).sum()) for a, b in zip(seen, winners)])
            e = {'logits': _rel(logits, f['train_logits64']),
                 'loss': abs(loss.item() - float(f['loss64'])) / float(f['loss64'])}
            noise = {}
            for n, p in model.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
                want, take = grad_entry(f, n)
                if n in ZERO_GRAD:
                    noise[n] = float(p.grad.abs().max())
                else:
                    e['d ' + n] = _rel(take(p.grad.cpu()), want)
            errs[mode] = (e, noise)
    finally:
        _lib.set_deterministic(was)
    ref32 = {'logits': float(f['train_dist']), 'loss': float(f['loss_dist'])}
    scale = max(float(np.abs(f[k]).max()) for k in f if k.startswith('grad/') and not k.endswith('/norm'))
    for k in errs['grouped'][0]:
        g, s = errs['grouped'][0][k], errs['split'][0][k]
        own = ref32.get(k, float(f['grad_dist']))
        print('%-60s grouped %.3e  split %.3e  (reference fp32 %.2e)' % (k, g, s, own))
        assert g <= FACTOR * own, (k, g, own)
        assert s <= FACTOR * g, (k, s, g)
    # analytically zero gradients: rounding noise of sums whose terms are of the other gradients' size (2^-24 per term,
    # at most 1024 terms)
    for mode in MODES:
        for n, v in errs[mode][1].items():
            print('%-60s %s |g| max %.3e (zero analytically)' % (n, mode, v))
            assert v <= 1024 * 2.0 ** -24 * scale, (mode, n, v, scale)


def _small_config(tmp_path, name='ModelNet', count=None, **top):
    raw = yaml.safe_load(open(CFG))
    base = dict(NAME=name, DATA_PATH='no_such_directory', N_POINTS=1300, NUM_CATEGORY=40, USE_NORMALS=False)
    for subset in ('train', 'val', 'test'):
        others = dict(raw['dataset'][subset]['others'])
        if count is not None:
            others['count'] = count
        raw['dataset'][subset] = dict(_base_=dict(base), others=others)
    raw.update(top)
    cfg = tmp_path / 'small.yaml'
    yaml.safe_dump(raw, open(cfg, 'w'))
    return cfg


def test_run_net_replays_one_graph_and_the_checkpoints_reload(tmp_path, monkeypatch, capsys):
    from point_dae_amd import builder, graph_step, main, parser, runner_finetune
    from point_dae_amd.config import get_config
    from point_dae_amd.misc import set_random_seed
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    cfg = _small_config(tmp_path, count=24)                          # (the test set too: three validation batches)
    args = parser.get_args(['--config', str(cfg), '--scratch_model', '--max_epoch', '1', '--steps_per_epoch', '3', '--total_bs', '8',
                            '--exp_name', 'g'])
    args.distributed, args.world_size, args.use_gpu = False, 1, True
    config = get_config(args)
    config.total_bs, config.max_epoch = args.total_bs, args.max_epoch
    config.dataset.train.others.bs = config.total_bs
    set_random_seed(args.seed)
    snaps = []
    orig = graph_step.GraphedClassifierStep._run

    def spy(self):
        snaps.append((self.graph is not None, self.model.flat_param.clone(),
                      int(self.model.module.pointnetv2_encoder.sa1.mlps[0].layer0.bn.bn.num_batches_tracked)))
        return orig(self)
    monkeypatch.setattr(graph_step.GraphedClassifierStep, '_run', spy)
    lines = []
    model = runner_finetune.run_net(args, config, log=lambda s: lines.append(str(s)))
    assert 'step: hipGraph replay (GraphedClassifierStep)' in lines
    assert 'Training from scratch!!!' in lines
    # six steps: two eager, the capture + first replay, then replays; the parameters move between two replayed steps and
    # num_batches_tracked advances by one per step, replayed or not
    assert [s[0] for s in snaps] == [False, False, False, True, True, True]
    assert not torch.equal(snaps[4][1], snaps[5][1]) and not torch.equal(snaps[5][1], model.flat_param)
    assert [s[2] for s in snaps] == [0, 1, 2, 3, 4, 5]
    assert sum('[Validation] EPOCH: ' in ln for ln in lines) == 2
    exp = args.experiment_path
    best, last = os.path.join(exp, 'ckpt-best.pth'), os.path.join(exp, 'ckpt-last.pth')
    assert os.path.exists(best) and os.path.exists(last)
    # ckpt-last holds the final state: a fresh model that loads it gives the live model's evaluation logits bit for bit
    pts = torch.from_numpy(fixture()['pts']).cuda()
    live = model.module.eval()
    fresh = build_model()
    builder.load_model(fresh, last)
    fresh = fresh.cuda().eval()
    with torch.no_grad():
        a, b = live(pts), fresh(pts)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # --test on ckpt-best: the plain accuracy and one voted round
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    capsys.readouterr()
    main.main(['--config', str(cfg), '--test', '--ckpts', best, '--vote_rounds', '1', '--total_bs', '8', '--exp_name', 'g_test'])
    out = capsys.readouterr().out
    assert out.count('[TEST] acc = ') == 1 and out.count('[TEST_VOTE_time ') == 1 and out.count('[TEST_VOTE] acc = ') == 1


def test_a_few_shot_episode_epoch_runs(tmp_path, monkeypatch, capsys):
    from point_dae_amd import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    cfg = _small_config(tmp_path, name='ModelNetFewShot')
    capsys.readouterr()
    main.main(['--config', str(cfg), '--scratch_model', '--way', '5', '--shot', '10', '--fold', '0', '--max_epoch', '0',
               '--total_bs', '10', '--exp_name', 'f'])
    out = capsys.readouterr().out
    assert 'args.way : 5' in out and 'args.shot : 10' in out and 'args.fold : 0' in out
    assert 'step: hipGraph replay (GraphedClassifierStep)' in out and '[Batch 5/5]' in out       # 50 clouds, 10 per step
    losses = [float(ln.split('Loss = ')[1].split()[0]) for ln in out.splitlines() if ln.startswith('[Epoch ') and 'Loss = ' in ln]
    assert losses and all(np.isfinite(losses))
    assert out.count('[Validation] EPOCH: 0  acc = ') == 1
    assert list(tmp_path.glob('experiments/*/*/f/ckpt-last.pth'))


def _stepper(part='all'):
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.finetune_ops import GradNormClip
    config = cfg_from_yaml_file(CFG)
    config.optimizer.part = part
    torch.manual_seed(0)
    net = weights.fill_state(build_model(), 5).cuda().train()
    model = FlatDataParallel(net)
    opt, _ = builder.build_opti_sche(model, config)
    model.zero_grad()
    return config, net, model, opt, GradNormClip(model.flat_grad, config.grad_norm_clip)


def test_diff_lr_builds_the_reference_groups_and_steps():
    from point_dae_amd import builder
    from point_dae_amd.graph_step import use_created_stream
    from point_dae_amd.runner_finetune import train_step
    from point_dae_amd.synthetic import labelled_clouds
    use_created_stream()
    config, net, model, opt, clip = _stepper('diff_lr')
    groups = builder.add_weight_decay(net, 0.05, part='diff_lr', lr=0.002)
    assert [len(g['params']) > 0 for g in groups] == [True, True, False, False]      # the new-parameter pair is empty
    assert [g.get('lr') for g in groups] == [0.002 * 0.1, 0.002 * 0.1, None, None]
    assert [g['weight_decay'] for g in groups] == [0.0, 0.05, 0.0, 0.05]
    named = dict(net.named_parameters())
    pre = {id(p) for g in groups[:2] for p in g['params']}
    assert pre == {id(p) for n, p in named.items() if 'cls' not in n}
    x, y = labelled_clouds(4, 1024, seed=2)
    before = {n: p.detach().clone() for n, p in named.items()}
    loss, _ = train_step(model, opt, clip, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    assert np.isfinite(loss.item())
    moved = {n for n, p in named.items() if not torch.equal(p.detach(), before[n])}
    # (the reference's quirk: the head's parameters are in no returned group, so only the pretrained ones move)
    assert not any('cls' in n for n in moved), sorted(n for n in moved if 'cls' in n)
    assert all(n in moved for n in named if n.endswith('conv.weight')), sorted(set(named) - moved)[:4]


def test_deterministic_mode_repeats_the_loss_sequence(monkeypatch):
    """Two runs of three steps under the default setting (split: every sum of csrc/sa_train.hip has a fixed order).  The
    grouped form is left out on purpose: its feature gradient is pdae_sa_group_rows_grad's, whose per-point sums are taken in
    the sort's order of arrival (include/pdae.h) -- deterministic mode never covered them, for the pretraining step either."""
    from point_dae_amd import _lib
    from point_dae_amd.graph_step import use_created_stream
    from point_dae_amd.point_cae_pointnetv2 import SA_FIRST_DEFAULT
    from point_dae_amd.runner_finetune import train_step
    from point_dae_amd.synthetic import labelled_clouds
    monkeypatch.delenv('PDAE_SA_FIRST', raising=False)
    use_created_stream()
    x, y = labelled_clouds(12, 1024, seed=4)
    xs, ys = torch.from_numpy(x).cuda().split(4), torch.from_numpy(y).cuda().split(4)
    was = _lib.deterministic()
    _lib.set_deterministic(True)                      # what PDAE_DETERMINISTIC=1 does at the first kernel call
    try:
        runs = []
        for _ in range(2):
            config, net, model, opt, clip = _stepper()
            assert net.sa_first == SA_FIRST_DEFAULT == 'split'
            torch.manual_seed(11)
            runs.append([train_step(model, opt, clip, xs[i], ys[i])[0].item() for i in range(3)])
    finally:
        _lib.set_deterministic(was)
    print('losses %s' % runs[0])
    assert runs[0] == runs[1] and all(np.isfinite(runs[0])) and len(set(runs[0])) == 3
