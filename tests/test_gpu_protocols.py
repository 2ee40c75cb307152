"""The frozen-encoder protocols (optimizer.part only_new / diff_lr) on the GPU: the segmented fused AdamW, the head block
with a frozen BatchNorm under a live Dropout, the two protocol models against the live-reference fixtures
(tests/golden/protocol_*_b4.npz), the graphed step, and the CLI end to end in child processes."""
import ast
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import _rel, _Without, check_grads, fill_state, grad_sample, load_fixture
from moments import fill_moments               # (tests/golden, on the path through golden_util)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {'linear': os.path.join(ROOT, 'cfgs', 'finetune_modelnet_linear_classification.yaml'),
        'nonlinear': os.path.join(ROOT, 'cfgs', 'finetune_modelnet_non_linear_classification.yaml'),
        'diff_lr': os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features_diff_lr.yaml')}


# ---- segmented AdamW ---------------------------------------------------------------------------------------------------

def _flat_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [t.cuda() for t in (torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01,
                               torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4)]


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('nd,wd_count', [(1000, 5003), (64, 22_000_001), (0, 4096)])
def test_segments_bit_equal_two_range_launches(nd, wd_count, scaled):
    """Two segments laid as FlatDataParallel lays no_decay_range / decay_range (the second 256-byte aligned, a padding
    between them and -- here -- behind them) against two pdae_adamw_step[_gscale] launches, three steps with an lr
    change: parameters and both moments bit-equal; the padding bit-unchanged."""
    from point_dae_amd import _lib
    pad = (-nd) % 64
    n = nd + pad + wd_count + 37
    ranges = [(0, nd, 0.0), (nd + pad, wd_count, 0.05)]
    p, g, m, v = _flat_state(n, nd + wd_count)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    gs = torch.full((1,), 0.37, device='cuda') if scaled else None
    for step, lr in ((1, 1e-2), (2, 1e-2), (3, 3.3e-3)):
        _lib.adamw_step_segments(p, g, m, v, [(o, c, lr, wd) for o, c, wd in ranges], 0.9, 0.999, 1e-8, step, gs)
        for o, c, wd in ranges:
            if c == 0:
                continue
            args = (p2, c, p2[o:].data_ptr(), g[o:].data_ptr(), m2[o:].data_ptr(), v2[o:].data_ptr(), lr, 0.9, 0.999, 1e-8,
                    wd, step)
            if scaled:
                _lib.call('pdae_adamw_step_gscale', *args, gs.data_ptr())
            else:
                _lib.call('pdae_adamw_step', *args)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)
    outside = torch.ones(n, dtype=torch.bool, device='cuda')
    for o, c, _ in ranges:
        outside[o:o + c] = False
    assert int(outside.sum()) == pad + 37
    for a, b in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(a[outside], b[outside])
        assert nd == 0 or not torch.equal(a[:nd], b[:nd])


def test_segments_unaligned_heads_and_tails_and_untouched_gaps():
    """Eight segments with every head / tail length, one shorter than a float4, against the fp64 formula; every element
    outside them keeps its bits (a NaN gradient there is never read into a moment)."""
    from point_dae_amd import _lib
    n = 6000
    segs = [(1, 9, 1e-2, 0.0), (13, 2, 1e-3, 0.05), (18, 1001, 1e-2, 0.05), (1024, 512, 5e-3, 0.0), (1539, 5, 1e-2, 0.1),
            (2000, 3, 1e-2, 0.0), (3001, 2047, 2e-3, 0.05), (5998, 2, 1e-2, 0.05)]
    p, g, m, v = _flat_state(n, 3)
    inside = torch.zeros(n, dtype=torch.bool, device='cuda')
    for o, c, _, _ in segs:
        inside[o:o + c] = True
    g[~inside] = float('nan')
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    coef = torch.full((1,), 0.5, device='cuda')
    _lib.adamw_step_segments(p, g, m, v, segs, 0.9, 0.999, 1e-8, 4, coef)
    for a, b in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(a[~inside], b[~inside])
    for o, c, lr, wd in segs:
        gg = g[o:o + c].double() * 0.5
        mm = 0.9 * m0[o:o + c].double() + 0.1 * gg
        vv = 0.999 * v0[o:o + c].double() + 0.001 * gg * gg
        pp = p0[o:o + c].double() * (1 - lr * wd) - lr / (1 - 0.9 ** 4) * mm / (vv.sqrt() / (1 - 0.999 ** 4) ** 0.5 + 1e-8)
        assert _rel(p[o:o + c], pp) <= 1e-6 and _rel(m[o:o + c], mm) <= 1e-6 and _rel(v[o:o + c], vv) <= 1e-6


def test_segments_entry_refuses_bad_tables():
    from point_dae_amd import _lib
    p, g, m, v = _flat_state(256, 1)
    for segs in ([(0, 300, 1e-3, 0.0)], [(-4, 8, 1e-3, 0.0)], [(0, 64, 1e-3, 0.0), (60, 8, 1e-3, 0.0)]):
        with pytest.raises(RuntimeError, match='adamw_step_segments'):
            _lib.adamw_step_segments(p, g, m, v, segs, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError, match='num_segments'):
        table = (_lib.AdamwSegment * 9)(*[_lib.AdamwSegment(8 * i, 4, 1e-3, 0.0) for i in range(9)])
        _lib.call('pdae_adamw_step_segments', p, 256, 9, table, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                  0.9, 0.999, 1e-8, 1, None)


class _TinyNet(torch.nn.Module):
    """A backbone and 'cls' parameters named so that builder.add_weight_decay sorts them as it sorts the classifiers'."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.cls_token = torch.nn.Parameter(torch.randn(1, 1, 64) * 0.1)
        self.cls_pos = torch.nn.Parameter(torch.randn(1, 1, 64) * 0.1)
        self.backbone = torch.nn.Sequential(torch.nn.Linear(37, 64), torch.nn.LayerNorm(64))
        self.middle = torch.nn.Linear(64, 63)
        self.cls_head_finetune = torch.nn.Sequential(torch.nn.Linear(63, 13))

    def forward(self, x):
        h = self.backbone(x) * (1 + self.cls_token[0]) + self.cls_pos[0]
        return self.cls_head_finetune(torch.tanh(self.middle(h)))


@pytest.mark.parametrize('max_norm', [0.05, 100.0])
@pytest.mark.parametrize('part', ['only_new', 'diff_lr'])
def test_flat_adamw_part_matches_torch_adamw_over_the_reference_groups(part, max_norm):
    """FlatAdamW(part=...) against clip_grad_norm_ + torch.optim.AdamW over builder.add_weight_decay's groups (the
    reference's, test_protocols_cpu.py), five steps with an lr change (each group from its own base value) and the clip
    coefficient; the state_dict loads into torch.optim.AdamW and back."""
    from point_dae_amd import builder, finetune_ops as F
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.optim import FlatAdamW
    net = _TinyNet().cuda()
    ref = copy.deepcopy(net)
    start = {n: p.detach().clone() for n, p in ref.named_parameters()}
    model = FlatDataParallel(net)
    opt = FlatAdamW(model, lr=1e-2, weight_decay=0.05, part=part)
    ropt = torch.optim.AdamW(builder.add_weight_decay(ref, 0.05, part=part, lr=1e-2), lr=1e-2)
    assert [g['lr'] for g in opt.param_groups] == [g['lr'] for g in ropt.param_groups]
    assert [g['weight_decay'] for g in opt.param_groups] == [g['weight_decay'] for g in ropt.param_groups]
    clip = F.GradNormClip(model.flat_grad, max_norm)
    for i in range(5):
        if i == 3:
            for o in (opt, ropt):
                for g in o.param_groups:
                    g['lr'] = g['lr'] * 0.31
        x = torch.randn(16, 37, device='cuda')
        (model(x) ** 2).mean().backward()
        opt.step(grad_scale=clip())
        opt.zero_grad()
        (ref(x) ** 2).mean().backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        ropt.step()
        ref.zero_grad()                     # (the runner's base_model.zero_grad(): the frozen parameters' gradients too)
    in_groups = {id(p) for g in ropt.param_groups for p in g['params']}
    moved = 0
    for (n, a), b in zip(net.named_parameters(), ref.parameters()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (n, (a - b).abs().max())
        if id(b) in in_groups:
            moved += int(not torch.equal(a, start[n]))
        else:
            assert torch.equal(a, start[n]), n                  # outside the optimiser: bit-unchanged
    assert moved == len(in_groups)
    # state_dict: torch.optim.AdamW's layout over exactly those groups, both ways
    sd = opt.state_dict()
    assert sorted(sd['state']) == list(range(len(in_groups)))
    assert [g['params'] for g in sd['param_groups']] == [g['params'] for g in ropt.state_dict()['param_groups']]
    ropt2 = torch.optim.AdamW(builder.add_weight_decay(ref, 0.05, part=part, lr=1e-2), lr=1e-2)
    ropt2.load_state_dict(sd)
    for k, st in ropt.state_dict()['state'].items():
        got = ropt2.state_dict()['state'][k]
        assert int(got['step']) == int(st['step']) == 5
        assert torch.allclose(got['exp_avg'], st['exp_avg'], rtol=1e-5, atol=1e-8)
        assert torch.allclose(got['exp_avg_sq'], st['exp_avg_sq'], rtol=1e-5, atol=1e-10)
    opt2 = FlatAdamW(FlatDataParallel(copy.deepcopy(ref)), lr=1e-2, weight_decay=0.05, part=part)
    opt2.load_state_dict(ropt.state_dict())
    assert opt2.steps == 5
    back = opt2.state_dict()
    for k, st in ropt.state_dict()['state'].items():
        assert torch.equal(back['state'][k]['exp_avg'], st['exp_avg'])
        assert torch.equal(back['state'][k]['exp_avg_sq'], st['exp_avg_sq'])
    assert [g['lr'] for g in opt2.param_groups] == [g['lr'] for g in ropt.param_groups]


def test_part_all_keeps_its_two_launches():
    from point_dae_amd import _lib
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.optim import FlatAdamW
    model = FlatDataParallel(_TinyNet().cuda())
    opt = FlatAdamW(model, lr=1e-2, weight_decay=0.05)
    (model(torch.randn(4, 37, device='cuda')) ** 2).mean().backward()
    seen = []
    _lib.CALL_HOOK = lambda name, args: seen.append(name)
    try:
        opt.step()
        FlatAdamW(model, lr=1e-2, weight_decay=0.05, part='only_new').step()
    finally:
        _lib.CALL_HOOK = None
    assert seen == ['pdae_adamw_step', 'pdae_adamw_step', 'pdae_adamw_step_segments']


# ---- the head block with a frozen BatchNorm ------------------------------------------------------------------------------

@pytest.mark.parametrize('slope', [None, 0.2])
@pytest.mark.parametrize('B', [2, 4, 32, 33, 128])
@pytest.mark.parametrize('N', [512, 4, 256])
def test_eval_bn_act_dropout_matches_batchnorm1d_eval(B, N, slope):
    """nn.BatchNorm1d.eval() -> ReLU / LeakyReLU -> the injected-mask dropout, forward and backward (the shapes and
    tolerances of test_bn_relu_dropout_matches_batchnorm1d); running statistics bit-unchanged."""
    from point_dae_amd import finetune_ops as F
    g = torch.Generator().manual_seed(B * 7 + N)
    mine = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        mine.weight.copy_(1 + 0.2 * torch.randn(N, generator=g))
        mine.bias.copy_(0.1 * torch.randn(N, generator=g))
        mine.running_mean.copy_(0.1 * torch.randn(N, generator=g))
        mine.running_var.copy_(torch.rand(N, generator=g) + 0.5)
    ref = copy.deepcopy(mine).double().eval()
    mine = mine.cuda().eval()
    state = [b.clone() for b in mine.buffers()]
    y = (torch.randn(B, N, generator=g) * 2 + 0.3).cuda().requires_grad_()
    keep = torch.rand(B, N, generator=g) >= 0.5
    act = torch.relu if slope is None else (lambda t: torch.nn.functional.leaky_relu(t, slope))
    if slope is None:
        out = F.bn_relu_dropout(y, mine, 0.5, keep=keep.cuda(), dropout=True)
    else:
        out = F.bn_lrelu_dropout(y, mine, 0.5, slope, keep=keep.cuda(), dropout=True)
    yr = y.detach().double().cpu().requires_grad_()
    want = act(ref(yr)) * keep.double() / 0.5
    assert _rel(out, want) <= 1e-5
    d = torch.randn(B, N, generator=g).cuda()
    out.backward(d)
    want.backward(d.double().cpu())
    term = float((ref.weight.detach().abs() / (ref.running_var + mine.eps).sqrt()).max() * d.abs().max())
    assert float((y.grad.double().cpu() - yr.grad).abs().max()) <= 1e-4 * max(float(yr.grad.abs().max()), 1e-2 * term)
    assert _rel(mine.weight.grad, ref.weight.grad) <= 1e-5
    assert _rel(mine.bias.grad, ref.bias.grad) <= 1e-5
    for b, s in zip(mine.buffers(), state):
        assert torch.equal(b, s)
    assert int(mine.num_batches_tracked) == 0
    # the uniform draw, and a frozen BatchNorm inside an eval-mode model: no dropout
    u = torch.rand(B, N, generator=g)
    fn = (lambda **k: F.bn_relu_dropout(y.detach(), mine, 0.5, **k)) if slope is None else \
        (lambda **k: F.bn_lrelu_dropout(y.detach(), mine, 0.5, slope, **k))
    with torch.no_grad():
        plain = act(ref(y.detach().double().cpu()))
    assert _rel(fn(u=u.cuda(), dropout=True), plain * (u >= 0.5).double() / 0.5) <= 1e-5
    assert _rel(fn(u=u.cuda(), dropout=False), plain) <= 1e-5
    assert torch.equal(fn(u=u.cuda()), fn(u=u.cuda(), dropout=False))


def test_eval_bn_block_backward_without_dropout():
    """The eval-mode backward with no draw (a frozen BatchNorm and no Dropout under a required gradient: an eval-mode
    model, or p = 0) against nn.BatchNorm1d.eval() -> ReLU / LeakyReLU on the CPU, the tolerances of the test above; one
    column block partly filled, and B = 1, which only the running estimates allow."""
    from point_dae_amd import finetune_ops as F
    for B, N, slope in ((1, 260, None), (5, 260, 0.2), (5, 260, None)):
        g = torch.Generator().manual_seed(B + N)
        mine = torch.nn.BatchNorm1d(N)
        with torch.no_grad():
            mine.weight.copy_(1 + 0.2 * torch.randn(N, generator=g))
            mine.bias.copy_(0.1 * torch.randn(N, generator=g))
            mine.running_mean.copy_(0.1 * torch.randn(N, generator=g))
            mine.running_var.copy_(torch.rand(N, generator=g) + 0.5)
        ref = copy.deepcopy(mine).double().eval()
        mine = mine.cuda().eval()
        state = [b.clone() for b in mine.buffers()]
        y = (torch.randn(B, N, generator=g) * 2 + 0.3).cuda().requires_grad_()
        u = torch.rand(B, N, generator=g).cuda()
        if slope is None:
            out = F.bn_relu_dropout(y, mine, 0.5, u=u, dropout=False)
            act = torch.relu
        else:
            out = F.bn_lrelu_dropout(y, mine, 0.5, slope, u=u, dropout=False)
            act = lambda t: torch.nn.functional.leaky_relu(t, slope)                     # noqa: E731
        yr = y.detach().double().cpu().requires_grad_()
        want = act(ref(yr))
        assert _rel(out, want) <= 1e-5
        d = torch.randn(B, N, generator=g).cuda()
        out.backward(d)
        want.backward(d.double().cpu())
        term = float((ref.weight.detach().abs() / (ref.running_var + mine.eps).sqrt()).max() * d.abs().max())
        assert float((y.grad.double().cpu() - yr.grad).abs().max()) <= 1e-4 * max(float(yr.grad.abs().max()), 1e-2 * term)
        assert _rel(mine.weight.grad, ref.weight.grad) <= 1e-5
        assert _rel(mine.bias.grad, ref.bias.grad) <= 1e-5
        for b, s in zip(mine.buffers(), state):
            assert torch.equal(b, s)


def test_bn_block_entry_checks_the_frozen_mode():
    """The entry's checks in mode 2 (running estimates under a live draw): B = 1 runs and needs neither mean nor invstd;
    null running estimates, a mode outside 0 / 1 / 2 and a bad p are refused before any launch; mode 1 still needs
    B >= 2.  The wrapper refuses a frozen BatchNorm that tracks no running statistics the same way."""
    from point_dae_amd import _lib, finetune_ops as F
    N = 260
    g = torch.Generator().manual_seed(5)
    bn = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        bn.running_mean.copy_(0.1 * torch.randn(N, generator=g))
        bn.running_var.copy_(torch.rand(N, generator=g) + 0.5)
    ref = copy.deepcopy(bn).double().eval()
    bn = bn.cuda().eval()
    y = torch.randn(1, N, generator=g).cuda()
    u = torch.rand(1, N, generator=g).cuda()
    out = torch.empty_like(y)

    def entry(mode, rmean=bn.running_mean.data_ptr(), rvar=bn.running_var.data_ptr(), p=0.5):
        _lib.call('pdae_bn_relu_dropout', y, 1, N, y.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.eps,
                  bn.momentum, rmean, rvar, bn.num_batches_tracked.data_ptr(), mode, p, u.data_ptr(), out.data_ptr(),
                  None, None)
    entry(2)
    want = torch.relu(ref(y.double().cpu())) * (u.cpu() >= 0.5).double() / 0.5
    assert _rel(out, want) <= 1e-5 and int(bn.num_batches_tracked) == 0
    for kw in (dict(rmean=None), dict(rvar=None)):
        for mode in (0, 2):
            with pytest.raises(RuntimeError, match='eval mode reads the running estimates'):
                entry(mode, **kw)
    for mode in (3, -1):
        with pytest.raises(RuntimeError, match='training must be 0, 1 or 2'):
            entry(mode)
    with pytest.raises(RuntimeError, match='0 <= p < 1'):
        entry(2, p=1.0)
    with pytest.raises(RuntimeError, match='B >= 2'):
        entry(1)
    untracked = torch.nn.BatchNorm1d(N, track_running_stats=False).cuda().eval()
    for dropout in (True, False):
        with pytest.raises(RuntimeError, match='eval mode reads the running estimates'):
            F.bn_relu_dropout(y, untracked, 0.5, u=u, dropout=dropout)


def test_training_mode_block_keeps_the_recorded_bits():
    """With the model's flag and the BatchNorm's flag equal the block computes what it computed before it learnt the
    frozen mode: tests/golden/bn_block_train.npz holds the results of the build before (make_bn_block_fixture.py), and
    forward, dy, dgamma, dbeta and the running estimates equal them bit for bit, with the flag left out and given."""
    from make_bn_block_fixture import SLOPE, run
    fx = load_fixture('bn_block_train.npz')
    for key, slope in (('relu', None), ('lrelu', SLOPE)):
        for kw in ({}, dict(dropout=True)):
            for k, v in run(slope, **kw).items():
                assert np.array_equal(v.cpu().numpy(), fx['%s/%s' % (key, k)]), (key, k, kw)


# ---- the protocol models against the live reference --------------------------------------------------------------------

def _protocol_model(kind, fx):
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.runner_finetune import set_train_mode
    cfg = cfg_from_yaml_file(CFGS[kind])
    for k, v in ast.literal_eval(str(fx['overrides'])):
        cfg.model[k] = v
    model = fill_state(builder.model_builder(cfg.model), int(fx['seed'])).cuda()
    return set_train_mode(model, 'only_new'), cfg


def _oracle(kind, cfg, fx):
    """test_gpu_finetune's CPU restatement with this protocol's head and BatchNorm modes, in fp64."""
    from point_dae_amd import builder
    from point_dae_amd.runner_finetune import set_bn_eval
    from test_gpu_finetune import _OracleClassifier
    ref = _OracleClassifier(cfg.model)
    if kind == 'linear':
        ref.cls_head_finetune = torch.nn.Sequential(torch.nn.Linear(2 * cfg.model.trans_dim, cfg.model.cls_dim))
    ref.load_state_dict(fill_state(builder.model_builder(cfg.model), int(fx['seed'])).state_dict())
    ref = ref.double().train()
    ref.apply(set_bn_eval)
    return ref


def _oracle_logits(kind, ref, pts, keeps):
    from oracle import model as OM
    nb, center = OM.group_divider(pts.float(), ref.G, ref.k)
    nb, center = nb.double(), center.double()
    B = pts.shape[0]
    x = torch.cat([ref.cls_token.expand(B, -1, -1), ref.encoder(nb)], 1)
    pos = torch.cat([ref.cls_pos.expand(B, -1, -1), ref.pos_embed(center)], 1)
    x = ref.norm(ref.blocks(x, pos))
    f = torch.cat([x[:, 0], x[:, 1:].max(1)[0]], -1)
    h = ref.cls_head_finetune
    if kind == 'linear':
        return h[0](f)
    f = torch.relu(h[1](h[0](f))) * keeps[0] / 0.5
    f = torch.relu(h[5](h[4](f))) * keeps[1] / 0.5
    return h[8](f)


def _tie_correction(kind, cfg, fx, decisions, labels, keeps):
    """test_gpu_finetune._tie_correction for the protocol models: the fp64 oracle at the product's own embedder decisions
    and at the same decisions with the fixture's recorded near-ties set the reference's way -> (d logits, d loss,
    {name: d grad}) or None when they agree.  Every decision the product takes otherwise than the oracle is a near-tie."""
    from oracle import model as OM
    from test_gpu_finetune import _assert_near_ties, _embed_decisions, _hook_embedder
    relus, winners = _embed_decisions(decisions)
    ref_relus, ref_winners = [m.clone() for m in relus], [w.clone() for w in winners]
    for m, key in zip(ref_relus, ('bn1', 'bn2')):
        m.view(-1)[torch.from_numpy(fx['tie/%s/idx' % key])] = torch.from_numpy(fx['tie/%s/on' % key])
    for w, key in zip(ref_winners, ('f1', 'f2')):
        w.view(-1)[torch.from_numpy(fx['tie/%s/idx' % key])] = torch.from_numpy(fx['tie/%s/win' % key]).long()
    same = all(torch.equal(a, b) for a, b in zip(relus + winners, ref_relus + ref_winners))
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    pts = torch.from_numpy(fx['pts']).double()
    runs = []
    for rl, wn in ((relus, winners),) if same else ((relus, winners), (ref_relus, ref_winners)):
        ref = _oracle(kind, cfg, fx)
        pre = _hook_embedder(ref.encoder)
        OM.RELU_AT[:], OM.POOL_AT[:] = rl, wn
        try:
            logits = _oracle_logits(kind, ref, pts, keeps)
            assert not OM.RELU_AT and not OM.POOL_AT
        finally:
            OM.RELU_AT.clear(), OM.POOL_AT.clear()
        loss = torch.nn.CrossEntropyLoss()(logits, labels.cpu())
        loss.backward()
        if not runs:
            _assert_near_ties(pre, relus, winners)
        runs.append((logits.detach(), loss.item(),
                     {n: (p.grad.detach() if p.grad is not None else torch.zeros_like(p)) for n, p in ref.named_parameters()}))
    if same:
        return None
    (lp, sp, gp), (lr, sr, gr) = runs
    return lp - lr, sp - sr, {n: gp[n] - gr[n] for n in gp}


@pytest.mark.parametrize('kind', ['linear', 'nonlinear'])
def test_protocol_model_reproduces_reference_fixture(kind):
    """B=4 in train() + set_bn_eval against the live reference: logits, loss, acc, every gradient, the total norm, the
    buffers after the step and the parameters after ONE clipped FlatAdamW(part='only_new') step -- the tolerances of
    test_model_reproduces_reference_fixture (near-ties replayed the same way), the AdamW tolerance of
    test_adamw_gscale_matches_clip_then_torch_adamw for the parameters after the step.  Frozen parameters and the
    buffers of eval-mode BatchNorms keep their bits.  The step starts, on both sides, from the moments of
    tests/golden/moments.py loaded through load_state_dict in torch.optim.AdamW's layout: from zero moments the first
    step is lr * sign(g) wherever |g| is of the size of eps, and where a gradient is analytically zero that sign is the
    reference's rounding noise (moments.py has the reasoning)."""
    from point_dae_amd import finetune_ops as F, patch_embed
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.optim import FlatAdamW
    fx = load_fixture('protocol_%s_b4.npz' % kind)
    model, cfg = _protocol_model(kind, fx)
    assert not model.encoder.first_conv[1].training and model.training
    flat = FlatDataParallel(model)
    flat.zero_grad()
    before = {n: t.detach().clone() for n, t in model.state_dict().items()}
    pts = torch.from_numpy(fx['pts']).cuda()
    labels = torch.from_numpy(fx['labels']).cuda()
    keep = (torch.from_numpy(fx['keep1']).cuda(), torch.from_numpy(fx['keep2']).cuda()) if kind == 'nonlinear' else None
    seen = []
    patch_embed.DECISION_HOOK = lambda d: seen.append({k: v.detach().clone() for k, v in d.items()})
    try:
        logits = flat(pts, drop_keep=keep)
    finally:
        patch_embed.DECISION_HOOK = None
    assert len(seen) == 1
    loss, acc = model.get_loss_acc(logits, labels)
    loss.backward()
    keeps_cpu = [torch.from_numpy(fx[k]).double() for k in ('keep1', 'keep2')] if kind == 'nonlinear' else None
    corr = _tie_correction(kind, cfg, fx, seen[0], labels, keeps_cpu)
    logits, loss = logits.detach(), loss.detach()
    raw_grad = flat.flat_grad.clone()
    if corr is not None:
        d_logits, d_loss, d_grad = corr
        print('tie correction: logits', d_logits.abs().max().item(), 'loss', d_loss)
        logits, loss = logits - d_logits.float().cuda(), loss - d_loss
        for n, p in model.named_parameters():
            p.grad -= d_grad[n].float().cuda()
    print(kind, 'logits rel', _rel(logits, torch.from_numpy(fx['logits'])), 'loss', loss.item(), float(fx['loss']))
    assert _rel(logits, torch.from_numpy(fx['logits'])) <= 1e-5
    assert abs(loss.item() - float(fx['loss'])) <= 1e-5 * abs(float(fx['loss']))
    assert abs(acc.item() - float(fx['acc'])) <= 1e-4
    # a gradient that is zero on both sides up to rounding (a bias in front of the head's training-mode BatchNorm(256))
    zero = [n for n, _ in model.named_parameters() if float(fx['grad/%s/norm' % n]) <= 1e-4]
    print(kind, 'analytically zero gradients', zero)
    assert set(zero) <= {'cls_head_finetune.4.bias'}
    worst = check_grads(_Without(model, zero), fx, 1e-4, 'protocol_%s_b4' % kind)
    for n in zero:
        assert dict(model.named_parameters())[n].grad.double().norm().item() <= 1e-4
    print(kind, 'worst grad err', worst)
    clip = F.GradNormClip(flat.flat_grad, 10.0)
    coef = clip()
    print(kind, 'total norm', clip.norm.item(), float(fx['total_norm']))
    assert abs(clip.norm.item() - float(fx['total_norm'])) <= 1e-5 * float(fx['total_norm'])
    # the step: over the whole flat gradient's coefficient, the optimiser reaching the 'cls' parameters only
    flat.flat_grad.copy_(raw_grad)
    step_grad = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    kw = cfg.optimizer.kwargs
    opt = FlatAdamW(flat, part='only_new', lr=kw.lr, weight_decay=kw.weight_decay)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    state = {}
    for n in (n for names in opt.group_names for n in names):               # torch's ids: group by group
        m, v = fill_moments(n, shapes[n], int(fx['seed']))
        state[len(state)] = {'step': torch.tensor(float(fx['steps_before'])), 'exp_avg': torch.from_numpy(m),
                             'exp_avg_sq': torch.from_numpy(v)}
    opt.load_state_dict({'state': state, 'param_groups': opt.state_dict()['param_groups']})
    assert opt.steps == int(fx['steps_before']) and float(opt.exp_avg_sq.sum()) > 0
    opt.step(grad_scale=clip())
    misses = []
    trained = set(json.loads(str(fx['trained'])))
    assert trained == {n for n, _ in model.named_parameters() if 'cls' in n}
    for n, p in model.named_parameters():
        key = 'param/' + n
        want = fx[key + '/full'] if key + '/full' in fx else fx[key + '/sample']
        got = p.detach().cpu().numpy() if key + '/full' in fx else grad_sample(p)
        if n in trained:                    # (the figures first: the worst element, its gradient here and in the reference)
            err = np.abs(got - want) - 1e-5 * np.abs(want)
            i = int(err.reshape(-1).argmax())
            gkey = 'grad/' + n
            gref = fx[gkey + '/full'] if gkey + '/full' in fx else fx[gkey + '/sample']
            ggot = step_grad[n].cpu().numpy() if gkey + '/full' in fx else grad_sample(step_grad[n])
            print(kind, 'after AdamW', n, 'beyond tolerance', int((err > 1e-6).sum()), 'of', err.size, 'worst |diff|',
                  float(np.abs(got - want).reshape(-1)[i]), 'gradient there', float(ggot.reshape(-1)[i]), 'reference',
                  float(gref.reshape(-1)[i]), 'coef', coef.item())
        if not np.allclose(got, want, rtol=1e-5, atol=1e-6):                    # (asserted at the end, behind the other checks)
            misses.append((n, float(np.abs(got - want).max())))
        if n in trained:
            assert not torch.equal(p, before[n]), n
        else:
            assert torch.equal(p, before[n]), n                             # frozen: bit-equal
    frozen_bn = {n for n, m in model.named_modules()
                 if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and not m.training}
    live_bn = {n for n, m in model.named_modules()
               if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training}
    assert live_bn == ({'cls_head_finetune.5'} if kind == 'nonlinear' else set())
    for bname, b in model.named_buffers():
        if bname not in before:                                                 # (a non-persistent work buffer)
            continue
        if bname.rsplit('.', 1)[0] in frozen_bn:
            assert torch.equal(b, before[bname]), bname                     # eval-mode buffers: bit-equal
        elif bname.rsplit('.', 1)[0] in live_bn and b.dtype.is_floating_point:
            assert not torch.equal(b, before[bname]), bname
        if b.dtype.is_floating_point and 'buf/' + bname in fx:
            assert _rel(b, torch.from_numpy(fx['buf/' + bname])) <= 1e-4, bname
    assert coef.item() <= 1.0
    assert not misses, misses


# ---- graphed step ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['linear', 'nonlinear', 'diff_lr'])
def test_graphed_protocol_step_equals_eager_step_bit_for_bit(kind):
    """test_graphed_classifier_step_equals_eager_step_bit_for_bit for the only_new and diff_lr steps: three replays
    against three eager steps from the same weights and generator states under deterministic reductions."""
    from point_dae_amd import _lib, builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.finetune_ops import GradNormClip
    from point_dae_amd.graph_step import GraphedClassifierStep, use_created_stream
    from point_dae_amd.optim import FlatAdamW
    from point_dae_amd.runner_finetune import set_train_mode, train_step
    from point_dae_amd.synthetic import labelled_clouds
    config = cfg_from_yaml_file(CFGS[kind])
    config.model.depth = 3
    part = config.optimizer.part
    B = 8
    use_created_stream()
    _lib.set_deterministic(True)
    try:
        torch.manual_seed(0)
        net_a = fill_state(builder.model_builder(config.model), 3).cuda()
        net_b = copy.deepcopy(net_a)
        x, y = labelled_clouds(B * 3, 1024, seed=2)
        xs = torch.from_numpy(x).cuda().split(B)
        ys = torch.from_numpy(y).cuda().split(B)
        runs = []
        for net, graphed in ((net_a, False), (net_b, True)):
            model = FlatDataParallel(net)
            set_train_mode(model, part)
            opt, _ = builder.build_opti_sche(model, config)
            assert isinstance(opt, FlatAdamW) and opt.part == part
            model.zero_grad()
            clip = GradNormClip(model.flat_grad, config.grad_norm_clip)
            step = None
            if graphed:
                step = GraphedClassifierStep(model, opt, clip, B, 1024, warmup_eager=0)
                p0, b0 = model.flat_param.clone(), [b.clone() for b in net.buffers()]
                step(xs[0], ys[0])
                model.flat_param.copy_(p0)
                for b, v in zip(net.buffers(), b0):
                    b.copy_(v)
                opt.exp_avg.zero_(), opt.exp_avg_sq.zero_()
                opt.steps = 0
            out = []
            for i in range(3):
                torch.manual_seed(100 + i)
                if graphed:
                    loss, acc = step(xs[i], ys[i])
                else:
                    loss, acc = train_step(model, opt, clip, xs[i], ys[i])
                out.append((loss.item(), acc.item()))
            if graphed:
                assert step.graph is not None
            runs.append((out, model.flat_param.clone(), [b.clone() for b in net.buffers()]))
        (ea, pa, ba), (eb, pb, bb) = runs
        assert ea == eb, (ea, eb)
        assert torch.equal(pa, pb)
        for u, v in zip(ba, bb):
            assert torch.equal(u, v)
    finally:
        _lib.set_deterministic(False)


def test_keep_bn_state_leaves_eval_mode_batchnorms_alone():
    from point_dae_amd.graph_step import _KeepBNState
    net = torch.nn.Sequential(torch.nn.BatchNorm1d(8), torch.nn.BatchNorm1d(8)).cuda().train()
    net[0].eval()
    with _KeepBNState(net):
        for bn in net:
            bn.running_mean.add_(1.0)
    assert float(net[0].running_mean.sum()) == 8.0              # eval mode: not the warm-up pass's to put back
    assert float(net[1].running_mean.sum()) == 0.0


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def _pretrain_ckpt(tmp_path):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_transformer import PointCAE_transformer
    pre = PointCAE_transformer(cfg_from_yaml_file(os.path.join(
        ROOT, 'cfgs', 'pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml')).model)
    pre = fill_state(pre, 9)
    ckpt = tmp_path / 'pretrain.pth'
    torch.save({'base_model': pre.state_dict()}, str(ckpt))
    return ckpt, pre.state_dict()


@pytest.mark.parametrize('kind', ['linear', 'nonlinear', 'diff_lr'])
def test_protocol_cli_runs_a_short_epoch(kind, tmp_path):
    from point_dae_amd.builder import remap_pretrain_keys
    ckpt, pre = _pretrain_ckpt(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'point_dae_amd.main', '--config', CFGS[kind],
           '--finetune_model', '--ckpts', str(ckpt), '--max_epoch', '0', '--steps_per_epoch', '12', '--exp_name', 't']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert 'Successful Loading the ckpt' in out and 'hipGraph replay' in out and '[Validation] EPOCH: 0' in out
    losses = [float(line.split('Loss = ')[1].split()[0]) for line in out.splitlines() if 'Loss = ' in line]
    assert losses and all(np.isfinite(losses)), out
    last = list(tmp_path.glob('experiments/*/cfgs/t/ckpt-last.pth'))
    assert last
    sd = torch.load(str(last[0]), map_location='cpu')
    got = sd['base_model']
    shared = {k: v for k, v in remap_pretrain_keys(pre).items() if k in got}
    assert any(k.startswith('encoder.') for k in shared) and any(k.startswith('blocks.') for k in shared)
    new = [k for k in got if 'cls' in k]
    if kind == 'diff_lr':
        moved = [k for k, v in shared.items() if v.dtype.is_floating_point and not torch.equal(got[k], v)]
        assert any(k.startswith('encoder.first_conv.0') for k in moved) and any(k.startswith('blocks.') for k in moved)
        assert any('running_mean' in k for k in moved)
        assert len(sd['optimizer']['param_groups']) == 4
    else:
        for k, v in shared.items():
            assert torch.equal(got[k], v), k                  # the encoder's parameters AND running statistics
        assert len(sd['optimizer']['param_groups']) == 2
        assert sum(len(g['params']) for g in sd['optimizer']['param_groups']) == len([k for k in new if 'running' not in k
                                                                                     and 'num_batches' not in k])
        assert len(sd['optimizer']['state']) == sum(len(g['params']) for g in sd['optimizer']['param_groups'])


def test_dgcnn_only_new_is_refused_with_the_reason(tmp_path):
    import yaml
    with open(os.path.join(ROOT, 'cfgs', 'finetune_modelnet_dgcnn_smooth.yaml')) as f:
        raw = yaml.safe_load(f)
    raw['optimizer']['part'] = 'only_new'
    for subset in ('train', 'val', 'test'):
        raw['dataset'][subset]['_base_'] = os.path.join(ROOT, raw['dataset'][subset]['_base_'])
    cfg = tmp_path / 'dgcnn_only_new.yaml'
    with open(cfg, 'w') as f:
        yaml.safe_dump(raw, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ['timeout', '-k', '10', '300', sys.executable, '-m', 'point_dae_amd.main', '--config', str(cfg), '--scratch_model',
           '--max_epoch', '0', '--steps_per_epoch', '2', '--exp_name', 't']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode != 0
    assert 'NotImplementedError' in r.stderr and 'bn4' in r.stderr and 'only_new' in r.stderr, r.stderr[-2000:]
