"""Classification fine-tuning on the GPU: every kernel of csrc/finetune.hip and pdae_adamw_step_gscale against an fp64
torch restatement, the PointTransformer model against the live-reference fixture (tests/golden/finetune_cls_b4.npz),
and the fine-tuning CLI end to end in a child process."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import _check_zero_grad_biases, _rel, _Without, check_grads, fill_state, load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features.yaml')


# ---- kernels -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [2, 4, 32, 33, 128])
@pytest.mark.parametrize('T,C', [(65, 384), (2, 4), (65, 4), (2, 384)])
def test_prepend_token_and_cls_max_concat(B, T, C):
    from point_dae_amd import finetune_ops as F
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + C)
    x = torch.randn(B, T - 1, C, generator=g).cuda().requires_grad_()
    tok = torch.randn(1, 1, C, generator=g).cuda().requires_grad_()
    out = F.prepend_token(x, tok)
    want = torch.cat([tok.double().expand(B, -1, -1), x.double()], 1)
    assert torch.equal(out.double(), want)
    d = torch.randn(B, T, C, generator=g).cuda()
    out.backward(d)
    assert torch.equal(x.grad, d[:, 1:])
    assert _rel(tok.grad, d.double()[:, :1].sum(0, keepdim=True)) <= 1e-6

    # cls + max pooling, with a tie: cloud 0 has its maximum of column 1 at t = 1 and t = T - 1 (first one wins)
    y = torch.randn(B, T, C, generator=g)
    if T > 2:
        y[0, T - 1, 1] = y[0, 1, 1] = y[0, :, 1].max() + 1.0
    y = y.cuda().requires_grad_()
    f = F.cls_max_concat(y)
    mx, arg = y.detach()[:, 1:].max(1)
    assert torch.equal(f[:, :C], y.detach()[:, 0]) and torch.equal(f[:, C:], mx)
    dy = torch.randn(B, 2 * C, generator=g).cuda()
    f.backward(dy)
    want = torch.zeros(B, T, C, dtype=torch.float64)
    want[:, 0] = dy[:, :C].double().cpu()
    first = (y.detach()[:, 1:] == mx[:, None]).float().argmax(1).cpu() + 1          # the first maximal t
    want.scatter_(1, first[:, None], dy[:, None, C:].double().cpu())
    assert torch.equal(y.grad.double().cpu(), want)
    if T > 2:
        assert y.grad[0, 1, 1] == dy[0, C + 1] and y.grad[0, T - 1, 1] == 0


@pytest.mark.parametrize('B', [2, 4, 32, 33, 128])
@pytest.mark.parametrize('N', [512, 4, 256])
def test_bn_relu_dropout_matches_batchnorm1d(B, N):
    from point_dae_amd import finetune_ops as F
    g = torch.Generator().manual_seed(B * 7 + N)
    mine = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        mine.weight.copy_(1 + 0.2 * torch.randn(N, generator=g))
        mine.bias.copy_(0.1 * torch.randn(N, generator=g))
        mine.running_mean.copy_(0.1 * torch.randn(N, generator=g))
        mine.running_var.copy_(torch.rand(N, generator=g) + 0.5)
    ref = copy.deepcopy(mine).double().train()
    mine = mine.cuda().train()
    y = (torch.randn(B, N, generator=g) * 2 + 0.3).cuda().requires_grad_()
    keep = torch.rand(B, N, generator=g) >= 0.5
    out = F.bn_relu_dropout(y, mine, 0.5, keep=keep.cuda())
    yr = y.detach().double().cpu().requires_grad_()
    want = torch.relu(ref(yr)) * keep.double() / 0.5
    assert _rel(out, want) <= 1e-5
    d = torch.randn(B, N, generator=g).cuda()
    out.backward(d)
    want.backward(d.double().cpu())
    # dy is a difference of terms of size |gamma invstd dout|; at B = 2 it cancels to ~1e-3 of them, so the bound
    # is taken against that term size rather than against dy itself
    term = float((ref.weight.detach().abs() / (yr.detach().var(0, unbiased=False) + mine.eps).sqrt()).max() * d.abs().max())
    assert float((y.grad.double().cpu() - yr.grad).abs().max()) <= 1e-4 * max(float(yr.grad.abs().max()), 1e-2 * term)
    assert _rel(mine.weight.grad, ref.weight.grad) <= 1e-5
    assert _rel(mine.bias.grad, ref.bias.grad) <= 1e-5
    assert _rel(mine.running_mean, ref.running_mean) <= 1e-6
    assert _rel(mine.running_var, ref.running_var) <= 1e-6
    assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    # a uniform draw: kept where u >= p
    u = torch.rand(B, N, generator=g)
    out2 = F.bn_relu_dropout(y.detach(), mine, 0.5, u=u.cuda())
    with torch.no_grad():
        want2 = torch.relu(ref(y.detach().double().cpu())) * (u >= 0.5).double() / 0.5
    assert _rel(out2, want2) <= 1e-5
    # eval: the running estimates, no dropout, nothing updated
    mine.eval(), ref.eval()
    rm = mine.running_mean.clone()
    out3 = F.bn_relu_dropout(y.detach(), mine, 0.5, u=u.cuda())
    with torch.no_grad():
        want3 = torch.relu(ref(y.detach().double().cpu()))
    assert _rel(out3, want3) <= 1e-5
    assert torch.equal(mine.running_mean, rm)


@pytest.mark.parametrize('B', [2, 4, 32, 33, 128])
@pytest.mark.parametrize('K', [15, 40])
def test_softmax_xent_matches_cross_entropy(B, K):
    from point_dae_amd import finetune_ops as F
    g = torch.Generator().manual_seed(B * 100 + K)
    x = torch.randn(B, K, generator=g) * 3
    labels = torch.randint(0, K, (B,), generator=g)
    x[0, 3] = x[0, 7] = x[0].max() + 1          # a tied row: argmax = 3 (the first)
    labels[0] = 3
    if B > 1:
        x[1, 2] = x[1, 5] = x[1].max() + 1
        labels[1] = 5                           # tie lost: not a hit
    xc = x.cuda().requires_grad_()
    loss, correct = F.softmax_xent(xc, labels.cuda())
    xr = x.double().requires_grad_()
    want = torch.nn.CrossEntropyLoss()(xr, labels)
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()) + 1e-7
    assert correct.item() == float((x.argmax(-1) == labels).sum())
    (2.5 * loss).backward()
    (2.5 * want).backward()
    assert _rel(xc.grad, xr.grad) <= 1e-5


def test_softmax_xent_rejects_too_many_classes():
    from point_dae_amd import finetune_ops as F
    with pytest.raises(RuntimeError, match='status'):
        F.softmax_xent(torch.zeros(4, 65, device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda'))


@pytest.mark.parametrize('n', [5, 1000, 22_600_003])
@pytest.mark.parametrize('max_norm', [10.0, 1e9])
def test_grad_norm_clip_matches_clip_grad_norm(n, max_norm):
    from point_dae_amd import finetune_ops as F
    g = torch.Generator().manual_seed(n)
    flat = (torch.randn(n, generator=g) * 0.01).cuda()
    params = [torch.nn.Parameter(torch.zeros(k, device='cuda')) for k in (n // 3, n // 3, n - 2 * (n // 3))]
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].clone()
        off += p.numel()
    clip = F.GradNormClip(flat, max_norm)
    coef = clip()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    assert abs(clip.norm.item() - total.item()) <= 1e-6 * total.item()
    want = min(1.0, max_norm / (total.item() + 1e-6))
    assert abs(coef.item() - want) <= 1e-6 * want
    clipped = torch.cat([p.grad for p in params])
    assert _rel(flat * coef, clipped) <= 1e-6


def _tiny_net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(37, 64), torch.nn.LayerNorm(64), torch.nn.Linear(64, 13)).cuda()


@pytest.mark.parametrize('max_norm', [0.05, 100.0])
def test_adamw_gscale_matches_clip_then_torch_adamw(max_norm):
    from point_dae_amd import finetune_ops as F
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.optim import FlatAdamW
    net = _tiny_net()
    ref = copy.deepcopy(net)
    model = FlatDataParallel(net)
    opt = FlatAdamW(model, lr=1e-2, weight_decay=0.05)
    clip = F.GradNormClip(model.flat_grad, max_norm)
    decay = [p for n, p in ref.named_parameters() if p.dim() > 1]
    no_decay = [p for n, p in ref.named_parameters() if p.dim() <= 1]
    ropt = torch.optim.AdamW([{'params': no_decay, 'weight_decay': 0.}, {'params': decay, 'weight_decay': 0.05}], lr=1e-2)
    for _ in range(5):
        x = torch.randn(16, 37, device='cuda')
        (model(x) ** 2).mean().backward()
        opt.step(grad_scale=clip())
        opt.zero_grad()
        (ref(x) ** 2).mean().backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        ropt.step()
        ropt.zero_grad()
    for a, b in zip(net.parameters(), ref.parameters()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()


def test_adamw_without_grad_scale_is_bit_equal_to_plain_step():
    from point_dae_amd import _lib
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.optim import FlatAdamW
    net = _tiny_net()
    model = FlatDataParallel(net)
    opt = FlatAdamW(model, lr=1e-2, weight_decay=0.05)
    x = torch.randn(16, 37, device='cuda')
    (model(x) ** 2).mean().backward()
    p0, g0 = model.flat_param.clone(), model.flat_grad.clone()
    opt.step()
    got = model.flat_param.clone()
    # the existing entry, called directly on the same start state
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for grp in opt.param_groups:
        a, b = grp['range']
        if b > a:
            _lib.call('pdae_adamw_step', p, b - a, p[a:].data_ptr(), g0[a:].data_ptr(), m[a:].data_ptr(),
                      v[a:].data_ptr(), float(grp['lr']), 0.9, 0.999, 1e-8, float(grp['weight_decay']), 1)
    assert torch.equal(got, p)
    # and a scale of exactly 1.0 through the new entry gives the same bits
    p2, m2, v2 = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    one = torch.ones(1, device='cuda')
    for grp in opt.param_groups:
        a, b = grp['range']
        if b > a:
            _lib.call('pdae_adamw_step_gscale', p2, b - a, p2[a:].data_ptr(), g0[a:].data_ptr(), m2[a:].data_ptr(),
                      v2[a:].data_ptr(), float(grp['lr']), 0.9, 0.999, 1e-8, float(grp['weight_decay']), 1,
                      one.data_ptr())
    assert torch.equal(got, p2)


# ---- model against the live reference ------------------------------------------------------------------------------

# biases whose gradient is analytically zero: each feeds a training-mode BatchNorm through affine steps and a max-pool
# (a constant shift of a column is removed by the batch mean), and norm.bias shifts every feature of the pooled vector
# the head's first BatchNorm normalises.  Both sides hold rounding noise there (the reference's: norms 6e-8 .. 8e-5);
# they are bounded on their own, against the size of the gradients around them, and left out of the relative checks
ZERO_GRAD = ('encoder.first_conv.0.bias', 'encoder.first_conv.3.bias', 'encoder.second_conv.0.bias', 'norm.bias',
             'cls_head_finetune.0.bias', 'cls_head_finetune.4.bias')


def _model(fx):
    import ast
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_transformer import PointTransformer
    cfg = cfg_from_yaml_file(CFG).model
    for k, v in ast.literal_eval(str(fx['overrides'])):
        cfg[k] = v
    return fill_state(PointTransformer(cfg), int(fx['seed'])).cuda()


def _tie_correction(fx, cfg, decisions, labels):
    """What the product's near-tie decisions in the patch embedder change against the reference's: the fp64 oracle
    run once at the product's own decisions and once at the same decisions with the fixture's recorded near-ties
    (tie/*: every BatchNorm-ReLU input and max-pool gap the reference met within 1e-5 of its channel's largest value)
    set the way the reference took them -> (d logits, d loss, {name: d grad}), None where the two sets agree.  Every
    decision the product takes differently from the oracle must itself be such a near-tie (_assert_near_ties)."""
    from point_dae_amd.point_transformer import PointTransformer
    relus, winners = _embed_decisions(decisions)
    ref_relus, ref_winners = [m.clone() for m in relus], [w.clone() for w in winners]
    for m, key in zip(ref_relus, ('bn1', 'bn2')):
        m.view(-1)[torch.from_numpy(fx['tie/%s/idx' % key])] = torch.from_numpy(fx['tie/%s/on' % key])
    for w, key in zip(ref_winners, ('f1', 'f2')):
        w.view(-1)[torch.from_numpy(fx['tie/%s/idx' % key])] = torch.from_numpy(fx['tie/%s/win' % key]).long()
    same = all(torch.equal(a, b) for a, b in zip(relus + winners, ref_relus + ref_winners))
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    state = fill_state(PointTransformer(cfg), int(fx['seed'])).state_dict()
    pts = torch.from_numpy(fx['pts']).double()
    k1, k2 = torch.from_numpy(fx['keep1']).double(), torch.from_numpy(fx['keep2']).double()
    runs = []
    for rl, wn in ((relus, winners),) if same else ((relus, winners), (ref_relus, ref_winners)):
        ref = _OracleClassifier(cfg)
        ref.load_state_dict(state)
        ref = ref.double().train()
        pre = _hook_embedder(ref.encoder)
        logits, loss = _oracle_at(ref, pts, k1, k2, labels.cpu(), rl, wn)
        loss.backward()
        if not runs:
            _assert_near_ties(pre, relus, winners)
        runs.append((logits.detach(), loss.item(), {n: p.grad.detach() for n, p in ref.named_parameters()}))
    if same:
        return None
    (lp, sp, gp), (lr, sr, gr) = runs
    return lp - lr, sp - sr, {n: gp[n] - gr[n] for n in gp}


def test_model_reproduces_reference_fixture():
    """B=4 against the live reference's fixture: logits, loss, every gradient, the total norm, the BatchNorm buffers and
    eval-mode logits.  Where the product's patch embedder decides a near-tie (a BatchNorm-ReLU input or a max-pool gap
    within 1e-5 of its channel's largest value) otherwise than the reference did, the fp64 oracle's measure of that
    difference (_tie_correction) is taken off the product's logits, loss and gradients first: under the fp32-input
    GEMMs one BatchNorm-ReLU input at 2.9e-8 of its channel's largest value flips and alone moves
    encoder.first_conv.0.weight by 2.5e-4 of its largest entry.  When every near-tie goes the reference's way the
    comparison is the plain one."""
    from point_dae_amd import finetune_ops as F, patch_embed
    fx = load_fixture('finetune_cls_b4.npz')
    model = _model(fx).train()
    pts = torch.from_numpy(fx['pts']).cuda()
    labels = torch.from_numpy(fx['labels']).cuda()
    keep = (torch.from_numpy(fx['keep1']).cuda(), torch.from_numpy(fx['keep2']).cuda())
    seen = []
    patch_embed.DECISION_HOOK = lambda d: seen.append({k: v.detach().clone() for k, v in d.items()})
    try:
        logits = model(pts, drop_keep=keep)
    finally:
        patch_embed.DECISION_HOOK = None
    assert len(seen) == 1
    loss, acc = model.get_loss_acc(logits, labels)
    loss.backward()
    import ast
    from point_dae_amd.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(CFG).model
    for k, v in ast.literal_eval(str(fx['overrides'])):
        cfg[k] = v
    corr = _tie_correction(fx, cfg, seen[0], labels)
    logits, loss = logits.detach(), loss.detach()
    if corr is not None:
        d_logits, d_loss, d_grad = corr
        print('tie correction: logits', d_logits.abs().max().item(), 'loss', d_loss)
        logits, loss = logits - d_logits.float().cuda(), loss - d_loss
        for n, p in model.named_parameters():
            p.grad -= d_grad[n].float().cuda()
    print('logits rel', _rel(logits, torch.from_numpy(fx['logits'])), 'loss', loss.item(), float(fx['loss']))
    assert _rel(logits, torch.from_numpy(fx['logits'])) <= 1e-5
    assert abs(loss.item() - float(fx['loss'])) <= 1e-5 * abs(float(fx['loss']))
    assert abs(acc.item() - float(fx['acc'])) <= 1e-4
    worst = check_grads(_Without(model, ZERO_GRAD), fx, 1e-4, 'finetune_cls_b4')
    _check_zero_grad_biases(model, {n: float(fx['grad/%s/norm' % n]) for n in ZERO_GRAD})
    print('worst grad err', worst)
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    clip = F.GradNormClip(flat, 10.0)
    clip()
    assert abs(clip.norm.item() - float(fx['total_norm'])) <= 1e-5 * float(fx['total_norm'])
    for bname, b in model.named_buffers():
        if b.dtype.is_floating_point and 'buf/' + bname in fx:
            assert _rel(b, torch.from_numpy(fx['buf/' + bname])) <= 1e-4, bname
    model.eval()
    with torch.no_grad():
        ev = model(pts)
    assert _rel(ev, torch.from_numpy(fx['eval_logits'])) <= 1e-5


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def test_finetune_cli_trains_from_a_pretraining_checkpoint(tmp_path):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_transformer import PointCAE_transformer
    pre = PointCAE_transformer(cfg_from_yaml_file(os.path.join(
        ROOT, 'cfgs', 'pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml')).model)
    ckpt = tmp_path / 'pretrain.pth'
    torch.save({'base_model': pre.state_dict()}, str(ckpt))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'point_dae_amd.main', '--config', CFG, '--finetune_model',
           '--ckpts', str(ckpt), '--max_epoch', '1', '--steps_per_epoch', '20', '--exp_name', 't']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert 'Successful Loading the ckpt' in out
    assert '[Validation] EPOCH: 0' in out and '[Validation] EPOCH: 1' in out
    losses = [float(line.split('Loss = ')[1].split()[0]) for line in out.splitlines() if 'Loss = ' in line]
    assert len(losses) == 2 and all(np.isfinite(losses)), out
    assert losses[1] < losses[0], losses
    assert list(tmp_path.glob('experiments/*/cfgs/t/ckpt-last.pth'))


def test_finetune_cli_epoch_with_a_one_cloud_tail_drops_it(tmp_path):
    """2 total_bs + 1 training clouds: the train loader drops the one-cloud tail, as the reference's drop_last does (a
    B = 1 training step would reach bn_relu_dropout, which refuses one row in training mode), so the epoch runs its two
    full batches; validation still scores every test cloud, the last batch of one included."""
    import yaml
    with open(CFG) as f:
        raw = yaml.safe_load(f)
    count = 2 * raw['total_bs'] + 1
    for subset in ('train', 'val', 'test'):
        node = raw['dataset'][subset]
        node['_base_'] = os.path.join(ROOT, node['_base_'])
        node['others']['count'] = count
    cfg = tmp_path / 'tail.yaml'
    with open(cfg, 'w') as f:
        yaml.safe_dump(raw, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'point_dae_amd.main', '--config', str(cfg),
           '--scratch_model', '--max_epoch', '0', '--exp_name', 't']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert '[Epoch 0/0][Batch 2/2]' in out, out
    assert '[Batch 3/' not in out, out
    losses = [float(line.split('Loss = ')[1].split()[0]) for line in out.splitlines() if 'Loss = ' in line]
    assert len(losses) == 1 and all(np.isfinite(losses)), out
    assert '[Validation] EPOCH: 0' in out


# ---- full size against the CPU oracle --------------------------------------------------------------------------------

class _OracleClassifier(torch.nn.Module):
    """PointTransformer restated on the CPU from oracle.model pieces plus a torch head; same attribute names as the
    product model, so the weights move by state_dict.  Dropout takes injected keep masks."""

    def __init__(self, cfg):
        super().__init__()
        from oracle import model as OM
        C = cfg.trans_dim
        self.G, self.k = cfg.num_group, cfg.group_size
        self.encoder = OM.Encoder(cfg.encoder_dims)
        self.cls_token = torch.nn.Parameter(torch.zeros(1, 1, C))
        self.cls_pos = torch.nn.Parameter(torch.zeros(1, 1, C))
        self.pos_embed = OM._pos_embed(C)
        self.blocks = OM.TransformerEncoder(C, cfg.depth, cfg.num_heads, [0.0] * cfg.depth)
        self.norm = torch.nn.LayerNorm(C)
        self.cls_head_finetune = torch.nn.Sequential(
            torch.nn.Linear(2 * C, 512), torch.nn.BatchNorm1d(512), torch.nn.ReLU(), torch.nn.Dropout(0.5),
            torch.nn.Linear(512, 256), torch.nn.BatchNorm1d(256), torch.nn.ReLU(), torch.nn.Dropout(0.5),
            torch.nn.Linear(256, cfg.cls_dim))

    def forward(self, pts, keep1, keep2):
        from oracle import model as OM
        nb, center = OM.group_divider(pts.float(), self.G, self.k)          # (the geometry oracle takes fp32)
        nb, center = nb.to(self.cls_token.dtype), center.to(self.cls_token.dtype)
        B = pts.shape[0]
        tok = self.encoder(nb)
        x = torch.cat([self.cls_token.expand(B, -1, -1), tok], 1)
        pos = torch.cat([self.cls_pos.expand(B, -1, -1), self.pos_embed(center)], 1)
        x = self.norm(self.blocks(x, pos))
        f = torch.cat([x[:, 0], x[:, 1:].max(1)[0]], -1)
        h = self.cls_head_finetune
        f = torch.relu(h[1](h[0](f))) * keep1 / 0.5
        f = torch.relu(h[5](h[4](f))) * keep2 / 0.5
        return h[8](f)


def _embed_decisions(d, n=32):
    """The patch embedder's decisions (patch_embed.DECISION_HOOK) in the oracle's layout: the two BatchNorm-ReLU masks
    as (groups, C, n) booleans, the two max-pool winners as (groups, C) int64 -- on the CPU."""
    def mask(y, sc, sh):
        return ((y * sc + sh) > 0).view(-1, n, y.shape[1]).permute(0, 2, 1).contiguous().cpu()
    return ([mask(d['y1'], d['sc1'], d['sh1']), mask(d['h3'], d['sc2'], d['sh2'])],
            [d['arg2'].long().cpu(), d['arg4'].long().cpu()])


def _hook_embedder(enc):
    """Forward hooks on the oracle Encoder's BatchNorm outputs and pre-pool activations -> the dict they fill."""
    pre = {}
    # (a clone: the un-injected ReLU runs in place on the BatchNorm's output)
    pre['hooks'] = [mod.register_forward_hook(lambda m, i, o, key=key: pre.update({key: o.detach().clone()}))
                    for key, mod in (('bn1', enc.first_conv[1]), ('f1', enc.first_conv[3]),
                                     ('bn2', enc.second_conv[1]), ('f2', enc.second_conv[3]))]
    return pre


def _assert_near_ties(pre, relus, winners, rel=1e-5):
    """Every replayed decision that differs from the oracle's own is a near-tie on the oracle's side: a BatchNorm-ReLU
    input within `rel` of its channel's largest |value|, a pool winner within `rel` of that channel's maximum."""
    for key, m in zip(('bn1', 'bn2'), relus):
        v = pre[key]
        assert m.shape == v.shape, (key, m.shape, v.shape)
        scale = v.abs().amax(dim=(0, 2), keepdim=True)
        off = m != (v > 0)
        gap = (v.abs() / scale)[off].max().item() if off.any() else 0.0
        print(key, 'ReLU decisions differing from the fp64 oracle', int(off.sum()), 'largest |x| / channel max', gap)
        assert gap <= rel, (key, int(off.sum()), gap)
    for key, w in zip(('f1', 'f2'), winners):
        v = pre[key]
        assert w.shape == v.shape[:2] and int(w.max()) < v.shape[2], (key, w.shape, v.shape)
        top, at = v.amax(2), v.gather(2, w.unsqueeze(-1)).squeeze(-1)
        scale = v.abs().amax(dim=(0, 2)).clamp_min(1e-30).view(1, -1)
        gap = ((top - at) / scale).max().item()
        print(key, 'pool winners differing in value', int((at != top).sum()), 'largest gap / channel max', gap)
        assert gap <= rel, (key, gap)


def _oracle_at(ref, pts, k1, k2, labels, relus, winners):
    """The oracle's forward with the embedder's decisions replayed (oracle/model.py RELU_AT, POOL_AT) -> logits, loss."""
    from oracle import model as OM
    OM.RELU_AT[:], OM.POOL_AT[:] = relus, winners
    try:
        logits = ref(pts, k1, k2)
        assert not OM.RELU_AT and not OM.POOL_AT                  # the Encoder consumed every decision
    finally:
        OM.RELU_AT.clear(), OM.POOL_AT.clear()
    return logits, torch.nn.CrossEntropyLoss()(logits, labels)


def test_full_batch_b32_loss_and_gradients_equal_the_oracle():
    """B=32, N=1024, G=64 (T=65 tokens), depth 12: the loss within 1e-5 and every gradient within 1e-3 relative L2 of
    the CPU restatement, run in fp64, on the same weights and the same dropout masks (stochastic depth off on both sides).

    The patch embedder's discrete decisions -- its two BatchNorm-ReLUs over 8 M and 33 M entries and its two max-pools
    -- are the product's own, replayed in the oracle (oracle/model.py RELU_AT, POOL_AT): at this seed the oracle's own
    fp32 run flips 8 ReLU entries within 7e-7 of zero and one pool winner 1.1e-7 apart against its fp64 run, and those
    alone move its encoder gradients by 1.2e-3 (with the fp64 decisions replayed it is at 7e-6).  Every decision the
    product takes differently from the un-injected fp64 oracle must be such a near-tie, and the injected oracle's loss
    must equal the un-injected one's."""
    from point_dae_amd import patch_embed
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_transformer import PointTransformer
    from point_dae_amd.synthetic import shapenet_like_clouds
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cfg = cfg_from_yaml_file(CFG).model
    cfg.drop_path_rate = 0.0
    B = 32
    mine = fill_state(PointTransformer(cfg), 11)
    ref = _OracleClassifier(cfg)
    ref.load_state_dict(mine.state_dict())
    mine, ref = mine.cuda().train(), ref.double().train()
    rng = np.random.default_rng(3)
    pts = shapenet_like_clouds(B, 1024, seed=13)
    labels = torch.from_numpy(rng.integers(0, cfg.cls_dim, B))
    k1, k2 = torch.from_numpy(rng.random((B, 512)) >= 0.5), torch.from_numpy(rng.random((B, 256)) >= 0.5)
    seen = []
    patch_embed.DECISION_HOOK = lambda d: seen.append({k: v.detach().clone() for k, v in d.items()})
    try:
        loss_m, _ = mine.get_loss_acc(mine(torch.from_numpy(pts).cuda(), drop_keep=(k1.cuda(), k2.cuda())),
                                      labels.cuda())
    finally:
        patch_embed.DECISION_HOOK = None
    loss_m.backward()
    assert len(seen) == 1
    relus, winners = _embed_decisions(seen[0])

    # the oracle's own decisions, and the values they are taken on: BatchNorm outputs and pre-pool activations
    pre = _hook_embedder(ref.encoder)
    with torch.no_grad():
        loss_r = torch.nn.CrossEntropyLoss()(ref(torch.from_numpy(pts).double(), k1.double(), k2.double()), labels)
    _assert_near_ties(pre, relus, winners)
    for h in pre.pop('hooks'):
        h.remove()

    _, loss_i = _oracle_at(ref, torch.from_numpy(pts).double(), k1.double(), k2.double(), labels, relus, winners)
    loss_i.backward()
    assert abs(loss_i.item() - loss_r.item()) <= 1e-5 * abs(loss_r.item()), (loss_i.item(), loss_r.item())
    assert abs(loss_m.item() - loss_r.item()) <= 1e-5 * abs(loss_r.item()), (loss_m.item(), loss_r.item())
    gr = dict(ref.named_parameters())
    worst = (0.0, '')
    for n, p in mine.named_parameters():
        if n in ZERO_GRAD:
            continue
        a, b = p.grad.double().cpu(), gr[n].grad.double()
        worst = max(worst, (float((a - b).norm() / b.norm()), n))
    print('worst rel-L2', worst)
    assert worst[0] <= 1e-3, worst
    _check_zero_grad_biases(mine, {n: gr[n].grad.double().norm().item() for n in ZERO_GRAD})


# ---- graphed step ----------------------------------------------------------------------------------------------------

def test_graphed_classifier_step_equals_eager_step_bit_for_bit():
    """Three steps replayed from one captured graph (forward, loss, backward, clip coefficient) against three eager
    steps from the same weights and generator states under deterministic reductions: losses, accuracies and every
    parameter after AdamW equal bit for bit.  The capture itself proves the captured region has no host sync."""
    from point_dae_amd import _lib, builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.finetune_ops import GradNormClip
    from point_dae_amd.graph_step import GraphedClassifierStep, use_created_stream
    from point_dae_amd.runner_finetune import train_step
    from point_dae_amd.synthetic import labelled_clouds
    config = cfg_from_yaml_file(CFG)
    config.model.depth = 3
    B = 8
    use_created_stream()
    _lib.set_deterministic(True)
    try:
        torch.manual_seed(0)
        net_a = builder.model_builder(config.model).cuda().train()
        net_b = copy.deepcopy(net_a)
        x, y = labelled_clouds(B * 3, 1024, seed=2)
        xs = torch.from_numpy(x).cuda().split(B)
        ys = torch.from_numpy(y).cuda().split(B)
        runs = []
        for net, graphed in ((net_a, False), (net_b, True)):
            model = FlatDataParallel(net)
            opt, _ = builder.build_opti_sche(model, config)
            model.zero_grad()
            clip = GradNormClip(model.flat_grad, config.grad_norm_clip)
            step = None
            if graphed:
                # capture once (its eager warm-up pass draws from the generator too), then put the start state back:
                # the three compared steps are replays that begin from the eager run's weights and generator states
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


# ---- data path -------------------------------------------------------------------------------------------------------

def test_resample_takes_npoints_of_the_point_all_fps_points():
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    from point_dae_amd.runner_finetune import resample
    from point_dae_amd.synthetic import labelled_clouds
    x, _ = labelled_clouds(3, 2048, seed=4)
    xd = torch.from_numpy(x).cuda()
    choice = np.random.default_rng(0).choice(1200, 1024, False)
    out = resample(xd, 1024, choice)
    fps = furthest_point_sample(xd, 1200).long()
    want = torch.gather(xd, 1, fps[:, torch.from_numpy(choice).cuda()][..., None].expand(-1, -1, 3))
    assert out.shape == (3, 1024, 3) and torch.equal(out, want)


def test_modelnet_train_augmentation_norm_scale_translate():
    from point_dae_amd.datasets import ModelNet
    base = dict(NAME='ModelNet', NUM_CATEGORY=40, npoints=512, bs=4, count=8, subset='train', seed=1)
    plain = ModelNet(dict(base))
    clean = ModelNet(dict(base, aug_type=['clean']))
    aug = ModelNet(dict(base, aug_type=['norm', 'scale', 'translate']))
    for (_, _, (a, la)), (_, _, (b, lb)), (_, _, (c, lc)) in zip(plain, clean, aug):
        assert torch.equal(a, b) and torch.equal(la, lc)
        # per cloud an anisotropic scale in [2/3, 3/2] and a shift in [-0.2, 0.2] of the normalised cloud
        ca, cc = a.mean(1), c.mean(1)
        s = (c - cc[:, None]).abs().amax(1) / (a - ca[:, None]).abs().amax(1)
        assert not torch.equal(a, c)
        assert bool(((s > 0.6) & (s < 1.6)).all()), s
        assert bool(((cc - ca).abs() <= 0.2 + 1e-3).all()), cc - ca
