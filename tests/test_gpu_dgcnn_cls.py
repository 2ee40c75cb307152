"""DGCNN classifier fine-tuning on the GPU: the LeakyReLU head glue and the label-smoothed cross-entropy of
csrc/finetune.hip against fp64 torch, the DGCNN model against the live-reference fixture (tests/golden/dgcnn_cls_b4.npz),
the head and loss at B=32 against an fp64 restatement, the graphed step against the eager step, and the CLI end to end
in a child process."""
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
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_dgcnn_smooth.yaml')


def _smooth_target(labels, K, eps):
    """The reference's target (PointCAE_DGCNN.py:595-597), fp64."""
    one_hot = torch.zeros(labels.shape[0], K, dtype=torch.float64).scatter(1, labels.view(-1, 1), 1)
    return one_hot * (1 - eps) + (1 - one_hot) * eps / (K - 1)


def _smooth_loss(logits, labels, eps):
    return -(_smooth_target(labels, logits.shape[1], eps) * torch.log_softmax(logits, 1)).sum(1).mean()


# ---- kernels -----------------------------------------------------------------------------------------------------------

def _bn_pair(N, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(N, generator=g))
        bn.bias.copy_(0.1 * torch.randn(N, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(N, generator=g))
        bn.running_var.copy_(torch.rand(N, generator=g) + 0.5)
    return bn, g


@pytest.mark.parametrize('slope', [0.2, 0.0])
@pytest.mark.parametrize('B', [2, 32, 100])
@pytest.mark.parametrize('N', [256, 512])
def test_bn_lrelu_dropout_matches_batchnorm1d(B, N, slope):
    from point_dae_amd import finetune_ops as F
    mine, g = _bn_pair(N, B * 7 + N)
    ref = copy.deepcopy(mine).double().train()
    mine = mine.cuda().train()
    y = (torch.randn(B, N, generator=g) * 2 + 0.3).cuda().requires_grad_()
    keep = torch.rand(B, N, generator=g) >= 0.5
    out = F.bn_lrelu_dropout(y, mine, 0.5, slope, keep=keep.cuda())
    yr = y.detach().double().cpu().requires_grad_()
    want = torch.nn.functional.leaky_relu(ref(yr), slope) * keep.double() / 0.5
    assert _rel(out, want) <= 1e-5
    d = torch.randn(B, N, generator=g).cuda()
    out.backward(d)
    want.backward(d.double().cpu())
    # dy is a difference of terms of size |gamma invstd dout| (it cancels at B = 2): bounded against that term size
    term = float((ref.weight.detach().abs() / (yr.detach().var(0, unbiased=False) + mine.eps).sqrt()).max() * d.abs().max())
    assert float((y.grad.double().cpu() - yr.grad).abs().max()) <= 1e-4 * max(float(yr.grad.abs().max()), 1e-2 * term)
    assert _rel(mine.weight.grad, ref.weight.grad) <= 1e-5
    assert _rel(mine.bias.grad, ref.bias.grad) <= 1e-5
    assert _rel(mine.running_mean, ref.running_mean) <= 1e-6
    assert _rel(mine.running_var, ref.running_var) <= 1e-6
    assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    # no dropout (the head's first block): p = 0 and no draw
    out1 = F.bn_lrelu_dropout(y.detach(), mine, 0.0, slope)
    with torch.no_grad():
        want1 = torch.nn.functional.leaky_relu(ref(y.detach().double().cpu()), slope)
    assert _rel(out1, want1) <= 1e-5
    # a uniform draw: kept where u >= p
    u = torch.rand(B, N, generator=g)
    out2 = F.bn_lrelu_dropout(y.detach(), mine, 0.5, slope, u=u.cuda())
    with torch.no_grad():
        want2 = torch.nn.functional.leaky_relu(ref(y.detach().double().cpu()), slope) * (u >= 0.5).double() / 0.5
    assert _rel(out2, want2) <= 1e-5
    # eval: the running estimates, no dropout, nothing updated
    mine.eval(), ref.eval()
    rm, nbt = mine.running_mean.clone(), int(mine.num_batches_tracked)
    out3 = F.bn_lrelu_dropout(y.detach(), mine, 0.5, slope, u=u.cuda())
    with torch.no_grad():
        want3 = torch.nn.functional.leaky_relu(ref(y.detach().double().cpu()), slope)
    assert _rel(out3, want3) <= 1e-5
    assert torch.equal(mine.running_mean, rm) and int(mine.num_batches_tracked) == nbt


@pytest.mark.parametrize('B', [2, 32, 100])
@pytest.mark.parametrize('N', [256, 512])
def test_bn_lrelu_dropout_at_slope_zero_is_bn_relu_dropout_bit_for_bit(B, N):
    from point_dae_amd import finetune_ops as F
    a, g = _bn_pair(N, B * 11 + N)
    b = copy.deepcopy(a)
    a, b = a.cuda().train(), b.cuda().train()
    y0 = torch.randn(B, N, generator=g) * 2 + 0.3
    y0[0, :8] = 0.0                                   # exact zeros and negatives on the kink
    keep = (torch.rand(B, N, generator=g) >= 0.5).cuda()
    d = torch.randn(B, N, generator=g).cuda()
    outs = []
    for bn, fn in ((a, lambda y, bn: F.bn_lrelu_dropout(y, bn, 0.5, 0.0, keep=keep)),
                   (b, lambda y, bn: F.bn_relu_dropout(y, bn, 0.5, keep=keep))):
        y = y0.clone().cuda().requires_grad_()
        out = fn(y, bn)
        out.backward(d)
        outs.append((out.detach(), y.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))
    for u, v in zip(*outs):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))        # the bits, signed zeros included
    a.eval(), b.eval()
    e1 = F.bn_lrelu_dropout(y0.cuda(), a, 0.5, 0.0)
    e2 = F.bn_relu_dropout(y0.cuda(), b, 0.5)
    assert torch.equal(e1.view(torch.int32), e2.view(torch.int32))


def test_bn_lrelu_dropout_refuses_one_row_in_training_mode():
    from point_dae_amd import finetune_ops as F
    bn = torch.nn.BatchNorm1d(16).cuda().train()
    with pytest.raises(RuntimeError, match='B >= 2'):
        F.bn_lrelu_dropout(torch.randn(1, 16, device='cuda'), bn, 0.0, 0.2)
    assert int(bn.num_batches_tracked) == 0
    bn.eval()                                          # eval mode takes a single row
    out = F.bn_lrelu_dropout(torch.randn(1, 16, device='cuda'), bn, 0.0, 0.2)
    assert out.shape == (1, 16)
    with pytest.raises(ValueError, match='slope'):
        F.bn_lrelu_dropout(torch.randn(4, 16, device='cuda'), bn, 0.0, 1.5)


@pytest.mark.parametrize('eps', [0.0, 0.3])
@pytest.mark.parametrize('K', [2, 15, 40, 64])
@pytest.mark.parametrize('B', [2, 32, 33])
def test_softmax_xent_smooth_matches_torch_formula(B, K, eps):
    from point_dae_amd import finetune_ops as F
    g = torch.Generator().manual_seed(B * 100 + K + int(eps * 10))
    x = torch.randn(B, K, generator=g) * 3
    labels = torch.randint(0, K, (B,), generator=g)
    x[0, 0] = x[0, K - 1] = x[0].max() + 1          # a tied row: argmax = 0 (the first)
    labels[0] = 0
    x[1, 0] = x[1, 1] = x[1].max() + 1
    labels[1] = 1                                   # tie lost: not a hit
    xc = x.cuda().requires_grad_()
    loss, correct = F.softmax_xent_smooth(xc, labels.cuda(), eps)
    xr = x.double().requires_grad_()
    want = _smooth_loss(xr, labels, eps)
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()) + 1e-7, (loss.item(), want.item())
    assert correct.item() == float((x.argmax(-1) == labels).sum())
    (2.5 * loss).backward()
    (2.5 * want).backward()
    assert _rel(xc.grad, xr.grad) <= 1e-5
    # the gradient is (softmax - t) dloss / B
    t = _smooth_target(labels, K, eps)
    assert _rel(xc.grad, (torch.softmax(x.double(), 1) - t) * 2.5 / B) <= 1e-5
    if eps == 0.0:
        # eps = 0 is the plain cross-entropy: softmax_xent's bits
        xp = x.cuda().requires_grad_()
        lp, cp = F.softmax_xent(xp, labels.cuda())
        (2.5 * lp).backward()
        assert torch.equal(loss.detach(), lp.detach()) and torch.equal(correct, cp)
        assert torch.equal(xc.grad, xp.grad)


def test_softmax_xent_smooth_refuses_unsupported_class_counts_and_flags_bad_labels():
    from point_dae_amd import finetune_ops as F
    lab = torch.zeros(4, dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match='status'):
        F.softmax_xent_smooth(torch.zeros(4, 65, device='cuda'), lab, 0.3)
    with pytest.raises(RuntimeError, match='status'):
        F.softmax_xent_smooth(torch.zeros(4, 1, device='cuda'), lab, 0.3)
    with pytest.raises(ValueError, match='eps'):
        F.softmax_xent_smooth(torch.zeros(4, 8, device='cuda'), lab, -0.1)
    loss, _ = F.softmax_xent_smooth(torch.zeros(4, 8, device='cuda'), torch.tensor([0, 1, 8, 2], device='cuda'), 0.3)
    assert torch.isnan(loss).item()


# ---- model against the live reference ------------------------------------------------------------------------------

# biases whose gradient is analytically zero: the head's two Linear biases feed a training-mode BatchNorm1d directly, and
# a constant shift of a column is removed by the batch mean; bn5.bias shifts a feature column by the same amount in
# every cloud while the pooled winners sit on LeakyReLU's positive side (the fixture's fp64 gradient there is ~1e-15),
# and the head's first BatchNorm removes that too.  Both sides hold rounding noise there (the reference's norms:
# 4e-7 .. 5e-7); they are bounded on their own and left out of the relative checks
ZERO_GRAD = ('cls_head_finetune.0.bias', 'cls_head_finetune.3.bias', 'dgcnn_encoder.bn5.bias')


def _model(seed):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.dgcnn_cls import DGCNN
    return fill_state(DGCNN(cfg_from_yaml_file(CFG).model), seed).cuda()


def test_model_reproduces_reference_fixture():
    from point_dae_amd import _lib, finetune_ops as F
    fx = load_fixture('dgcnn_cls_b4.npz')
    model = _model(int(fx['seed'])).train()
    pts = torch.from_numpy(fx['pts']).cuda()
    labels = torch.from_numpy(fx['labels']).cuda()
    cap = {}
    logits = model(pts, drop_keep=torch.from_numpy(fx['keep']).cuda(), capture=cap)
    loss, acc = model.get_loss_acc(logits, labels)
    model.smoothing = False
    loss_plain, _ = model.get_loss_acc(logits.detach(), labels)
    model.smoothing = True
    loss.backward()
    print('feature rel', _rel(cap['feature'], torch.from_numpy(fx['feature'])), 'logits rel',
          _rel(logits, torch.from_numpy(fx['logits'])), 'loss', loss.item(), float(fx['loss']),
          'plain', loss_plain.item(), float(fx['loss_plain']))
    # (the fixture's seed is one where the reference's fp32 and fp64 runs agree: no encoder decision within rounding)
    assert _rel(cap['feature'], torch.from_numpy(fx['feature'])) <= 1e-5
    assert _rel(logits, torch.from_numpy(fx['logits'])) <= 1e-5
    assert abs(loss.item() - float(fx['loss'])) <= 1e-5 * abs(float(fx['loss']))
    assert abs(loss_plain.item() - float(fx['loss_plain'])) <= 1e-5 * abs(float(fx['loss_plain']))
    assert abs(acc.item() - float(fx['acc'])) <= 1e-4
    # The reference's own fp32 and fp64 gradients agree to 2e-5 on this fixture; the default arithmetic stays within
    # 1e-4 (6.5e-5 measured).  Under PDAE_GEMM=f32mfma, whose products sit further from the fp64 ones, an edge winner
    # whose pre-activation is within rounding of LeakyReLU's kink takes slope 1 on one side and 0.2 on the other and
    # moves single entries of the layers below it (test_gpu_model.py, the DGCNN fixtures): seven tensors of conv1-3 /
    # bn1-2 miss 3e-3 there, the largest bn2.bias entry by 1.7e-2 of its maximum, and the total norm moves by 1.3e-4.
    # That mode gets the `spike` allowance; the L2 norms keep 3e-3
    if _lib.gemm_arith() == _lib.GEMM_F32MFMA:
        worst = check_grads(_Without(model, ZERO_GRAD), fx, 3e-3, 'dgcnn_cls_b4', spike=5e-2, max_spikes=8)
        norm_rtol = 1e-3
    else:
        worst = check_grads(_Without(model, ZERO_GRAD), fx, 1e-4, 'dgcnn_cls_b4')
        norm_rtol = 1e-5
    _check_zero_grad_biases(model, {n: float(fx['grad/%s/norm' % n]) for n in ZERO_GRAD})
    print('worst grad err', worst)
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    clip = F.GradNormClip(flat, 10.0)
    clip()
    print('total norm', clip.norm.item(), float(fx['total_norm']))
    assert abs(clip.norm.item() - float(fx['total_norm'])) <= norm_rtol * float(fx['total_norm'])
    for bname, b in model.named_buffers():
        if b.dtype.is_floating_point and 'buf/' + bname in fx:
            assert _rel(b, torch.from_numpy(fx['buf/' + bname])) <= 1e-4, bname
    model.eval()
    with torch.no_grad():
        ev = model(pts)
    print('eval logits rel', _rel(ev, torch.from_numpy(fx['eval_logits'])))
    assert _rel(ev, torch.from_numpy(fx['eval_logits'])) <= 1e-5


class _Head64(torch.nn.Module):
    """cls_head_finetune restated in fp64 torch (PointCAE_DGCNN.py:579-588), the Dropout on an injected keep mask."""

    def __init__(self, head):
        super().__init__()
        self.h = copy.deepcopy(head).cpu().double().train()

    def forward(self, f, keep):
        h = self.h
        x = torch.nn.functional.leaky_relu(h[1](h[0](f)), 0.2)
        x = torch.nn.functional.leaky_relu(h[4](h[3](x)), 0.2) * keep / 0.5
        return h[7](x)


def test_full_batch_b32_head_and_loss_equal_fp64_restatement():
    """B=32, N=1024: the product's own encoder feature through the head and the smoothed loss, against fp64 torch on the
    same feature, weights and keep mask: logits, loss, every head gradient, d(feature) and the head's running estimates."""
    from point_dae_amd.synthetic import shapenet_like_clouds
    B = 32
    model = _model(11).train()
    ref = _Head64(model.cls_head_finetune)
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(shapenet_like_clouds(B, 1024, seed=13)).cuda()
    labels = torch.from_numpy(rng.integers(0, model.cls_dim, B))
    keep = torch.from_numpy(rng.random((B, 256)) >= 0.5)
    cap = {}
    logits = model(pts, drop_keep=keep.cuda(), capture=cap)
    feat = cap['feature']
    feat.retain_grad()
    loss, acc = model.get_loss_acc(logits, labels.cuda())
    loss.backward()
    fr = feat.detach().double().cpu().requires_grad_()
    want_logits = ref(fr, keep.double())
    want = _smooth_loss(want_logits, labels, 0.3)
    want.backward()
    print('logits rel', _rel(logits, want_logits), 'loss', loss.item(), want.item())
    assert _rel(logits, want_logits) <= 1e-5
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    assert acc.item() == 100.0 * float((want_logits.argmax(-1) == labels).sum()) / B
    assert _rel(feat.grad, fr.grad) <= 1e-4, _rel(feat.grad, fr.grad)
    gr = dict(ref.h.named_parameters())
    worst = (0.0, '')
    for n, p in model.cls_head_finetune.named_parameters():
        if 'cls_head_finetune.' + n in ZERO_GRAD:
            continue
        a, b = p.grad.double().cpu(), gr[n].grad
        worst = max(worst, (float((a - b).norm() / b.norm()), n))
    print('worst head rel-L2', worst)
    assert worst[0] <= 1e-4, worst
    _check_zero_grad_biases(model, {n: gr[n[len('cls_head_finetune.'):]].grad.norm().item() for n in ZERO_GRAD
                                    if n.startswith('cls_head_finetune.')})
    for n, b in model.cls_head_finetune.named_buffers():
        if b.dtype.is_floating_point:
            assert _rel(b, dict(ref.h.named_buffers())[n]) <= 1e-5, n


# ---- graphed step ----------------------------------------------------------------------------------------------------

def test_graphed_classifier_step_equals_eager_step_bit_for_bit():
    """Three steps of DGCNN replayed from one captured graph (forward, smoothed loss, backward, clip coefficient)
    against three eager steps from the same weights and generator states under deterministic reductions: losses,
    accuracies, every parameter after AdamW and the BatchNorm running estimates equal bit for bit."""
    from point_dae_amd import _lib, builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.finetune_ops import GradNormClip
    from point_dae_amd.graph_step import GraphedClassifierStep, use_created_stream
    from point_dae_amd.runner_finetune import train_step
    from point_dae_amd.synthetic import labelled_clouds
    config = cfg_from_yaml_file(CFG)
    B = 8
    use_created_stream()
    was_deterministic = _lib.deterministic()
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
                # capture once (its eager warm-up pass draws from the generator too), then put the start state back
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
        assert all(np.isfinite(v[0]) for v in ea)
        assert torch.equal(pa, pb)
        for u, v in zip(ba, bb):
            assert torch.equal(u, v)
    finally:
        _lib.set_deterministic(was_deterministic)       # (a PDAE_DETERMINISTIC=1 suite stays deterministic)


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def _autoencoder_ckpt(path):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_dgcnn import Point_CAE_DGCNN_FCOnly
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'pretrain_PointCAE_clean.yaml')).model
    cfg.NAME = 'Point_CAE_DGCNN_FCOnly'
    torch.manual_seed(0)
    torch.save({'base_model': Point_CAE_DGCNN_FCOnly(cfg).state_dict()}, str(path))


def _run_main(tmp_path, *extra, config=CFG):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'point_dae_amd.main', '--config', config, *extra,
           '--exp_name', 't']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    losses = [float(line.split('Loss = ')[1].split()[0]) for line in out.splitlines() if 'Loss = ' in line]
    return out, losses


def test_finetune_cli_trains_dgcnn_from_an_autoencoder_checkpoint(tmp_path):
    ckpt = tmp_path / 'pretrain.pth'
    _autoencoder_ckpt(ckpt)
    out, losses = _run_main(tmp_path, '--finetune_model', '--ckpts', str(ckpt), '--max_epoch', '1',
                            '--steps_per_epoch', '20')
    assert 'Successful Loading the ckpt' in out
    assert '[Validation] EPOCH: 0' in out and '[Validation] EPOCH: 1' in out
    assert len(losses) == 2 and all(np.isfinite(losses)), out
    assert losses[1] < losses[0], losses
    assert list(tmp_path.glob('experiments/*/cfgs/t/ckpt-last.pth'))


def test_finetune_cli_trains_dgcnn_from_scratch(tmp_path):
    out, losses = _run_main(tmp_path, '--scratch_model', '--max_epoch', '0', '--steps_per_epoch', '5')
    assert 'Training from scratch!!!' in out
    assert '[Validation] EPOCH: 0' in out
    assert len(losses) == 1 and all(np.isfinite(losses)), out
    assert list(tmp_path.glob('experiments/*/cfgs/t/ckpt-last.pth'))


def test_finetune_cli_epoch_with_a_one_cloud_tail_drops_it(tmp_path):
    """2 total_bs + 1 training clouds: the train loader drops the one-cloud tail, as the reference's drop_last does (a
    B = 1 training step would reach bn_lrelu_dropout, which refuses one row in training mode), so the epoch runs its two
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
    out, losses = _run_main(tmp_path, '--scratch_model', '--max_epoch', '0', config=str(cfg))
    assert '[Epoch 0/0][Batch 2/2]' in out, out
    assert '[Batch 3/' not in out, out
    assert len(losses) == 1 and all(np.isfinite(losses)), out
    assert '[Validation] EPOCH: 0' in out
