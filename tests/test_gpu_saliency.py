"""Input-point gradients on the GPU (saliency_ops, main --vis_saliency): the grouping backward kernel against its fp64
formula, the position embedding's and the eval-mode patch embedder's input gradients against fp64 torch, the whole
classifier against a CPU fp64 restatement at the product's own discrete decisions, the two backends against each other,
the training step left bit for bit where it was, and the CLI end to end in a child process."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from golden_util import _rel, fill_state
from test_saliency_cpu import group_backward_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features.yaml')
DGCNN_CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_dgcnn_smooth.yaml')


def _clouds(B, N, seed):
    from point_dae_amd.synthetic import shapenet_like_clouds
    return torch.from_numpy(shapenet_like_clouds(B, N, seed=seed))


def _rel_l2(got, want):
    """Per-cloud relative L2 error of (B, N, 3) gradients -> (B,) floats."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)).tolist()


# ---- 1. the grouping backward kernel --------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,N,G,k', [(2, 64, 4, 32), (2, 512, 8, 32)])
def test_group_points_backward_equals_the_fp64_formula(B, N, G, k):
    """(2,64,4,32): G k > N, points lie in many groups; (2,512,8,32): at least half the points lie in none.  Indices from
    the product's own FPS and kNN.  A point's gradient is a sum of at most G k + 1 fp32 terms added one by one, so the
    error is at most (G k + 1) 2^-23 of the largest sum of |terms|; uncovered points are exactly 0.0; two runs agree bit
    for bit."""
    from point_dae_amd import _lib
    from point_dae_amd.knn_cuda import knn
    from point_dae_amd.pointnet2_utils import furthest_point_sample_with_centres
    xyz = _clouds(B, N, seed=N).cuda()
    fps_idx, ctr = furthest_point_sample_with_centres(xyz, G)
    _, knn_idx, _ = knn(xyz, ctr, k, with_neighbourhood=True)
    g = torch.Generator().manual_seed(N + G)
    d_nbr = torch.randn(B, G, k, 3, generator=g).cuda()
    d_center = torch.randn(B, G, 3, generator=g).cuda()

    def run():
        out = torch.full((B, N, 3), float('nan'), device='cuda')
        _lib.call('pdae_group_points_backward', d_nbr, B, N, G, k, d_nbr.data_ptr(), d_center.data_ptr(),
                  knn_idx.data_ptr(), fps_idx.data_ptr(), out.data_ptr())
        return out
    got, again = run(), run()
    assert torch.equal(got, again)
    want = group_backward_reference(d_nbr.double().cpu(), d_center.double().cpu(), knn_idx.cpu(), fps_idx.cpu(), N)
    terms = group_backward_reference(d_nbr.double().cpu().abs(), d_center.double().cpu().abs() + 2 * d_nbr.double().cpu().abs().sum(2),
                                     knn_idx.cpu(), fps_idx.cpu(), N)                 # sum of |terms| per coordinate
    err = (got.double().cpu() - want).abs().max().item()
    bound = (G * k + 1) * 2.0 ** -23 * terms.max().item()
    print('group_points_backward', (B, N, G, k), 'max abs err', err, 'bound', bound)
    assert err <= bound
    covered = torch.zeros(B, N, dtype=torch.bool)
    covered.scatter_(1, knn_idx.cpu().reshape(B, -1), True)
    covered.scatter_(1, fps_idx.cpu().long(), True)
    if G * k <= N // 2:
        assert int((~covered).sum()) >= B * N // 2
    assert (~covered).any() or G * k > N
    assert torch.equal(got.cpu()[~covered], torch.zeros(int((~covered).sum()), 3))
    # no centre gradient: the neighbour terms and the centres' subtraction alone
    out = torch.empty(B, N, 3, device='cuda')
    _lib.call('pdae_group_points_backward', d_nbr, B, N, G, k, d_nbr.data_ptr(), None, knn_idx.data_ptr(),
              fps_idx.data_ptr(), out.data_ptr())
    want0 = group_backward_reference(d_nbr.double().cpu(), torch.zeros(B, G, 3, dtype=torch.float64), knn_idx.cpu(),
                                     fps_idx.cpu(), N)
    assert (out.double().cpu() - want0).abs().max().item() <= bound
    with pytest.raises(RuntimeError, match='null pointer'):
        _lib.call('pdae_group_points_backward', d_nbr, B, N, G, k, None, None, knn_idx.data_ptr(), fps_idx.data_ptr(),
                  out.data_ptr())


def test_group_forward_is_bit_identical_with_and_without_a_gradient():
    from point_dae_amd.point_cae_transformer import Group
    xyz = _clouds(3, 256, seed=2).cuda()
    grp = Group(16, 32)
    nb0, c0 = grp(xyz)
    idx = {}
    nb1, c1 = grp(xyz.clone().requires_grad_(), idx)
    assert torch.equal(nb0, nb1) and torch.equal(c0, c1) and not nb0.requires_grad and nb1.requires_grad
    assert idx['fps_idx'].shape == (3, 16) and idx['knn_idx'].shape == (3, 16, 32)


# ---- 2. position embedding and embedder alone ------------------------------------------------------------------------------

def test_pos_embed_input_gradient():
    """Linear(3,128) -> GELU -> Linear(128,384) on centre rows, whole and through a row list (unlisted rows get 0.0),
    against fp64 torch; the bound is 4x the error of the same torch modules run in fp32 against fp64."""
    from point_dae_amd import nn_ops
    from point_dae_amd.point_cae_transformer import pos_embed_layers
    seq = fill_state(pos_embed_layers(384), 3)
    ref64 = fill_state(pos_embed_layers(384), 3).double()
    ref32 = fill_state(pos_embed_layers(384), 3)
    seq = seq.cuda()
    for p in seq.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    xyz = torch.randn(48, 3, generator=g) * 0.5
    d = torch.randn(48, 384, generator=g)
    rows = torch.tensor([5, 0, 47, 13, 21, 8])

    def oracle(ref, dtype, ids):
        x = xyz.detach().to(dtype).clone().requires_grad_()
        y = ref(x if ids is None else x[ids])
        y.backward(d.to(dtype) if ids is None else d[:ids.numel()].to(dtype))
        return x.grad
    for ids in (None, rows):
        x = xyz.cuda().requires_grad_()
        y = nn_ops.pos_embed(x, seq, rows=None if ids is None else ids.cuda())
        y.backward(d.cuda() if ids is None else d[:ids.numel()].cuda())
        want = oracle(ref64, torch.float64, ids)
        base = (oracle(ref32, torch.float32, ids).double() - want).norm() / want.norm()
        err = (x.grad.double().cpu() - want).norm() / want.norm()
        print('pos_embed input gradient rel-L2', float(err), 'fp32 torch', float(base))
        assert float(err) <= 4 * float(base)
        if ids is not None:
            rest = torch.ones(48, dtype=torch.bool)
            rest[ids] = False
            assert torch.equal(x.grad.cpu()[rest], torch.zeros(int(rest.sum()), 3))
        assert all(p.grad is None for p in seq.parameters())


def _embedder_case(BG=8, seed=4):
    from oracle import model as OM
    from point_dae_amd.point_cae_transformer import Encoder
    mine = fill_state(Encoder(384), seed)
    state = mine.state_dict()
    mine = mine.cuda().eval()
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(BG, 32, 3, generator=g) * 0.3
    d = torch.randn(BG, 384, generator=g)
    refs = []
    for dtype in (torch.float64, torch.float32):
        ref = OM.Encoder(384)
        ref.load_state_dict(state)
        refs.append(ref.to(dtype).eval())
    return mine, refs, pts, d


def test_embedder_eval_input_gradient():
    """BG = 8 groups of 32 points, eval mode on non-trivial running statistics: d tokens -> d points against the fp64
    oracle Encoder with the product's ReLU and max-pool decisions replayed; bound: 4x the fp32 oracle's own error at the
    same decisions.  The eval-mode backward still raises when a parameter requires a gradient."""
    from oracle import model as OM
    from point_dae_amd import patch_embed
    from test_gpu_finetune import _assert_near_ties, _embed_decisions, _hook_embedder
    mine, (ref64, ref32), pts, d = _embedder_case()
    for p in mine.parameters():
        p.requires_grad_(False)
    seen = []
    patch_embed.DECISION_HOOK = lambda dd: seen.append({k: v.detach().clone() for k, v in dd.items()})
    try:
        x = pts.cuda().requires_grad_()
        tok = patch_embed.patch_embed(x, mine.first_conv, mine.second_conv, False)
    finally:
        patch_embed.DECISION_HOOK = None
    tok.backward(d.cuda())
    assert x.grad.shape == (8, 32, 3) and all(p.grad is None for p in mine.parameters())
    relus, winners = _embed_decisions(seen[0])
    pre = _hook_embedder(ref64.encoder if hasattr(ref64, 'encoder') else ref64)
    with torch.no_grad():
        ref64(pts.double().view(1, 8, 32, 3))
    _assert_near_ties(pre, relus, winners)
    for h in pre.pop('hooks'):
        h.remove()
    grads = []
    for ref, dtype in ((ref64, torch.float64), (ref32, torch.float32)):
        xr = pts.detach().to(dtype).clone().requires_grad_()
        OM.RELU_AT[:], OM.POOL_AT[:] = [m.clone() for m in relus], [w.clone() for w in winners]
        try:
            t = ref(xr.view(1, 8, 32, 3)).view(8, 384)
            assert not OM.RELU_AT and not OM.POOL_AT
        finally:
            OM.RELU_AT.clear(), OM.POOL_AT.clear()
        if dtype == torch.float64:
            assert _rel(tok, t) <= 1e-5
        t.backward(d.to(dtype))
        grads.append(xr.grad.double())
    want, g32 = grads
    base = float((g32 - want).norm() / want.norm())
    err = float((x.grad.double().cpu() - want).norm() / want.norm())
    print('embedder eval input gradient rel-L2', err, 'fp32 oracle', base)
    assert err <= 4 * base
    # a parameter that requires a gradient in eval mode: the fused backward refuses, as before
    mine.first_conv[3].weight.requires_grad_(True)
    tok = patch_embed.patch_embed(pts.cuda().requires_grad_(), mine.first_conv, mine.second_conv, False)
    with pytest.raises(NotImplementedError, match='training-mode BatchNorm'):
        tok.backward(d.cuda())


def test_embedder_input_gradient_names_its_restrictions():
    from point_dae_amd import patch_embed
    from point_dae_amd.point_cae_transformer import Encoder
    enc = Encoder(384).cuda().eval()
    with pytest.raises(NotImplementedError, match='group_size == 32'):
        patch_embed.patch_embed(torch.zeros(4, 16, 3, device='cuda', requires_grad=True), enc.first_conv, enc.second_conv, False)
    sync = torch.nn.SyncBatchNorm.convert_sync_batchnorm(Encoder(384)).cuda().eval()
    with pytest.raises(NotImplementedError, match='SyncBatchNorm'):
        patch_embed.patch_embed(torch.zeros(4, 32, 3, device='cuda', requires_grad=True), sync.first_conv, sync.second_conv, False)


# ---- 3. whole model --------------------------------------------------------------------------------------------------------

def _cfg(depth, num_group):
    from point_dae_amd.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(CFG).model
    cfg.depth, cfg.num_group, cfg.drop_path_rate = depth, num_group, 0.0
    return cfg


def _oracle_forward(ref, pts, fps_idx, knn_idx, relus, winners, xwin):
    """_OracleClassifier in eval mode from the product's indices: neighbourhoods and centres by differentiable indexing,
    the embedder's decisions and the token max-pool winners replayed (None: the oracle's own) -> logits, norm output."""
    from oracle import model as OM
    B = pts.shape[0]
    bi = torch.arange(B)[:, None]
    center = pts[bi, fps_idx]
    nb = pts[bi[:, :, None], knn_idx] - center[:, :, None]
    if relus is not None:
        OM.RELU_AT[:], OM.POOL_AT[:] = [m.clone() for m in relus], [w.clone() for w in winners]
    try:
        tok = ref.encoder(nb)
        assert not OM.RELU_AT and not OM.POOL_AT
    finally:
        OM.RELU_AT.clear(), OM.POOL_AT.clear()
    x = torch.cat([ref.cls_token.expand(B, -1, -1), tok], 1)
    pos = torch.cat([ref.cls_pos.expand(B, -1, -1), ref.pos_embed(center)], 1)
    x = ref.norm(ref.blocks(x, pos))
    mx = x[:, 1:].max(1)[0] if xwin is None else x[:, 1:].gather(1, xwin[:, None, :]).squeeze(1)
    f = torch.cat([x[:, 0], mx], -1)
    h = ref.cls_head_finetune
    f = torch.relu(h[1](h[0](f)))
    f = torch.relu(h[5](h[4](f)))
    return h[8](f), x


def _oracle_grads(ref, pts, labels, *replay):
    """-> logits, {'logit': grad, 'loss': grad} of the oracle at the replayed decisions."""
    x = pts.clone().requires_grad_()
    logits, _ = _oracle_forward(ref, x, *replay)
    seed = torch.zeros_like(logits).scatter_(1, labels[:, None], 1.0)
    g_logit, = torch.autograd.grad(logits, x, seed, retain_graph=True)
    g_loss, = torch.autograd.grad(torch.nn.functional.cross_entropy(logits, labels, reduction='sum'), x)
    return logits.detach(), {'logit': g_logit, 'loss': g_loss}


_CASES = {}


def _case(depth, num_group, B, N):
    """The product's and the oracle's logits and gradients of one configuration, computed once per module run."""
    key = (depth, num_group, B, N)
    if key in _CASES:
        return _CASES[key]
    from point_dae_amd import patch_embed, saliency_ops
    from point_dae_amd.point_transformer import PointTransformer
    from test_gpu_finetune import _assert_near_ties, _embed_decisions, _hook_embedder, _OracleClassifier
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cfg = _cfg(depth, num_group)
    mine = fill_state(PointTransformer(cfg), 11)
    state = mine.state_dict()
    mine = mine.cuda().eval()
    for p in mine.parameters():
        p.requires_grad_(False)
    pts = _clouds(B, N, seed=13)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, cfg.cls_dim, B))
    seen, cap = [], {}
    patch_embed.DECISION_HOOK = lambda d: seen.append({k: v.detach().clone() for k, v in d.items()})
    try:
        x = pts.cuda().requires_grad_()
        logits = mine(x, capture=cap)
    finally:
        patch_embed.DECISION_HOOK = None
    logits.backward(torch.zeros_like(logits).scatter_(1, labels.cuda()[:, None], 1.0))
    assert x.grad is not None and x.grad.shape == (B, N, 3)               # (None on a library without input gradients)
    assert len(seen) == 1 and all(p.grad is None for p in mine.parameters())
    mine_g = {'logit': x.grad.clone()}
    for score in ('logit', 'loss'):
        lg, g = saliency_ops.input_gradients(mine, pts.cuda(), labels.cuda(), score)
        assert torch.equal(lg, logits.detach())
        if score == 'logit':
            assert torch.equal(g, mine_g['logit'])                            # two runs: the same bits
        mine_g[score] = g
    relus, winners = _embed_decisions(seen[0])
    xwin = cap['x'].detach()[:, 1:].max(1)[1].cpu()
    fps_idx, knn_idx = cap['fps_idx'].long().cpu(), cap['knn_idx'].cpu()
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ref = _OracleClassifier(cfg)
        ref.load_state_dict(state)
        ref = ref.to(dtype).eval()
        for p in ref.parameters():
            p.requires_grad_(False)
        refs[dtype] = ref
    # the oracle's own decisions: every one the product takes differently must be a near-tie
    pre = _hook_embedder(refs[torch.float64].encoder)
    with torch.no_grad():
        own_logits, own_x = _oracle_forward(refs[torch.float64], pts.double(), fps_idx, knn_idx, None, None, None)
    _assert_near_ties(pre, relus, winners)
    for h in pre.pop('hooks'):
        h.remove()
    tokens = own_x[:, 1:]
    gap = ((tokens.amax(1) - tokens.gather(1, xwin[:, None, :]).squeeze(1)) / tokens.abs().amax(dim=(0, 1)).clamp_min(1e-30)).max().item()
    print('token max-pool: largest gap / channel max of a replayed winner', gap)
    assert gap <= 1e-5
    l64, g64 = _oracle_grads(refs[torch.float64], pts.double(), labels, fps_idx, knn_idx, relus, winners, xwin)
    l32, g32 = _oracle_grads(refs[torch.float32], pts.float(), labels, fps_idx, knn_idx, relus, winners, xwin)
    _CASES[key] = types.SimpleNamespace(cfg=cfg, mine=mine, pts=pts, labels=labels, logits=logits.detach(), grads=mine_g,
                                        l64=l64, g64=g64, g32=g32, own_logits=own_logits)
    return _CASES[key]


@pytest.mark.parametrize('depth,num_group,B,N', [(2, 16, 3, 256), (12, 64, 2, 1024)])
def test_model_input_gradients_equal_the_fp64_oracle(depth, num_group, B, N):
    """PointTransformer in eval mode, weights from fill_state, every parameter frozen: logits within 1e-5 and the
    gradient of both scores with respect to the points within 4x what the oracle's own fp32 run shows against its fp64
    run (same replayed decisions), per cloud in relative L2.  The oracle takes the product's FPS / kNN indices, its
    embedder decisions and its token max-pool winners; every decision that differs from the oracle's own is a near-tie.

    Measured on an MI355X (worst cloud, relative L2; product / fp32 oracle):
      depth 2,  G 16, B 3, N 256:   logit 6.17e-7 / 1.06e-6,  loss 5.86e-7 / 1.38e-6
      depth 12, G 64, B 2, N 1024:  logit 5.74e-7 / 8.80e-7,  loss 6.02e-7 / 9.17e-7
    (at depth 12 one embedder pool winner differs from the fp64 oracle's own, 9.7e-8 of its channel's maximum apart)
    """
    c = _case(depth, num_group, B, N)
    assert _rel(c.logits, c.l64) <= 1e-5 and _rel(c.own_logits, c.l64) <= 1e-5
    for score in ('logit', 'loss'):
        mine, base = max(_rel_l2(c.grads[score], c.g64[score])), max(_rel_l2(c.g32[score], c.g64[score]))
        print('input gradient (%s) depth %d G %d: product rel-L2 %.3e, fp32 oracle %.3e' % (score, depth, num_group, mine, base))
        assert torch.isfinite(c.grads[score]).all() and float(c.grads[score].abs().max()) > 0
        assert mine <= 4 * base, (score, mine, base)


def test_linear_classifier_input_gradients():
    """PointTransformerLinearClassification shares the trunk: its points take a finite, non-zero gradient too."""
    from point_dae_amd import saliency_ops
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_transformer import PointTransformerLinearClassification
    cfg = _cfg(2, 16)
    model = fill_state(PointTransformerLinearClassification(cfg), 5).cuda()
    pts = _clouds(3, 256, seed=1).cuda()
    logits, grad = saliency_ops.input_gradients(model, pts, torch.tensor([1, 0, 7]).cuda())
    assert grad.shape == (3, 256, 3) and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    assert all(p.requires_grad and p.grad is None for p in model.parameters())


# ---- 4. backends -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('score', ['logit', 'loss'])
def test_backends_share_the_logits_and_agree_on_the_gradient(score, monkeypatch):
    from point_dae_amd import saliency_ops
    c = _case(2, 16, 3, 256)
    out = {}
    for name in ('hip', 'torch'):
        monkeypatch.setenv('PDAE_SALIENCY', name)
        out[name] = saliency_ops.input_gradients(c.mine, c.pts.cuda(), c.labels.cuda(), score)
    assert torch.equal(out['hip'][0], out['torch'][0])
    bound = 4 * max(_rel_l2(c.g32[score], c.g64[score]))
    diff = max(_rel_l2(out['torch'][1], out['hip'][1]))
    print('backends (%s): torch against hip rel-L2 %.3e, torch against fp64 %.3e, bound %.3e'
          % (score, diff, max(_rel_l2(out['torch'][1], c.g64[score])), bound))
    assert diff <= bound
    assert max(_rel_l2(out['torch'][1], c.g64[score])) <= bound


# ---- 5. nothing moved ------------------------------------------------------------------------------------------------------

def test_training_step_is_bit_identical_with_the_switches_bypassed(monkeypatch):
    """Points without a gradient, parameters with one: a training-mode step gives the bits of the path before input
    gradients existed (the grouping under no_grad with its two launches, every weight gradient issued)."""
    from point_dae_amd import _lib, rows
    from point_dae_amd.knn_cuda import knn
    from point_dae_amd.point_cae_transformer import Group
    from point_dae_amd.point_transformer import PointTransformer
    from point_dae_amd.pointnet2_utils import furthest_point_sample_with_centres

    @torch.no_grad()
    def old_group(self, xyz, indices=None):
        _, center = furthest_point_sample_with_centres(xyz, self.num_group)
        _, _, neighborhood = knn(xyz, center, self.group_size, with_neighbourhood=True)
        return neighborhood, center
    cfg = _cfg(2, 16)
    pts, labels = _clouds(4, 256, seed=6).cuda(), torch.tensor([3, 1, 0, 2]).cuda()
    _lib.set_deterministic(True)
    try:
        runs = []
        for bypass in (False, True):
            if bypass:
                monkeypatch.setattr(rows, 'SKIP_FROZEN_WGRAD', False)
                monkeypatch.setattr(Group, 'forward', old_group)
            model = fill_state(PointTransformer(cfg), 9).cuda().train()
            torch.manual_seed(4)
            loss, _ = model.get_loss_acc(model(pts), labels)
            loss.backward()
            runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
    finally:
        _lib.set_deterministic(False)
    (la, ga), (lb, gb) = runs
    assert torch.equal(la, lb) and ga.keys() == gb.keys() and len(ga) > 40
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_frozen_model_leaves_no_parameter_gradient():
    c = _case(2, 16, 3, 256)
    x = c.pts.cuda().requires_grad_()
    c.mine(x).sum().backward()
    assert x.grad is not None and all(p.grad is None for p in c.mine.parameters())


# ---- 6. CLI ----------------------------------------------------------------------------------------------------------------

def _tiny_yaml(tmp_path, src, bs, model=None):
    import yaml
    raw = yaml.safe_load(open(src))
    base = dict(NAME='ModelNet', DATA_PATH='unused', N_POINTS=300, NUM_CATEGORY=40, USE_NORMALS=False)
    for subset in ('train', 'val', 'test'):
        raw['dataset'][subset] = dict(_base_=dict(base), others=dict(raw['dataset'][subset]['others'], count=2 * bs + 1))
    raw['total_bs'], raw['npoints'] = bs, 256
    raw['model'].update(model or {})
    cfg = tmp_path / 'saliency.yaml'
    yaml.safe_dump(raw, open(cfg, 'w'))
    return cfg


def test_cli_writes_the_saliency_tensor_of_the_whole_test_set(tmp_path):
    """2 bs + 1 synthetic test clouds through `main --vis_saliency` in a child process: exit 0, '[TEST] acc', and
    saliency.pt = (2 bs + 1, npoints, 6): the FPS-sampled points, then their finite, non-zero gradients."""
    from point_dae_amd import builder, runner_finetune
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.misc import fps
    from point_dae_amd.svm_probe import Acc_Metric
    bs = 2
    cfg = _tiny_yaml(tmp_path, CFG, bs, dict(depth=2, num_group=16, drop_path_rate=0.0))
    config = cfg_from_yaml_file(str(cfg))
    model = builder.model_builder(config.model)
    model.load_model_from_ckpt(None, log=lambda *a: None)
    args = types.SimpleNamespace(experiment_path=str(tmp_path / 'saved'), local_rank=0)
    os.makedirs(args.experiment_path)
    builder.save_checkpoint(model, torch.optim.AdamW(model.parameters()), 0, Acc_Metric(0.), Acc_Metric(0.), 'ckpt-best', args)
    ckpt = tmp_path / 'saved' / 'ckpt-best.pth'
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop('PDAE_SALIENCY', None)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'point_dae_amd.main', '--config', str(cfg), '--vis_saliency',
           '--ckpts', str(ckpt), '--exp_name', 's']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('[TEST] acc = ') == 1 and 'Saliency backend: hip, score: logit' in r.stdout, r.stdout
    saved = list(tmp_path.glob('experiments/*/*/s/saliency.pt'))
    assert len(saved) == 1 and saved[0].name in r.stdout
    sal = torch.load(str(saved[0]), map_location='cpu')
    assert sal.shape == (2 * bs + 1, 256, 6) and sal.dtype == torch.float32
    loader = runner_finetune._loader(config.dataset.test, torch.device('cuda', 0), 0, 0, 1, bs)
    want = torch.cat([fps(data[0].cuda(), 256)[1][:, :, :3] for _, _, data in loader]).cpu()
    assert torch.equal(sal[:, :, :3], want)
    assert torch.isfinite(sal[:, :, 3:]).all() and float(sal[:, :, 3:].abs().max()) > 0
    assert all(float(sal[i, :, 3:].abs().max()) > 0 for i in range(2 * bs + 1))


def test_cli_names_the_attribute_for_a_model_without_input_gradients(tmp_path):
    bs = 2
    cfg = _tiny_yaml(tmp_path, DGCNN_CFG, bs)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'point_dae_amd.main', '--config', str(cfg), '--vis_saliency',
           '--ckpts', str(tmp_path / 'none.pth'), '--exp_name', 's']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode != 0
    assert 'input_grad_supported' in r.stdout + r.stderr
    assert not list(tmp_path.glob('experiments/*/*/s/saliency.pt'))
