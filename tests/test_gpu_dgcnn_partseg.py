"""The two-layer EdgeConv kernel (csrc/edge2_eval.hip), the DGCNN head kernels of csrc/partseg.hip, DGCNNPartSeg
(point_dae_amd/dgcnn_partseg.py) and the --part_seg --test protocol with it, on the GPU.

Yardstick (as tests/test_gpu_partseg.py): errors are max norms relative to the largest output, against fp64
(tests/dgcnn_partseg_restatement.py, itself checked against the live reference in tests/test_dgcnn_partseg_cpu.py);
e_layers is the error of the `layers` form -- kernels that predate this model plus framework glue -- on the same case
against the same fp64 result; the new path is of the same arithmetic class (fp32 products, fp32 accumulation), so it must
stay within 4 e_layers, and within the project's 1e-5 pin for evaluation-mode outputs.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import dgcnn_partseg_restatement as R  # noqa: E402
import partseg_restatement as PR  # noqa: E402
import weights  # noqa: E402
from test_dgcnn_partseg_cpu import CONFIG, GAP_FACTOR, build_model, fixture  # noqa: E402
from test_gpu_partseg import TAIL_CASES  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
PIN = 1e-5
DEAD = (1, 17, 40)                       # layer-2 channels whose shift makes every output negative
DEAD1 = 9                                # a layer-1 channel dead in the same way
#               B, N, k
EDGE2_CASES = [(1, 1, 1),                # one point, its own neighbour
               (1, 20, 20),              # every point neighbours every point
               (2, 70, 20),              # N k no multiple of a row tile; a cloud boundary falls inside a block
               (3, 33, 7)]               # 18 points per block: blocks straddle clouds, the last one is partial


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


def _signed(n, gen):
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return sign * (1.0 + 0.1 * torch.randn(n, generator=gen)), 0.3 * torch.randn(n, generator=gen)


# ---- pdae_edge2_eval_forward -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge2_case(B, N, k):
    """Seeded inputs (CPU, fp32) and the fp64 definition's result."""
    gen = torch.Generator().manual_seed(10000 * B + 100 * N + k)
    pq = torch.randn(B * N, 128, generator=gen)
    idx = torch.randint(0, N, (B, N, k), generator=gen, dtype=torch.int32)      # in range, with repeats
    if k == N:                                                                   # every point neighbours every point (itself too)
        idx = torch.stack([torch.stack([torch.randperm(N, generator=gen) for _ in range(N)]) for _ in range(B)]).int()
    else:
        idx[:, :, 0] = torch.arange(N, dtype=torch.int32)                        # self-edges
        idx[:, :, 2] = idx[:, :, 1]                                              # a repeated neighbour in every row
    s1, t1 = _signed(64, gen)
    s2, t2 = _signed(64, gen)
    s1[DEAD1], t1[DEAD1] = 0.5, -1000.0
    for c in DEAD:
        s2[c], t2[c] = 0.5, -1000.0
    w2 = torch.randn(64, 64, generator=gen) / 8.0
    w2[:, DEAD1] *= 1e-3                                                         # (the dead input is -200: keep its share small)
    want = R.edge2(pq.double().reshape(B, N, 128), idx.long(), s1.double(), t1.double(), w2.double(), s2.double(), t2.double())
    return pq, idx, s1, t1, w2, s2, t2, want.reshape(B * N, 64)


def run_edge2(dims, out2=None, col=0):
    from point_dae_amd import dgcnn_partseg
    pq, idx, s1, t1, w2, s2, t2 = (t.cuda() for t in edge2_case(*dims)[:7])
    out = dgcnn_partseg.edge2_eval(pq, idx, s1, t1, w2, s2, t2, out2=out2, col=col)
    torch.cuda.synchronize()
    return out


def run_edge2_layers(dims):
    """The same block layer by layer on kernels that predate csrc/edge2_eval.hip: the per-edge tensor by index gather,
    pdae_bn_lrelu_rows, the row GEMM, amax."""
    from point_dae_amd.dgcnn_partseg import bn_lrelu_rows
    from point_dae_amd.rows import linear_any
    B, N, k = dims
    pq, idx, s1, t1, w2, s2, t2 = (t.cuda() for t in edge2_case(*dims)[:7])
    flat = (idx.long() + (torch.arange(B, device=pq.device) * N).view(B, 1, 1)).reshape(-1)
    e = (pq[:, :64][flat].reshape(B * N, k, 64) + pq[:, 64:].unsqueeze(1)).reshape(B * N * k, 64).contiguous()
    h = bn_lrelu_rows(e, s1, t1)
    out = bn_lrelu_rows(linear_any(h, w2), s2, t2).reshape(B * N, k, 64).amax(1)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dims', EDGE2_CASES, ids=lambda d: 'x'.join(str(v) for v in d))
def test_edge2_against_the_fp64_definition(dims):
    B, N, k = dims
    want = edge2_case(*dims)[-1]
    got = run_edge2(dims)
    layers = run_edge2_layers(dims)
    err, e_layers = _rel(got, want), _rel(layers, want)
    live = [c for c in range(64) if c not in DEAD]
    err_live = _rel(got[:, live], want[:, live])
    print('edge2_eval %s: error %.3e, e_layers %.3e (ratio %.2f); live channels alone %.3e, layers %.3e'
          % (dims, err, e_layers, err / max(e_layers, 1e-30), err_live, _rel(layers[:, live], want[:, live])))
    assert got.shape == want.shape == (B * N, 64) and got.dtype == torch.float32
    assert err <= FACTOR * e_layers
    assert err <= PIN
    assert err_live <= PIN                                   # (the dead channels' -200 does not carry the norm)
    got = got.cpu()
    for c in DEAD:                                           # every edge's output is negative: the max is that negative number
        assert bool((got[:, c] < -100.0).all())
        assert _rel(got[:, c], want[:, c]) <= PIN
    # the second copy at a column offset of a 192-wide tensor, and nothing else of it
    wide = torch.full((B * N, 192), -7.0, device='cuda')
    again = run_edge2(dims, out2=wide, col=64)
    assert torch.equal(again.cpu(), got)                     # the same bits twice
    wide = wide.cpu()
    assert torch.equal(wide[:, 64:128], got)
    assert bool((wide[:, :64] == -7.0).all()) and bool((wide[:, 128:] == -7.0).all())


def test_edge2_refused_layouts_return_unsupported_and_write_nothing():
    from point_dae_amd import _lib, dgcnn_partseg
    lib = _lib.lib()
    assert all(dgcnn_partseg.edge2_supported(k) for k in range(1, 33))
    assert not dgcnn_partseg.edge2_supported(0) and not dgcnn_partseg.edge2_supported(33)
    assert not dgcnn_partseg.edge2_supported(20, 48, 64) and not dgcnn_partseg.edge2_supported(20, 64, 32)
    unsupported = _lib.CONST['PDAE_ERR_UNSUPPORTED']
    B, N = 2, 40
    for k, C1, C2 in ((33, 64, 64), (20, 48, 64), (20, 64, 32)):
        pq = torch.randn(B * N, 2 * C1, device='cuda')
        idx = torch.zeros(B, N, k, dtype=torch.int32, device='cuda')
        vec = torch.ones(64, device='cuda')
        w2 = torch.ones(C2, C1, device='cuda')
        out = torch.full((B * N, 64), -7.0, device='cuda')
        wide = torch.full((B * N, 192), -7.0, device='cuda')
        rc = lib.pdae_edge2_eval_forward(B, N, k, C1, C2, pq.data_ptr(), idx.data_ptr(), vec.data_ptr(), vec.data_ptr(),
                                         w2.data_ptr(), vec.data_ptr(), vec.data_ptr(), out.data_ptr(), wide.data_ptr(), 192,
                                         _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == unsupported and b'edge2_eval' in lib.pdae_last_error()
        assert bool((out == -7.0).all()) and bool((wide == -7.0).all())
        # null pointers: never looked at
        assert lib.pdae_edge2_eval_forward(B, N, k, C1, C2, *([None] * 9), 0, None) == unsupported


# ---- pdae_partseg_cloud_bias_lrelu -----------------------------------------------------------------------------------
def test_cloud_bias_lrelu_is_bit_equal_to_the_framework_expression():
    from point_dae_amd import dgcnn_partseg
    B, N, C = 2, 70, 256
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(B * N, C, generator=gen).cuda()
    g = torch.randn(B, C, generator=gen).cuda()
    z = (y.reshape(B, N, C) + g.unsqueeze(1)).reshape(B * N, C)
    want = torch.where(z > 0, z, 0.2 * z)
    got = dgcnn_partseg.cloud_bias_lrelu(y.clone(), g, B, N)
    torch.cuda.synchronize()
    assert bool((want < 0).any()) and bool((want > 0).any())
    assert torch.equal(got, want)


# ---- pdae_partseg_logits_tail ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_case(S, N, ranges, with_bias):
    gen = torch.Generator().manual_seed(91 * N + S)
    y = torch.randn(S * N, 128, generator=gen)
    scale, shift = _signed(128, gen)
    for c in DEAD:
        scale[c], shift[c] = 0.5, -1000.0
    w = torch.randn(50, 128, generator=gen) / 11.0
    w[:, list(DEAD)] *= 1e-2
    bias = 0.1 * torch.randn(50, generator=gen) if with_bias else None
    # two identical rows inside each range: their logits tie exactly, the lower index must win
    w[29], w[33] = w[28], w[31]
    if with_bias:
        bias[29], bias[33] = bias[28], bias[31]
    lo = torch.tensor([r[0] for r in ranges], dtype=torch.int32)
    hi = torch.tensor([r[1] for r in ranges], dtype=torch.int32)
    seg = torch.stack([torch.randint(r[0], r[1] + 1, (N,), generator=gen, dtype=torch.int32) for r in ranges])
    want = R.logits_tail(y.double(), scale.double(), shift.double(), w.double(), bias.double() if with_bias else None)
    return y, scale, shift, w, bias, seg, lo, hi, want


def run_tail(dims, with_bias):
    from point_dae_amd import dgcnn_partseg, partseg_ops
    S, N, ranges = dims
    y, scale, shift, w, bias, seg, lo, hi = (t.cuda() if t is not None else None for t in tail_case(*dims, with_bias)[:8])
    counts = partseg_ops.Counts(S, y.device)
    logits, pred = dgcnn_partseg.logits_tail(y, scale, shift, w, bias, S, N, seg, lo, hi, counts)
    torch.cuda.synchronize()
    counts.filled, counts.points = S, S * N
    return logits.cpu(), pred.cpu(), counts.read()


@pytest.mark.parametrize('with_bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('dims', TAIL_CASES, ids=lambda d: '%dx%d' % d[:2])
def test_logits_tail_against_the_fp64_definition_and_exactly(dims, with_bias):
    S, N, ranges = dims
    seg, want = tail_case(*dims, with_bias)[5], tail_case(*dims, with_bias)[-1]
    logits, pred, counts = run_tail(dims, with_bias)
    err = _rel(logits, want)
    print('partseg_logits_tail %dx%d bias %s: error %.3e' % (S, N, with_bias, err))
    assert logits.shape == (S * N, 50) and logits.dtype == torch.float32
    assert err <= PIN
    # the prediction is the restricted argmax of the RETURNED logits, first index on ties
    lg = logits.numpy().reshape(S, N, 50)
    want_pred = np.stack([PR.restricted_argmax(lg[s], list(range(ranges[s][0], ranges[s][1] + 1))) for s in range(S)])
    assert np.array_equal(pred.numpy().reshape(S, N), want_pred)
    assert bool((lg[:, :, 28] == lg[:, :, 29]).all()) and bool((lg[:, :, 31] == lg[:, :, 33]).all())
    assert 29 not in want_pred and 33 not in want_pred
    # every count equals the numpy definition on those predictions
    classes = {'c%d' % s: list(range(r[0], r[1] + 1)) for s, r in enumerate(dict.fromkeys(ranges))}
    ref = PR.metric(want_pred, seg.numpy(), classes)['counts']
    for key in ('shape_iu', 'shape_correct', 'part_seen', 'part_correct'):
        assert np.array_equal(counts[key], ref[key]), key
    logits2, pred2, counts2 = run_tail(dims, with_bias)
    assert torch.equal(logits2, logits) and torch.equal(pred2, pred)
    assert all(np.array_equal(counts2[k], counts[k]) for k in ('shape_iu', 'shape_correct', 'part_seen', 'part_correct'))


def test_logits_tail_refusals():
    from point_dae_amd import _lib
    lib = _lib.lib()
    unsupported = _lib.CONST['PDAE_ERR_UNSUPPORTED']
    for K, P in ((256, 50), (128, 40), (64, 50)):            # null pointers: never looked at
        assert lib.pdae_partseg_logits_tail(2, 64, K, P, None, None, None, 0.2, *([None] * 11), None) == unsupported
        assert b'partseg_logits_tail' in lib.pdae_last_error()
    assert lib.pdae_partseg_cloud_bias_lrelu(2, 64, 254, None, None, 0.2, None) == unsupported


# ---- the model on the live-reference fixtures --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_run(which, backend):
    """One forward of the model on fixture `which` under PDAE_PARTSEG=backend with the fixture's graphs injected ->
    (logits (CPU), capture (CPU tensors), the error of the logits at sub_idx against logits64)."""
    f = fixture(which)
    old = os.environ.get('PDAE_PARTSEG')
    os.environ['PDAE_PARTSEG'] = backend
    try:
        model = weights.fill_state(build_model(), int(f['seed'])).cuda().eval()
        graphs = torch.from_numpy(f['graphs'].astype(np.int32)).cuda()
        cap = {}
        logits = model(torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['cls']).cuda(), capture=cap, graphs=graphs)
        plain = model(torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['cls']).cuda(), graphs=graphs)
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ['PDAE_PARTSEG']
        else:
            os.environ['PDAE_PARTSEG'] = old
    assert torch.equal(plain, logits)                                     # capture changes no bits
    logits = logits.cpu()
    sub = torch.from_numpy(f['sub_idx']).long()
    got = torch.gather(logits, 1, sub.unsqueeze(-1).expand(-1, -1, 50))
    cap = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in cap.items()}
    return logits, cap, _rel(got, torch.from_numpy(f['logits64']))


@pytest.mark.parametrize('backend', ['layers', 'hip'])
@pytest.mark.parametrize('which', ['a', 'b'])
def test_model_on_the_live_reference_fixtures(which, backend):
    f = fixture(which)
    logits, cap, err = model_run(which, backend)
    print('dgcnn partseg %s PDAE_PARTSEG=%s: logits vs reference fp64 %.3e (reference fp32 %.2e)'
          % (which, backend, err, float(f['dist'])))
    assert cap['partseg'] == backend
    assert logits.shape == (2, 512, 50) and logits.dtype == torch.float32
    assert err <= PIN
    if backend == 'hip':
        e_layers = model_run(which, 'layers')[2]
        print('    e_layers %.3e (ratio %.2f)' % (e_layers, err / max(e_layers, 1e-30)))
        assert err <= FACTOR * e_layers
    # the full-range argmax agrees wherever the fp64 top-two gap is at least 100 times the measured error
    abs_err = err * float(f['scale64'])
    clear = torch.from_numpy(f['margin64'].astype(np.float64)) >= 100.0 * abs_err
    assert float(clear.double().mean()) >= 0.99
    assert torch.equal(logits.argmax(-1)[clear], torch.from_numpy(f['argmax64']).long()[clear])
    # the model's own selection on the features at hand: the fixture's graph, as a set, on every row whose k-th / (k+1)-th
    # gap is clear of the distance expression's rounding
    assert torch.equal(cap['graphs'], torch.from_numpy(f['graphs'].astype(np.int32)))
    for l in range(3):
        ok = torch.from_numpy(f['gap64'][l] >= GAP_FACTOR * f['pd_err'][l])
        assert float(ok.double().mean()) >= 0.98
        own, want = cap['graphs_own'][l].long().sort(-1)[0], torch.from_numpy(f['graphs'][l].astype(np.int64)).sort(-1)[0]
        assert torch.equal(own[ok], want[ok]), 'layer %d' % l
    assert cap['x1'].shape == cap['x2'].shape == cap['x3'].shape == (2 * 512, 64) and cap['global'].shape == (2, 1024)


@pytest.mark.parametrize('backend', ['layers', 'hip'])
def test_model_without_graphs_equals_a_run_injected_with_its_own(backend, monkeypatch):
    monkeypatch.setenv('PDAE_PARTSEG', backend)
    f = fixture('a')
    model = weights.fill_state(build_model(), int(f['seed'])).cuda().eval()
    pts, cls = torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['cls']).cuda()
    cap = {}
    free = model(pts, cls, capture=cap)
    assert torch.equal(cap['graphs'], cap['graphs_own']) and cap['graphs'].shape == (3, 2, 512, 20)
    injected = model(pts, cls, graphs=cap['graphs'].clone())
    plain = model(pts, cls)
    torch.cuda.synchronize()
    assert torch.equal(injected, free) and torch.equal(plain, free)
    with pytest.raises(ValueError, match='graphs'):
        model(pts, cls, graphs=cap['graphs'][:2])


def test_refused_layout_falls_back_to_layers_and_says_so(monkeypatch):
    """cls_dim = 40 is outside pdae_partseg_logits_tail: the layers form runs under PDAE_PARTSEG=hip, and both the capture
    and the line the runner prints (partseg_mode) name it."""
    monkeypatch.setenv('PDAE_PARTSEG', 'hip')
    from point_dae_amd.synthetic import shapenet_like_clouds
    pts = torch.from_numpy(shapenet_like_clouds(2, 96, seed=9))
    cls = torch.tensor([3, 11])
    model = weights.fill_state(build_model(cls_dim=40), 12).cuda().eval()
    assert model.partseg_mode() == 'layers' and build_model().partseg_mode() == 'hip'
    cap = {}
    logits = model(pts.cuda(), cls.cuda(), capture=cap)
    torch.cuda.synchronize()
    assert cap['partseg'] == 'layers' and logits.shape == (2, 96, 40)
    sd = {k: (v.double().cpu() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}
    want = R.forward(pts.double(), cls, sd, cap['graphs'].cpu().long())['logits']
    err = _rel(logits, want)
    print('cls_dim 40 (layers): logits vs fp64 on the model\'s own graphs %.3e' % err)
    assert err <= PIN


def test_prepared_operands_follow_the_weights(monkeypatch):
    """The hip form keeps its weight-only operands between forwards; new weights (load_state_dict writes in place) must be
    seen: the same bits as a fresh model with those weights."""
    monkeypatch.setenv('PDAE_PARTSEG', 'hip')
    f = fixture('a')
    pts, cls = torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['cls']).cuda()
    graphs = torch.from_numpy(f['graphs'].astype(np.int32)).cuda()
    model = weights.fill_state(build_model(), 11).cuda().eval()
    first = model(pts, cls, graphs=graphs)
    assert model.prepared() is model.prepared()
    weights.fill_state(model, 12)
    second = model(pts, cls, graphs=graphs)
    fresh = weights.fill_state(build_model(), 12).cuda().eval()(pts, cls, graphs=graphs)
    torch.cuda.synchronize()
    assert torch.equal(second, fresh) and not torch.equal(second, first)


def test_model_in_training_mode_raises():
    model = build_model().cuda().train()
    with pytest.raises(NotImplementedError, match='training is not built'):
        model(torch.rand(2, 64, 3).cuda(), torch.zeros(2, dtype=torch.long).cuda())


# ---- the protocol ------------------------------------------------------------------------------------------------------
def _protocol(tmp_path, monkeypatch):
    from point_dae_amd import parser, runner_finetune
    from point_dae_amd.config import get_config
    from point_dae_amd.misc import set_random_seed
    monkeypatch.chdir(ROOT)
    monkeypatch.setenv('LOCAL_RANK', '0')
    args = parser.get_args(['--config', CONFIG, '--part_seg', '--test', '--scratch_model', '--total_bs', '8', '--exp_name',
                            'ci_dgcnn_partseg', '--root_folder', os.path.relpath(str(tmp_path / 'exp'), ROOT)])
    args.distributed, args.world_size, args.use_gpu = False, 1, True
    config = get_config(args)
    config.total_bs = args.total_bs
    for split in ('train', 'val', 'test'):
        config.dataset[split].others.npoints = 256
        config.dataset[split].others.count = 16
    config.npoints = 256
    set_random_seed(args.seed)
    lines = []

    def log(s):
        print(s)
        lines.append(str(s))
    miou = runner_finetune.part_seg_test(args, config, log=log)
    return lines, miou, args, config


@pytest.mark.parametrize('backend', ['hip', 'layers'])
def test_part_seg_test_on_the_synthetic_stand_in(tmp_path, monkeypatch, backend):
    from point_dae_amd import builder, partseg_ops, runner_finetune
    from point_dae_amd.misc import set_random_seed
    monkeypatch.setenv('PDAE_PARTSEG', backend)
    lines, miou, args, config = _protocol(tmp_path, monkeypatch)
    assert 'Part-segmentation backend: %s' % backend in lines
    assert any(ln.startswith('ShapeNetPart test source: synthetic stand-in') for ln in lines)
    cats = [ln for ln in lines if ln.startswith('eval mIoU of ')]
    assert [ln[len('eval mIoU of '):][:14].strip() for ln in cats] == sorted(partseg_ops.SEG_CLASSES) and len(cats) == 16
    assert all(len(ln.split()) == 5 for ln in cats)
    final = [ln for ln in lines if ln.startswith('test Accuracy: ')]
    m = args.part_seg_metrics
    assert final == ['test Accuracy: %f  Class avg mIOU: %f   Inctance avg mIOU: %f'
                     % (m['accuracy'], m['class_avg_iou'], m['inctance_avg_iou'])]
    assert lines[-1] == final[0] and miou == m['inctance_avg_iou']
    # the four metrics equal the numpy definition on the model's own per-point predictions, taken through forward
    set_random_seed(args.seed)
    device = torch.device('cuda', torch.cuda.current_device())
    loader = runner_finetune._loader(config.dataset.test, device, args.seed, 0, 1, config.total_bs)
    set_random_seed(args.seed)
    model = builder.model_builder(config.model)
    model.load_model_from_ckpt(None, log=lambda s: None)
    model = model.to(device).eval()
    cat_of = {l: c for c, ls in partseg_ops.SEG_CLASSES.items() for l in ls}
    preds, segs = [], []
    for _, _, (points, cls, seg) in loader:
        logits = model(points, cls).cpu().numpy()
        seg = seg.cpu().numpy()
        preds.append(np.stack([PR.restricted_argmax(logits[i], partseg_ops.SEG_CLASSES[cat_of[int(seg[i, 0])]])
                               for i in range(len(seg))]))
        segs.append(seg)
    ref = PR.metric(np.concatenate(preds), np.concatenate(segs), partseg_ops.SEG_CLASSES)
    for key in ('accuracy', 'class_avg_accuracy', 'class_avg_iou', 'inctance_avg_iou'):
        np.testing.assert_allclose(m[key], ref[key], rtol=0, atol=1e-12, equal_nan=True, err_msg=key)
    for cat, v in ref['category_iou'].items():
        np.testing.assert_allclose(m['category_iou'][cat], v, rtol=0, atol=1e-12, err_msg=cat)
    lines2, miou2, _, _ = _protocol(tmp_path, monkeypatch)
    assert lines2 == lines and miou2 == miou
