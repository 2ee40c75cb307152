"""The part-segmentation head's kernels (csrc/partseg.hip, point_dae_amd/partseg_ops.py), PointTransformerPartSeg
(point_dae_amd/part_seg.py) and the --part_seg --test protocol on the GPU.

Yardstick (as tests/test_gpu_sa_eval.py): errors are max norms relative to the largest output; e_layers is the error of
the `layers` form -- kernels that predate csrc/partseg.hip -- on the same case against the same fp64 result
(tests/partseg_restatement.py, itself checked against the live reference in tests/test_partseg_cpu.py); the new path is
of the same arithmetic class, so it must stay within 4 e_layers, and within the project's 1e-5 pin for evaluation-mode
outputs.
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
import partseg_restatement as R  # noqa: E402
import weights  # noqa: E402
from test_partseg_cpu import CONFIG, build_model, fixture  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
PIN = 1e-5
MARGIN = 1e-6
#              B, N, G, C
PROP_CASES = [(2, 70, 3, 64),            # exactly three centres, N no multiple of a block's 32 points
              (1, 1, 4, 64),
              (3, 96, 7, 1536),
              (2, 200, 128, 1536)]
DEAD = (1, 17, 40)                       # channels whose shift makes every pre-activation negative
#              S, N, (lo, hi) per shape
TAIL_CASES = [(1, 1, ((28, 29),)), (1, 70, ((30, 35),)), (2, 200, ((28, 29), (30, 35)))]


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


# ---- pdae_partseg_propagate ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prop_case(B, N, G, C):
    """Seeded inputs (CPU, fp32) and the fp64 result of the LITERAL first layer: interpolate the features F (B, G, K),
    concatenate them with the point, one affine + ReLU layer of width C."""
    K = 24                                                   # the feature width ahead of the layer (a multiple of 4)
    gen = torch.Generator().manual_seed(1000 * N + 10 * G + C)
    direction = torch.randn(B, N + G, 3, generator=gen)
    pts = direction / direction.norm(dim=-1, keepdim=True) * torch.rand(B, N + G, 1, generator=gen) ** (1.0 / 3.0)
    # the centres are a subset of the points where the cloud has that many: d = 0 occurs
    if N >= G:
        pts = pts[:, :N].contiguous()
        pick = torch.stack([torch.randperm(N, generator=gen)[:G] for _ in range(B)])
        center = R.gather_rows(pts, pick)
    else:                                                    # fewer points than centres: the points are the first centres
        center = pts[:, :G].contiguous()
        pts = pts[:, :N].contiguous()
    F = torch.randn(B, G, K, generator=gen)
    w0 = torch.randn(C, 3 + K, generator=gen) / (3 + K) ** 0.5
    b0 = 0.1 * torch.randn(C, generator=gen)
    sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
    scale = sign * (1.0 + 0.1 * torch.randn(C, generator=gen))
    shift = 0.3 * torch.randn(C, generator=gen)
    for c in DEAD:
        scale[c], shift[c] = 0.5, -1000.0
    want, idx = R.propagate_first_layer(pts.double(), center.double(), F.double(), w0.double(), b0.double(), scale.double(),
                                        shift.double())
    return pts, center, F, w0, b0, scale, shift, want.reshape(B * N, C), idx, R.third_fourth_gap(pts, center)


def run_propagate(dims):
    from point_dae_amd import partseg_ops
    from point_dae_amd.rows import rows_gemm
    B, N, G, C = dims
    pts, center, F, w0, b0, scale, shift = (t.cuda() for t in prop_case(*dims)[:7])
    T = rows_gemm(F.reshape(B * G, -1).contiguous(), w0[:, 3:].contiguous(), bias=b0)
    a0, idx = partseg_ops.propagate(pts, center, T, w0[:, :3], scale, shift, want_idx=True)
    torch.cuda.synchronize()
    return a0, idx


def run_propagate_layers(dims):
    """The same layer on kernels that predate csrc/partseg.hip: three_nn, three_interpolate, the row GEMM."""
    from point_dae_amd.pointnet2_utils import three_interpolate, three_nn
    from point_dae_amd.rows import linear_any
    B, N, G, C = dims
    pts, center, F, w0, b0, scale, shift = (t.cuda() for t in prop_case(*dims)[:7])
    dist, idx = three_nn(pts, center)
    recip = 1.0 / (dist * dist + 1e-8)
    weight = (recip / recip.sum(2, keepdim=True)).contiguous()
    interp = three_interpolate(F.transpose(1, 2).contiguous(), idx, weight)
    x = torch.cat([pts.reshape(B * N, 3), interp.transpose(1, 2).reshape(B * N, -1)], 1)
    out = linear_any(x, (w0 * scale[:, None]).contiguous(), (b0 * scale + shift).contiguous(), relu=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dims', PROP_CASES, ids=lambda d: 'x'.join(str(v) for v in d))
def test_propagate_against_the_fp64_definition(dims):
    B, N, G, C = dims
    want, want_idx, gap = prop_case(*dims)[7:]
    assert gap >= MARGIN, gap                                # no point's third neighbour hangs on rounding: none is excluded
    got, idx = run_propagate(dims)
    err, e_layers = _rel(got, want), _rel(run_propagate_layers(dims), want)
    print('partseg_propagate %s: error %.3e, e_layers %.3e (ratio %.2f), least 3rd/4th gap %.2e'
          % (dims, err, e_layers, err / e_layers, gap))
    assert torch.equal(idx.cpu().long(), want_idx)           # the chosen three, nearest first, at EVERY point
    assert got.shape == want.shape
    assert err <= FACTOR * e_layers
    assert err <= PIN
    got = got.cpu()
    for c in DEAD:
        assert bool((got[:, c] == 0.0).all())
    assert bool(((got == 0) == (want == 0)).all())
    again, idx2 = run_propagate(dims)
    assert torch.equal(again.cpu(), got) and torch.equal(idx2, idx)


# ---- pdae_partseg_tail -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_case(S, N, ranges):
    gen = torch.Generator().manual_seed(77 * N + S)
    y = torch.randn(S * N, 256, generator=gen)
    sign = torch.where(torch.rand(256, generator=gen) < 0.5, -1.0, 1.0)
    scale = sign * (1.0 + 0.1 * torch.randn(256, generator=gen))
    shift = 0.3 * torch.randn(256, generator=gen)
    for c in DEAD:
        scale[c], shift[c] = 0.5, -1000.0
    w3 = torch.randn(50, 256, generator=gen) / 16.0
    b3 = 0.1 * torch.randn(50, generator=gen)
    # two identical rows inside each range: their log-probabilities tie exactly, the lower index must win
    w3[29], b3[29] = w3[28], b3[28]
    w3[33], b3[33] = w3[31], b3[31]
    lo = torch.tensor([r[0] for r in ranges], dtype=torch.int32)
    hi = torch.tensor([r[1] for r in ranges], dtype=torch.int32)
    seg = torch.stack([torch.randint(r[0], r[1] + 1, (N,), generator=gen, dtype=torch.int32) for r in ranges])
    want = R.tail(y.double(), scale.double(), shift.double(), w3.double(), b3.double())
    return y, scale, shift, w3, b3, seg, lo, hi, want


def run_tail(dims):
    from point_dae_amd import partseg_ops
    S, N, ranges = dims
    y, scale, shift, w3, b3, seg, lo, hi = (t.cuda() for t in tail_case(*dims)[:8])
    counts = partseg_ops.Counts(S, y.device)
    logp, pred = partseg_ops.tail(y, scale, shift, w3, b3, S, N, seg, lo, hi, counts)
    torch.cuda.synchronize()
    counts.filled, counts.points = S, S * N
    return logp.cpu(), pred.cpu(), counts.read()


def run_tail_layers(dims):
    from point_dae_amd.rows import linear_any
    y, scale, shift, w3, b3 = (t.cuda() for t in tail_case(*dims)[:5])
    out = torch.log_softmax(linear_any(torch.relu(y * scale + shift), w3, b3), dim=1)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dims', TAIL_CASES, ids=lambda d: '%dx%d' % d[:2])
def test_tail_against_the_fp64_definition_and_exactly(dims):
    S, N, ranges = dims
    seg, want = tail_case(*dims)[5], tail_case(*dims)[-1]
    logp, pred, counts = run_tail(dims)
    err, e_layers = _rel(logp, want), _rel(run_tail_layers(dims), want)
    print('partseg_tail %dx%d: error %.3e, e_layers %.3e (ratio %.2f)' % (S, N, err, e_layers, err / e_layers))
    assert logp.shape == (S * N, 50) and logp.dtype == torch.float32
    assert err <= FACTOR * e_layers
    assert err <= PIN
    # the prediction is the restricted argmax of the RETURNED log-probabilities, first index on ties
    lp = logp.numpy().reshape(S, N, 50)
    want_pred = np.stack([R.restricted_argmax(lp[s], list(range(ranges[s][0], ranges[s][1] + 1))) for s in range(S)])
    assert np.array_equal(pred.numpy().reshape(S, N), want_pred)
    assert bool((lp[:, :, 28] == lp[:, :, 29]).all()) and bool((lp[:, :, 31] == lp[:, :, 33]).all())
    assert 29 not in want_pred and 33 not in want_pred
    # every count equals the numpy definition on those predictions
    classes = {'c%d' % s: list(range(r[0], r[1] + 1)) for s, r in enumerate(dict.fromkeys(ranges))}
    ref = R.metric(want_pred, seg.numpy(), classes)['counts']
    assert np.array_equal(counts['shape_iu'], ref['shape_iu'])
    assert np.array_equal(counts['shape_correct'], ref['shape_correct'])
    assert np.array_equal(counts['part_seen'], ref['part_seen'])
    assert np.array_equal(counts['part_correct'], ref['part_correct'])
    logp2, pred2, counts2 = run_tail(dims)
    assert torch.equal(logp2, logp) and torch.equal(pred2, pred)
    assert all(np.array_equal(counts2[k], counts[k]) for k in ('shape_iu', 'shape_correct', 'part_seen', 'part_correct'))


# ---- refusals and the fallback ---------------------------------------------------------------------------------------
def test_refused_layouts_return_unsupported_before_anything_is_read():
    from point_dae_amd import _lib, partseg_ops
    lib = _lib.lib()
    assert partseg_ops.supported(3, 64) and partseg_ops.supported(128, 1536) and partseg_ops.supported(256, 4)
    assert not partseg_ops.supported(2, 1536) and not partseg_ops.supported(257, 1536)
    assert not partseg_ops.supported(128, 1538) and not partseg_ops.supported(128, 1536, 128, 50)
    assert not partseg_ops.supported(128, 1536, 256, 40)
    unsupported = _lib.CONST['PDAE_ERR_UNSUPPORTED']
    for G, C in ((2, 1536), (128, 1538)):                    # null pointers: never looked at
        assert lib.pdae_partseg_propagate(2, 64, G, C, None, None, None, None, None, None, None, None, None) == unsupported
        assert b'partseg_propagate' in lib.pdae_last_error()
    for K, P in ((128, 50), (256, 40)):
        assert lib.pdae_partseg_tail(2, 64, K, P, *([None] * 14), None) == unsupported
        assert b'partseg_tail' in lib.pdae_last_error()


@functools.lru_cache(maxsize=None)
def small_model_case(cls_dim):
    """A small model whose layout the kernels refuse (cls_dim 40) or take (50), on a seeded B = 2, N = 96 cloud, and the fp64
    log-probabilities of the restatement on the model's own geometric decisions."""
    from point_dae_amd.synthetic import shapenet_like_clouds
    pts = torch.from_numpy(shapenet_like_clouds(2, 96, seed=9))
    cls = torch.tensor([3, 11])
    model = weights.fill_state(build_model(cls_dim=cls_dim, num_group=16, group_size=8), 12)
    return pts, cls, model


@pytest.mark.parametrize('cls_dim,used', [(40, 'layers'), (50, 'hip')])
def test_model_falls_back_to_layers_on_a_refused_layout(cls_dim, used, monkeypatch):
    monkeypatch.delenv('PDAE_PARTSEG', raising=False)
    pts, cls, model = small_model_case(cls_dim)
    model = model.cuda().eval()
    cap = {}
    logp = model(pts.cuda(), cls.cuda(), capture=cap)
    torch.cuda.synchronize()
    assert cap['partseg'] == used
    sd = {k: (v.double().cpu() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}
    want = R.forward(pts.double(), cls, sd, cap['fps_idx'].cpu(), cap['knn_idx'].cpu())
    assert R.third_fourth_gap(pts, want['center']) >= MARGIN
    assert torch.equal(cap['three_idx'].cpu().long(), want['three_idx'])
    err = _rel(logp, want['logp'])
    print('cls_dim %d (%s): log-probabilities vs fp64 %.3e' % (cls_dim, used, err))
    assert logp.shape == (2, 96, cls_dim) and err <= PIN


# ---- the model on the live-reference fixtures --------------------------------------------------------------------------
_measured = {}


@pytest.mark.parametrize('backend', ['layers', 'hip'])
@pytest.mark.parametrize('which', ['a', 'b'])
def test_model_on_the_live_reference_fixtures(which, backend, monkeypatch):
    monkeypatch.setenv('PDAE_PARTSEG', backend)
    f = fixture(which)
    model = weights.fill_state(build_model(), int(f['seed'])).cuda().eval()
    cap = {}
    logp = model(torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['cls']).cuda(), capture=cap)
    torch.cuda.synchronize()
    assert cap['partseg'] == backend
    assert torch.equal(cap['fps_idx'].cpu(), torch.from_numpy(f['fps_idx']))
    assert torch.equal(cap['knn_idx'].cpu(), torch.from_numpy(f['knn_idx']))
    assert torch.equal(cap['three_idx'].cpu(), torch.from_numpy(f['three_idx']))
    logp = logp.cpu()
    sub = torch.from_numpy(f['sub_idx']).long()
    got = torch.gather(logp, 1, sub.unsqueeze(-1).expand(-1, -1, 50))
    err = _rel(got, torch.from_numpy(f['logp64']))
    _measured[(which, backend)] = err
    print('partseg %s PDAE_PARTSEG=%s: log-probabilities vs reference fp64 %.3e (reference fp32 %.2e)'
          % (which, backend, err, float(f['dist'])))
    assert logp.shape == (2, 512, 50) and logp.dtype == torch.float32
    assert err <= PIN
    if backend == 'hip':
        assert err <= FACTOR * _measured[(which, 'layers')]
    # the full-range argmax agrees wherever the fp64 top-two gap is at least 100 times the measured error
    abs_err = err * float(f['scale64'])
    clear = torch.from_numpy(f['margin64'].astype(np.float64)) >= 100.0 * abs_err
    assert float(clear.double().mean()) >= 0.99
    assert torch.equal(logp.argmax(-1)[clear], torch.from_numpy(f['argmax64']).long()[clear])
    again = model(torch.from_numpy(f['pts']).cuda(), torch.from_numpy(f['cls']).cuda())
    assert torch.equal(again.cpu(), logp)                                # capture changes nothing; same bits twice


def test_model_in_training_mode_raises():
    model = build_model().cuda().train()
    with pytest.raises(NotImplementedError, match='training is not built'):
        model(torch.rand(2, 64, 3).cuda(), torch.zeros(2, dtype=torch.long).cuda())


# ---- the protocol ------------------------------------------------------------------------------------------------------
def _protocol(tmp_path, monkeypatch, want_pred=False):
    from point_dae_amd import parser, runner_finetune
    from point_dae_amd.config import get_config
    from point_dae_amd.misc import set_random_seed
    monkeypatch.chdir(ROOT)
    monkeypatch.setenv('LOCAL_RANK', '0')
    args = parser.get_args(['--config', CONFIG, '--part_seg', '--test', '--scratch_model', '--total_bs', '8', '--exp_name',
                            'ci_partseg', '--root_folder', os.path.relpath(str(tmp_path / 'exp'), ROOT)])
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
    assert [ln[len('eval mIoU of '):][:14].strip() for ln in cats] == sorted(partseg_ops.SEG_CLASSES)
    assert all(len(ln.split()) == 5 for ln in cats)
    final = [ln for ln in lines if ln.startswith('test Accuracy: ')]
    m = args.part_seg_metrics
    assert final == ['test Accuracy: %f  Class avg mIOU: %f   Inctance avg mIOU: %f'
                     % (m['accuracy'], m['class_avg_iou'], m['inctance_avg_iou'])]
    assert miou == m['inctance_avg_iou']
    # the four metrics equal the numpy definition on the model's own per-point predictions, taken through forward
    set_random_seed(args.seed)
    device = torch.device('cuda', torch.cuda.current_device())
    loader = runner_finetune._loader(config.dataset.test, device, args.seed, 0, 1, config.total_bs)
    set_random_seed(args.seed)
    model = builder.model_builder(config.model)
    model.load_model_from_ckpt(None, log=lambda s: None)
    model = model.to(device).eval()
    preds, segs = [], []
    for _, _, (points, cls, seg) in loader:
        logp = model(points, cls).cpu().numpy()
        seg = seg.cpu().numpy()
        cat_of = {l: c for c, ls in partseg_ops.SEG_CLASSES.items() for l in ls}
        preds.append(np.stack([R.restricted_argmax(logp[i], partseg_ops.SEG_CLASSES[cat_of[int(seg[i, 0])]])
                               for i in range(len(seg))]))
        segs.append(seg)
    ref = R.metric(np.concatenate(preds), np.concatenate(segs), partseg_ops.SEG_CLASSES)
    for key in ('accuracy', 'class_avg_accuracy', 'class_avg_iou', 'inctance_avg_iou'):
        np.testing.assert_allclose(m[key], ref[key], rtol=0, atol=1e-12, equal_nan=True, err_msg=key)
    for cat, v in ref['category_iou'].items():
        np.testing.assert_allclose(m['category_iou'][cat], v, rtol=0, atol=1e-12, err_msg=cat)
    lines2, miou2, _, _ = _protocol(tmp_path, monkeypatch)
    assert lines2 == lines and miou2 == miou
