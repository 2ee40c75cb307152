"""Point-M2AE as the linear-SVM feature extractor on the GPU (point_dae_amd/point_m2ae.py, csrc/m2ae.hip).

  * the masked attention core against its fp64 definition -- the explicit (B, T, T) additive mask of the reference,
    built from the case's centres and visible lengths -- within 4 e_old, where e_old is the error of the existing
    unmasked core (pdae_attention_forward) against fp64 at (B 2, T 64, H 6, D 64) on the same generator, measured in
    the same test.  The factor 4 covers key rows up to 8 times longer (an fp32 accumulation error grows roughly with
    sqrt 8).  Errors are max norms relative to the largest output.
  * the two token embedders against tests/m2ae_restatement.py in fp64: 1e-5 relative, the project's pin for
    evaluation-mode features (tests/test_gpu_dgcnn_cls.py).
  * the model on the live-reference fixtures tests/golden/m2ae_svmfeat_{a,b,c}.npz: len and T_pad per level exact, the
    feature within 1e-5 of the reference's fp64 feature (its own fp32 run sits 4e-7 to 6e-7 from it).
  * --svm_classification end to end on the synthetic ModelNet stand-in with a small pyramid.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import m2ae_restatement as R  # noqa: E402
import weights  # noqa: E402
from test_m2ae_cpu import CFG, FIXTURES, build_model, fixture  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
H = 6


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


def _qkv(gen, B, T, D):
    """Seeded (B*T, 3*H*D) rows [3][H][D]: q and k scaled so that the scores have a standard deviation near 2."""
    qkv = torch.randn(B, T, 3, H, D, generator=gen)
    qkv[:, :, :2] *= 2.0 ** 0.5
    return qkv


def _split64(qkv):
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)
    return q, k, v


_e_old = []


def e_old():
    """The yardstick: the unmasked core of the flat Transformer against fp64 at (2, 64, 6, 64)."""
    if not _e_old:
        from point_dae_amd import nn_ops
        gen = torch.Generator().manual_seed(1234)
        B, T, D = 2, 64, 64
        qkv = _qkv(gen, B, T, D)
        with torch.no_grad():
            o = nn_ops.attention_core(qkv.reshape(B * T, 3 * H * D).cuda(), B, T, H, D ** -0.5)
        q, k, v = _split64(qkv)
        want = R.attention(q, k, v, D ** -0.5, torch.zeros(B, T, T, dtype=torch.float64)).transpose(1, 2).reshape(B * T, H * D)
        _e_old.append(_rel(o, want))
    return _e_old[0]


ATTENTION_CASES = [
    (3, 72, 16, [72, 67, 72], 0.32),
    (2, 133, 16, [131, 133], 0.32),          # crosses a 128-row boundary, not a tile multiple
    (3, 29, 32, [29, 27, 29], 0.64),         # below one tile
    (2, 512, 16, [512, 505], 0.32),
    (2, 255, 32, [252, 255], 0.64),
    (2, 64, 64, [64, 64], 1.28),             # no padding
    (2, 40, 16, [40, 33], 0.0),              # valid rows compared, padded rows must be zero
    (1, 1, 16, [1], 0.32),
]


@pytest.mark.parametrize('B,T,D,lens,radius', ATTENTION_CASES)
def test_attention_local_against_the_fp64_definition(B, T, D, lens, radius):
    from point_dae_amd.point_m2ae import attention_local
    gen = torch.Generator().manual_seed(100 * T + D)
    qkv = _qkv(gen, B, T, D)
    # centres uniform in the unit ball (some inside, some outside the radius of the origin); padded rows zero
    direction = torch.randn(B, T, 3, generator=gen)
    cen = direction / direction.norm(dim=-1, keepdim=True) * torch.rand(B, T, 1, generator=gen) ** (1.0 / 3.0)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    valid = torch.arange(T).unsqueeze(0) < lens_t.unsqueeze(1)
    cen = cen * valid.unsqueeze(-1)
    if radius > 0:                       # no mask decision of the case hangs on rounding
        assert float((cen.double().norm(dim=-1) - radius).abs().min()) > 1e-6
    scale = D ** -0.5
    o = attention_local(qkv.reshape(B * T, 3 * H * D).cuda(), cen.reshape(B * T, 3).cuda(), lens_t.cuda(), B, T, H, scale,
                        radius)
    torch.cuda.synchronize()
    q, k, v = _split64(qkv)
    mask = R.attention_mask(cen.double(), lens_t.long(), radius)
    want = R.attention(q, k, v, scale, mask).transpose(1, 2).reshape(B, T, H * D)
    o = o.reshape(B, T, H * D).cpu()
    if radius == 0:
        assert bool((o[~valid] == 0).all())
        o, want = o[valid], want[valid]
    err, old = _rel(o, want), e_old()
    print('attention_local B %d T %d D %d radius %g: error %.3e, e_old %.3e (ratio %.2f)' % (B, T, D, radius, err, old, err / old))
    assert err <= FACTOR * old


def _small_model():
    return weights.fill_state(build_model([72, 40, 8], [16, 8, 4]), 7).cuda().eval()


def _sd64(model):
    return {k: (v.double().cpu() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}


def test_level0_embedder_against_the_restatement():
    from point_dae_amd.point_m2ae import token_embed_points
    model = _small_model()
    gen = torch.Generator().manual_seed(3)
    patches = 0.15 * torch.randn(3 * 72, 16, 3, generator=gen)
    with torch.no_grad():
        got = token_embed_points(model.h_encoder.token_embed[0], patches.cuda())
    want = R.token_embed(_sd64(model), 'h_encoder.token_embed.0', patches.double())
    print('level-0 embedder rel %.3e' % _rel(got, want))
    assert got.shape == (216, 96) and _rel(got, want) <= 1e-5


@pytest.mark.parametrize('level,S,P,k', [(1, 72, 40, 8), (2, 40, 8, 4)])
def test_merging_embedder_against_the_restatement(level, S, P, k):
    from point_dae_amd.point_m2ae import token_embed_merge
    model = _small_model()
    te = model.h_encoder.token_embed[level]
    gen = torch.Generator().manual_seed(10 + level)
    B = 3
    table = torch.randn(B * S, te.in_c, generator=gen)
    # an index table that repeats some sources and never references others (the top quarter of every sample)
    local = torch.randint(0, S - S // 4, (B, P * k), generator=gen)
    local[:, :3] = local[:, 3:6]
    idx = (local + torch.arange(B).unsqueeze(1) * S).reshape(-1)
    with torch.no_grad():
        got = token_embed_merge(te, table.cuda(), idx.cuda(), B * P, k)
    want = R.token_embed(_sd64(model), 'h_encoder.token_embed.%d' % level, table.double()[idx].reshape(B * P, k, -1))
    print('merging embedder level %d rel %.3e' % (level, _rel(got, want)))
    assert got.shape == (B * P, te.out_c) and _rel(got, want) <= 1e-5


@pytest.mark.parametrize('name', list(FIXTURES))
def test_model_on_the_live_reference_fixtures(name):
    num_groups, group_sizes, t_pads, visible = FIXTURES[name]
    f = fixture(name)
    model = weights.fill_state(build_model(num_groups, group_sizes), 7).cuda().eval()
    cap = {}
    feat = model(torch.from_numpy(f['pts']).cuda(), capture=cap)
    plain = model(torch.from_numpy(f['pts']).cuda())
    torch.cuda.synchronize()
    assert torch.equal(plain, feat)                  # the capture changes where the last branch is added, not the values
    dists = []
    for i in range(3):
        lv = cap['level%d' % i]
        assert lv['T_pad'] == t_pads[i] == int(f['T_pad%d' % i])
        assert lv['lens'].cpu().tolist() == visible[i] == f['len%d' % i].tolist()
        dists.append(_rel(lv['rows'][::7], torch.from_numpy(f['rows%d_sample' % i])))
    err = _rel(feat, torch.from_numpy(f['feature64']))
    print('%s: feature vs reference fp64 %.3e (reference fp32 %.2e); level output rows %s'
          % (name, err, float(f['dist']), ' '.join('%.2e' % d for d in dists)))
    assert feat.shape == f['feature64'].shape and err <= 1e-5, dists


def _protocol(tmp_path, monkeypatch, backend):
    from point_dae_amd import parser, runner_finetune
    from point_dae_amd.config import get_config
    from point_dae_amd.misc import set_random_seed
    monkeypatch.chdir(ROOT)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setenv('PDAE_SVM', backend)
    args = parser.get_args(['--config', 'cfgs/finetune_modelnet_svm_pointm2ae.yaml', '--scratch_model',
                            '--svm_classification', '--total_bs', '16', '--steps_per_epoch', '3', '--model_name',
                            'Point_M2AE_SVMFeature', '--exp_name', 'ci_' + backend, '--root_folder',
                            os.path.relpath(str(tmp_path / 'exp'), ROOT)])
    args.distributed, args.world_size, args.use_gpu = False, 1, True
    config = get_config(args)
    config.model.NAME = args.model_name
    config.model.num_groups, config.model.group_sizes = [72, 40, 8], [16, 8, 4]
    config.total_bs = args.total_bs
    config.dataset.train.others.bs = config.total_bs
    set_random_seed(args.seed)
    lines = []

    def log(s):
        print(s)
        lines.append(str(s))
    metric = runner_finetune.svm_classification(args, config, log=log)
    return lines, metric


def test_svm_protocol_runs_on_the_new_model(tmp_path, monkeypatch):
    lines, metric = _protocol(tmp_path, monkeypatch, 'hip')
    assert 'SVM backend: hip' in lines and '(48, 384)' in lines and '(256, 384)' in lines
    rows = [ln.split() for ln in lines if len(ln.split()) == 2 and ln.split()[0] in ('0.001', '0.01', '0.1', '1', '10', '100')]
    assert [r[0] for r in rows] == ['0.001', '0.01', '0.1', '1', '10', '100']
    accs = [float(r[1]) for r in rows]
    assert all(b >= a for a, b in zip(accs, accs[1:])) and 0.0 <= accs[-1] <= 1.0
    final = [ln for ln in lines if ln.startswith('[Validation] EPOCH: ')]
    assert len(final) == 1 and final[0].startswith('[Validation] EPOCH: 100  acc = ')
    assert abs(float(final[0].split('acc = ')[1]) - accs[-1]) < 5e-5
    lines2, metric2 = _protocol(tmp_path, monkeypatch, 'sklearn')
    assert 'SVM backend: sklearn' in lines2
    final2 = [ln for ln in lines2 if ln.startswith('[Validation] EPOCH: ')]
    assert final2 == final and metric2.acc == metric.acc
