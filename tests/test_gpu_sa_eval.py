"""pdae_sa_eval_forward (csrc/sa_eval.hip, point_dae_amd/sa_eval_ops.py): one evaluation-mode set-abstraction level as one
kernel, against its fp64 definition -- explicit grouped rows, three affine + ReLU layers, max
(tests/svmfeat_restatement.py sa_level, itself checked against the live reference in tests/test_svmfeat_cpu.py).

Yardstick: e_layers, the error against the same fp64 result of the kernels the layer-by-layer form runs on the same
case -- pdae_sa_group_rows -> pdae_conv_stats x 3 with the given affines -> pdae_bnrelu_group_max.  The new kernel is of
the same arithmetic class (fp32 products accumulated in fp32), so it must stay within 4 e_layers, the project's margin
for such a kernel (tests/test_gpu_m2ae.py), and within 1e-5 of the largest output, the project's pin for
evaluation-mode features.  Errors are max norms relative to the largest output.

Inputs: coordinates in the unit ball, non-negative off-centre features (they follow a ReLU), idx with repeats and one
group whose entries are all one point (a one-member ball), scales of both signs, and in every layer a few channels whose
shift makes every pre-activation negative.
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import svmfeat_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
PIN = 1e-5
#        B, N, np, ns, C0, C1, C2, C3
CASES = [(2, 64, 5, 32, 0, 64, 64, 128),          # centres not a multiple of a block's share
         (1, 40, 1, 32, 0, 64, 64, 128),          # one group: half a block
         (2, 96, 33, 64, 128, 128, 128, 256),     # level-2 widths
         (2, 96, 2, 64, 128, 128, 128, 256),
         (2, 64, 3, 64, 8, 64, 64, 128),          # the other nsample of each width
         (2, 96, 3, 32, 128, 128, 128, 256)]
DEAD = (1, 17, 40)                                # channels switched off in every layer


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


@functools.lru_cache(maxsize=None)
def case(B, N, npoint, ns, C0, C1, C2, C3):
    """Seeded inputs (CPU, fp32) and the fp64 result, computed once per case."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * npoint + ns + C0)
    direction = torch.randn(B, N, 3, generator=gen)
    xyz = direction / direction.norm(dim=-1, keepdim=True) * torch.rand(B, N, 1, generator=gen) ** (1.0 / 3.0)
    centres = torch.stack([torch.randperm(N, generator=gen)[:npoint] for _ in range(B)])
    new_xyz = R.gather_rows(xyz, centres)
    idx = torch.randint(0, N, (B, npoint, ns), generator=gen, dtype=torch.int32)
    idx[:, :, ns // 2:ns // 2 + 5] = idx[:, :, :5]                 # repeats inside every group
    idx[0, 0, :] = 7                                               # a one-member ball
    feats = torch.rand(B, N, C0, generator=gen) + 0.25 if C0 else None
    layers = []
    for cin, cout in ((3 + C0, C1), (C1, C2), (C2, C3)):
        w = torch.randn(cout, cin, generator=gen) / cin ** 0.5
        sign = torch.where(torch.rand(cout, generator=gen) < 0.5, -1.0, 1.0)
        scale = sign * (1.0 + 0.1 * torch.randn(cout, generator=gen))
        shift = 0.3 * torch.randn(cout, generator=gen)
        for c in DEAD:
            scale[c], shift[c] = 0.5, -1000.0
        layers.append((w, scale, shift))
    want = R.sa_level(xyz.double(), new_xyz.double(), idx, feats.double() if C0 else None,
                      [tuple(t.double() for t in layer) for layer in layers])
    return xyz, new_xyz, idx, feats, layers, want.reshape(B * npoint, C3)


def _device(B, N, npoint, ns, C0, C1, C2, C3):
    xyz, new_xyz, idx, feats, layers, want = case(B, N, npoint, ns, C0, C1, C2, C3)
    rows = feats.reshape(B * N, C0).cuda() if C0 else None
    return xyz.cuda(), new_xyz.cuda(), idx.cuda(), rows, [tuple(t.cuda() for t in layer) for layer in layers], want


def run_new(dims):
    from point_dae_amd import sa_eval_ops
    xyz, new_xyz, idx, rows, layers, _ = _device(*dims)
    out = sa_eval_ops.forward(xyz, new_xyz, idx, rows, layers)
    torch.cuda.synchronize()
    return out


def run_layers(dims):
    """The kernels of the layer-by-layer form on the same case, with the given affines in place of batch statistics."""
    from point_dae_amd import _lib
    from point_dae_amd.rows import empty, insert_zero_col
    B, N, npoint, ns, C0, C1, C2, C3 = dims
    xyz, new_xyz, idx, rows, layers, _ = _device(*dims)
    M = B * npoint * ns
    x = empty((M, 4 + C0), xyz)
    _lib.call('pdae_sa_group_rows', xyz, B, N, npoint, ns, C0, _lib.ptr(xyz), _lib.ptr(new_xyz), _lib.ptr(idx), _lib.ptr(rows),
              _lib.ptr(x))
    sc = sh = None
    for i, (w, scale, shift) in enumerate(layers):
        w = (insert_zero_col(w, 3) if i == 0 else w).contiguous()
        y = empty((M, w.shape[0]), x)
        stats = empty((8, 2, w.shape[0]), x)
        _lib.call('pdae_conv_stats', x, M, w.shape[0], w.shape[1], _lib.ptr(x), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(w),
                  _lib.ptr(y), _lib.ptr(stats))
        x, sc, sh = y, scale.contiguous(), shift.contiguous()
    out = empty((B * npoint, C3), x)
    arg = empty((B * npoint, C3), x, torch.uint8)
    _lib.call('pdae_bnrelu_group_max', x, B * npoint, ns, C3, _lib.ptr(x), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(out),
              _lib.ptr(arg))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dims', CASES, ids=lambda d: 'x'.join(str(v) for v in d))
def test_sa_eval_forward_against_the_fp64_definition(dims):
    want = case(*dims)[-1]
    got = run_new(dims)
    err, e_layers = _rel(got, want), _rel(run_layers(dims), want)
    print('sa_eval %s: error %.3e, e_layers %.3e (ratio %.2f)' % (dims, err, e_layers, err / e_layers))
    assert got.shape == want.shape
    assert err <= FACTOR * e_layers
    assert err <= PIN
    got = got.cpu()
    assert bool((got[:, list(DEAD)] == 0).all())               # dead channels: exactly 0.0
    assert bool((got >= 0).all())


@pytest.mark.parametrize('dims', [CASES[0], CASES[2]], ids=['level1', 'level2'])
def test_two_launches_give_the_same_bits(dims):
    assert torch.equal(run_new(dims), run_new(dims))


def test_supported_layouts_and_refusals():
    from point_dae_amd import _lib, sa_eval_ops
    assert sa_eval_ops.supported(32, (0, 64, 64, 128))         # level 1
    assert sa_eval_ops.supported(64, (128, 128, 128, 256))     # level 2
    unsupported = _lib.CONST['PDAE_ERR_UNSUPPORTED']
    for ns, widths in ((48, (0, 64, 64, 128)), (64, (128, 128, 128, 512)), (32, (0, 64, 128, 128)), (16, (0, 64, 64, 128))):
        assert not sa_eval_ops.supported(ns, widths)
        # refused before anything is read or launched: the null pointers are never looked at
        rc = _lib.lib().pdae_sa_eval_forward(2, 64, 5, ns, *widths, *([None] * 14), None)
        assert rc == unsupported, (ns, widths, rc)
        assert b'sa_eval' in _lib.lib().pdae_last_error()
    xyz, new_xyz, idx, rows, layers, _ = _device(*CASES[0])
    with pytest.raises(RuntimeError, match='status -3'):
        sa_eval_ops.forward(xyz, new_xyz, idx[:, :, :16].contiguous(), rows, layers)


@pytest.mark.parametrize('nsample,mlp', [(48, [0, 64, 64, 128]), (32, [0, 64, 64, 512])], ids=['ns48', 'C3_512'])
def test_module_falls_back_to_layers_on_a_refused_layout(nsample, mlp):
    """A level the kernel refuses takes the layer-by-layer form inside the fused-eval module and still matches fp64."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import weights
    from point_dae_amd import sa_eval_ops
    from point_dae_amd.point_cae_pointnetv2 import PointnetSAModule
    torch.manual_seed(0)
    sa = PointnetSAModule(npoint=9, radius=0.6, nsample=nsample, mlp=list(mlp), fused_eval=True)
    sa = weights.fill_state(sa, 11).cuda().eval()
    assert not sa_eval_ops.supported(nsample, [0] + mlp[1:])
    xyz = case(*CASES[0])[0].cuda()
    cap = {}
    with torch.no_grad():
        new_xyz, out = sa(xyz, None, cap)
    sd = {'sa.' + k: v.double().cpu() for k, v in sa.state_dict().items() if v.is_floating_point()}
    want = R.sa_level(xyz.double().cpu(), new_xyz.double().cpu(), cap['ball_idx'].cpu(), None, R.level_layers(sd, 'sa'))
    err = _rel(out, want.reshape(out.shape))
    print('fallback ns %d C3 %d: error %.3e' % (nsample, mlp[-1], err))
    assert err <= PIN


def test_group_all_level_against_fp64():
    """The last level (one group per cloud) on the existing kernels with the running-estimate affines."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import weights
    from point_dae_amd import sa_eval_ops
    from point_dae_amd.point_cae_pointnetv2 import PointnetSAModule
    sa = weights.fill_state(PointnetSAModule(mlp=[256, 256, 512, 1024], fused_eval=True), 5).cuda().eval()
    gen = torch.Generator().manual_seed(3)
    xyz = torch.rand(3, 128, 3, generator=gen) - 0.5
    feats = torch.rand(3, 128, 256, generator=gen)
    with torch.no_grad():
        got = sa_eval_ops.group_all(xyz.cuda(), feats.reshape(-1, 256).cuda(), list(sa.mlps[0]))
        _, via_module = sa(xyz.cuda(), feats.reshape(-1, 256).cuda())
    sd = {'sa.' + k: v.double().cpu() for k, v in sa.state_dict().items() if v.is_floating_point()}
    want = R.group_all(xyz.double(), feats.double(), R.level_layers(sd, 'sa'))
    err = _rel(got, want)
    print('group-all level: error %.3e' % err)
    assert got.shape == (3, 1024) and err <= PIN and torch.equal(got, via_module)
