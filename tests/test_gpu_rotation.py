"""The rotation-robustness fine-tuning protocol on the GPU: csrc/resample.hip (the subset + gather + per-cloud map of the
runner's batch preparation, one launch) against torch indexing, the existing resample() and an fp64 evaluation;
data_transforms.resample_transformed against the live-reference fixture and the reference's np.random order; the
--so3_rotation dispatch and the CLI end to end in a child process."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import proc_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rotate_transform_b4.npz')
CFG_NAME = 'finetune_modelnet_rotation_z2so3_officialmodelnet.yaml'
U = 2.0 ** -24
SMALL = dict(B=3, P=40, point_all=24, npoints=16)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case(B, P, point_all, npoints, C, seed):
    """raw (B,P,C) with one cloud of O(100) coordinates, exact and negative zeros; fps_idx (B,point_all) distinct indices
    per cloud; choice (npoints,) distinct FPS columns that include the zeros' rows -- all on the host."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand(B, P, C, generator=g) * 2 - 1
    raw[1] *= 100.0
    fps_idx = torch.stack([torch.randperm(P, generator=g)[:point_all] for _ in range(B)]).to(torch.int32)
    choice = torch.randperm(point_all, generator=g)[:npoints].to(torch.int32)
    for b in range(B):                                   # the first chosen point of every cloud: (-0, 0, -0)
        row = int(fps_idx[b, int(choice[0])])
        raw[b, row, 0], raw[b, row, 1], raw[b, row, 2] = -0.0, 0.0, -0.0
    return raw, fps_idx, choice


def _gathered(raw, fps_idx, choice):
    """raw[b, fps_idx[b, choice], :3] with torch indexing."""
    cols = fps_idx.long()[:, choice.long()]
    return raw[torch.arange(raw.shape[0])[:, None], cols, :3]


def _maps(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 3, generator=g), torch.randn(B, 3, generator=g)


def _check_map(got, x, A, t):
    """|got - fp64(x A + t)| <= 4 u (|x||A0j| + |y||A1j| + |z||A2j| + |tj|) elementwise: gamma_4 of the four-term fp32 sum
    ((x A0j + y A1j) + z A2j) + tj -- no term is touched by more than four roundings (its product, up to three adds), and
    an fma only removes roundings.  x, A, t: the fp32 inputs on the host."""
    xd = x.double()
    Ad = A.double() if A is not None else torch.eye(3, dtype=torch.float64).expand(x.shape[0], 3, 3)
    want = torch.einsum('bni,bij->bnj', xd, Ad)
    mag = torch.einsum('bni,bij->bnj', xd.abs(), Ad.abs())
    if t is not None:
        want, mag = want + t.double()[:, None, :], mag + t.double().abs()[:, None, :]
    err, bound = (got.double().cpu() - want).abs(), 4 * U * mag
    print('map path: max err / bound = %.3f' % (err / bound.clamp_min(1e-300)).max().item())
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.fixture(scope='module')
def big():
    """B=2, P=1300 -> the table's 1200 FPS points -> 1024: four blocks per cloud, FPS run once for the module."""
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    from point_dae_amd.synthetic import shapenet_like_clouds
    pts = torch.from_numpy(shapenet_like_clouds(2, 1300, seed=9))
    pts[1] *= 100.0
    pts[0, 5], pts[1, 7, 1] = torch.tensor([-0.0, 0.0, -0.0]), -0.0
    dev = pts.cuda()
    choice = np.random.default_rng(4).choice(1200, 1024, False)
    return dict(host=pts, dev=dev, fps_idx=furthest_point_sample(dev, 1200), choice=choice)


@pytest.mark.parametrize('C', [3, 6])
def test_identity_path_is_the_indexed_gather_bit_for_bit(C):
    from point_dae_amd.data_transforms import resample_affine
    raw, fps_idx, choice = _case(C=C, seed=C, **SMALL)
    got = resample_affine(raw.cuda(), fps_idx.cuda(), choice.cuda())
    want = _gathered(raw, fps_idx, choice)
    assert tuple(got.shape) == (3, 16, 3)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_bits(got.cpu()), _bits(want))          # signed zeros included
    assert (_bits(want) == _bits(torch.tensor(-0.0))).any()


def test_identity_path_equals_resample_through_the_table(big):
    from point_dae_amd.data_transforms import resample_transformed
    from point_dae_amd.runner_finetune import resample
    want = resample(big['dev'], 1024, big['choice'])
    got = resample_transformed(big['dev'], 1024, None, big['choice'])
    assert tuple(got.shape) == (2, 1024, 3)
    assert torch.equal(_bits(got), _bits(want))
    ref = _gathered(big['host'], big['fps_idx'].cpu(), torch.from_numpy(big['choice']))
    assert torch.equal(_bits(got.cpu()), _bits(ref))


@pytest.mark.parametrize('C', [3, 6])
@pytest.mark.parametrize('use', ['A+t', 'A', 't'])
def test_map_path_small(C, use):
    from point_dae_amd.data_transforms import resample_affine
    raw, fps_idx, choice = _case(C=C, seed=10 + C, **SMALL)
    A, t = _maps(3, 5)
    A, t = (A if 'A' in use else None), (t if 't' in use else None)
    got = resample_affine(raw.cuda(), fps_idx.cuda(), choice.cuda(), None if A is None else A.cuda(),
                          None if t is None else t.cuda())
    _check_map(got, _gathered(raw, fps_idx, choice), A, t)


def test_map_path_across_blocks(big):
    from point_dae_amd.data_transforms import resample_affine
    A, t = _maps(2, 6)
    choice = torch.from_numpy(big['choice']).to(torch.int32)
    got = resample_affine(big['dev'], big['fps_idx'], choice.cuda(), A.cuda(), t.cuda())
    _check_map(got, _gathered(big['host'], big['fps_idx'].cpu(), choice), A, t)


def test_out_buffer_is_written_and_nothing_around_it():
    from point_dae_amd.data_transforms import resample_affine
    raw, fps_idx, choice = _case(C=3, seed=21, **SMALL)
    A, t = _maps(3, 7)
    whole = torch.full((3 + 2, 16, 3), 777.0, device='cuda')
    out = whole[1:4]
    ret = resample_affine(raw.cuda(), fps_idx.cuda(), choice.cuda(), A.cuda(), t.cuda(), out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert (whole[0] == 777.0).all() and (whole[4] == 777.0).all()
    fresh = resample_affine(raw.cuda(), fps_idx.cuda(), choice.cuda(), A.cuda(), t.cuda())
    assert torch.equal(_bits(out), _bits(fresh))
    with pytest.raises(ValueError, match='out'):
        resample_affine(raw.cuda(), fps_idx.cuda(), choice.cuda(), out=whole[:2])


def test_rejected_arguments_raise_with_the_library_message():
    from point_dae_amd.data_transforms import resample_affine
    raw, fps_idx, choice = _case(C=3, seed=22, **SMALL)
    out = torch.full((3, 16, 3), 777.0, device='cuda')
    with pytest.raises(RuntimeError, match=r'pdae_resample_affine failed.*c >= 3'):
        resample_affine(raw[:, :, :2].contiguous().cuda(), fps_idx.cuda(), choice.cuda(), out=out)
    many = torch.arange(25, dtype=torch.int32).cuda() % 24           # 25 columns of 24 FPS points
    with pytest.raises(RuntimeError, match=r'pdae_resample_affine failed.*npoints > point_all'):
        resample_affine(raw.cuda(), fps_idx.cuda(), many, out=torch.full((3, 25, 3), 777.0, device='cuda'))
    torch.cuda.synchronize()
    assert (out == 777.0).all()                                      # nothing was launched


def test_fixture_on_the_device(monkeypatch):
    """The live reference's PointcloudRotate output from resample_transformed at P = point_all = npoints = 64 with the
    columns in FPS order (choice = arange): row n of cloud b is the reference's row fps_idx[b, n].  Both sides sum two
    non-zero fp32 products per coordinate (the y-axis rotation's zeros and one add exactly), so each is within 2 u of the
    exact value and the two within the four-term bound of each other."""
    from point_dae_amd import runner_finetune
    from point_dae_amd.data_transforms import PointcloudRotate, resample_transformed
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    fx = np.load(GOLDEN)
    x, want = torch.from_numpy(fx['input']), torch.from_numpy(fx['output'])
    monkeypatch.setitem(runner_finetune.POINT_ALL, 64, 64)
    np.random.seed(int(fx['seed']))
    got = resample_transformed(x.cuda(), 64, PointcloudRotate(), choice=np.arange(64))
    assert np.random.uniform() == float(fx['next_uniform'])
    order = furthest_point_sample(x.cuda(), 64).cpu().long()
    assert all(sorted(order[b].tolist()) == list(range(64)) for b in range(4))
    rows = torch.arange(4)[:, None]
    np.random.seed(int(fx['seed']))
    A, _ = PointcloudRotate().draw(4)
    mag = torch.einsum('bni,bij->bnj', x[rows, order].double().abs(), A.double().abs())
    err = (got.double().cpu() - want[rows, order].double()).abs()
    print('fixture: max err / bound = %.3f' % (err / (4 * U * mag).clamp_min(1e-300)).max().item())
    assert (err <= 4 * U * mag).all()


def test_draw_order_is_the_references(big):
    """runner_finetune.py:416-420: np.random.choice for the subset FIRST, then one uniform per cloud."""
    from point_dae_amd.data_transforms import PointcloudRotate, resample_affine, resample_transformed
    np.random.seed(77)
    got = resample_transformed(big['dev'], 1024, PointcloudRotate())
    nxt = np.random.uniform()
    np.random.seed(77)
    choice = np.random.choice(1200, 1024, False)
    A, t = PointcloudRotate().draw(2)
    assert t is None and nxt == np.random.uniform()
    want = resample_affine(big['dev'], big['fps_idx'], torch.from_numpy(choice.astype(np.int32)).cuda(), A.cuda())
    assert torch.equal(_bits(got), _bits(want))


def test_scale_and_translate_through_the_kernel(big):
    """PointcloudScaleAndTranslate (the reference's test_transforms) is the same launch with a diagonal map and a shift."""
    from point_dae_amd.data_transforms import PointcloudScaleAndTranslate, resample_transformed
    np.random.seed(5)
    got = resample_transformed(big['dev'], 1024, PointcloudScaleAndTranslate(), big['choice'])
    np.random.seed(5)
    A, t = PointcloudScaleAndTranslate().draw(2)
    _check_map(got, _gathered(big['host'], big['fps_idx'].cpu(), torch.from_numpy(big['choice'])), A.cpu(), t.cpu())


# ---- runner ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flag,taken', [((), 'run_net'), (('--so3_rotation',), 'run_net_rotation')])
def test_main_dispatches_on_so3_rotation(tmp_path, monkeypatch, flag, taken):
    """main.py:96-107: with --scratch_model the flag selects run_net_rotation; without it run_net, as before."""
    from point_dae_amd import main, runner_finetune
    calls = []
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(runner_finetune, 'run_net', lambda args, config: calls.append('run_net'))
    monkeypatch.setattr(runner_finetune, 'run_net_rotation', lambda args, config: calls.append('run_net_rotation'))
    main.main(['--config', os.path.join(ROOT, 'cfgs', CFG_NAME), '--scratch_model', '--max_epoch', '0',
               '--steps_per_epoch', '2', '--total_bs', '4', *flag])
    assert calls == [taken]


def _run_main(tmp_path, cfg, extra=(), limit=300):
    """tests/test_gpu_runner.py's child: main in a fresh process of its own session under a time limit, killed with its
    descendants when it outlives it (proc_util.run); the experiment goes under tmp_path."""
    cfgdir = tmp_path / 'cfgs'
    cfgdir.mkdir(exist_ok=True)
    path = cfgdir / CFG_NAME
    yaml.safe_dump(cfg, open(path, 'w'))
    cmd = [sys.executable, '-m', 'point_dae_amd.main', '--config', os.path.join('cfgs', CFG_NAME), *extra,
           '--exp_name', 'ci']
    return proc_util.run(cmd, limit, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT))


def test_so3_rotation_cli_trains_and_validates(tmp_path):
    """z/SO(3) from scratch, one epoch (the loop runs to max_epoch inclusive) of two steps of four clouds, then the ten
    validation passes over eight test clouds."""
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'cfgs', CFG_NAME)))
    for subset in ('train', 'val', 'test'):
        node = cfg['dataset'][subset]
        node['_base_'] = os.path.join(ROOT, node['_base_'])
        node['others']['count'] = 8
    r = _run_main(tmp_path, cfg, ('--scratch_model', '--so3_rotation', '--max_epoch', '0', '--steps_per_epoch', '2',
                                  '--total_bs', '4'))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert 'step: hipGraph replay' in out, out[-1500:]
    assert 'PointcloudRotate' in out and 'validate_rotation' in out
    assert out.count('[Validation] EPOCH: 0') == 1
    acc = float(out.split('[Validation] EPOCH: 0  acc = ')[1].split()[0])
    assert 0.0 <= acc <= 100.0
    losses = [float(line.split('Loss = ')[1].split()[0]) for line in out.splitlines() if 'Loss = ' in line]
    assert len(losses) == 1 and np.isfinite(losses[0]), out
    assert '[Epoch 0/0][Batch 2/2]' in out
    assert list(tmp_path.glob('experiments/*/cfgs/ci/ckpt-last.pth'))
