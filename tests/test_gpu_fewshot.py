"""Few-shot fine-tuning on the GPU: pdae_fewshot_batch (csrc/fewshot.hip) bit for bit against the existing FPS entry on the
materialised shuffle and against the CPU oracle through the host twin of its definition, its handling of bad indices, the
two backends of fewshot_ops on a synthetic episode, the per-fold validation point sets, and main end to end.

Nothing here has a tolerance: the kernel moves coordinates and picks indices, so every comparison is exact (indices with
torch.equal, coordinates on their int32 views, signed zeros included).
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fewshot_cpu import GRID_ROW, SKIP_ROW, tie_case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'cfgs', 'fewshot_modelnet_transferring_features.yaml')
SEED = 0           # tests/test_fewshot_cpu.py::test_the_tie_case_really_has_a_tie checks this seed on the host

# P: the T x P branch of the ladder it reaches; m, npoints, S clouds in the set, B rows
SHAPES = {'64x2_padding_lanes': dict(P=70, m=40, npoints=33, S=5, B=3),
          'multi_wave_slots': dict(P=300, m=120, npoints=100, S=5, B=3),
          '512x4': dict(P=1300, m=1200, npoints=1024, S=4, B=2),
          '1024x8_lds_limit': dict(P=8192, m=40, npoints=32, S=3, B=2)}


def _bits(t):
    return t.contiguous().view(torch.int32)


@contextlib.contextmanager
def _backend(name):
    old = os.environ.get('PDAE_FEWSHOT')
    os.environ['PDAE_FEWSHOT'] = name
    try:
        yield
    finally:
        if old is None:
            del os.environ['PDAE_FEWSHOT']
        else:
            os.environ['PDAE_FEWSHOT'] = old


def _choice(m, npoints, seed):
    """npoints distinct FPS columns, column 0 (the row's first point) among them."""
    choice = np.random.default_rng(seed).permutation(m)[:npoints]
    if 0 not in choice:
        choice[0] = 0
    return choice


def _expected(set_, item, perm, m):
    """The existing entry on the materialised shuffle -> (idx (B,m) int32, points (B,m,3))."""
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    sh = set_[item.long()][:, :, :3]
    if perm is not None:
        sh = torch.gather(sh, 1, perm.long().unsqueeze(-1).expand(-1, -1, 3))
    sh = sh.contiguous()
    f = furthest_point_sample(sh, m).long()
    idx = f if perm is None else perm.long().gather(1, f)
    return idx.to(torch.int32), torch.gather(sh, 1, f.unsqueeze(-1).expand(-1, -1, 3))


# ---- the kernel against the existing entry ---------------------------------------------------------------------------------

@pytest.mark.parametrize('with_slot', [True, False], ids=['slot', 'noslot'])
@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'noperm'])
@pytest.mark.parametrize('C', [3, 6])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_kernel_equals_the_existing_fps_on_the_materialised_shuffle(shape, C, with_perm, with_slot):
    from point_dae_amd import fewshot_ops
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    s = SHAPES[shape]
    P, m, B = s['P'], s['m'], s['B']
    set_h, item_h, perm_h = tie_case(P, s['S'], B, C, SEED)
    set_, item = torch.from_numpy(set_h).cuda(), torch.from_numpy(item_h).cuda()
    perm = torch.from_numpy(perm_h).cuda() if with_perm else None
    want_idx, want_pts = _expected(set_, item, perm, m)
    if with_perm:
        # the tie case really has a tie: started from the SAME point, FPS of the shuffled grid cloud picks other indices
        # than FPS of the cloud in its stored order (only the tie order by position can do that); and, as the issue
        # states it, the expected indices differ from those of the unshuffled FPS
        plain = furthest_point_sample(set_[item.long()][:, :, :3].contiguous(), m)
        assert any(not torch.equal(want_idx[b], plain[b]) for b in range(B))
        g, start = GRID_ROW, int(perm_h[GRID_ROW, 0])
        rolled = torch.from_numpy(np.concatenate([[start], np.delete(np.arange(P), start)]).astype(np.int32)[None]).cuda()
        same_start, _ = _expected(set_, item[g:g + 1], rolled, m)
        assert same_start[0, 0] == want_idx[g, 0] and not torch.equal(same_start[0], want_idx[g])
    if with_slot:
        npoints = s['npoints']
        choice = _choice(m, npoints, SEED + 1)
        slot = torch.from_numpy(fewshot_ops.slot_of(choice, m)).cuda()
        want_out = want_pts[:, torch.from_numpy(choice).cuda().long()]
    else:
        npoints, choice, slot, want_out = m, np.arange(m), None, want_pts
    out = torch.full((B, npoints, 3), 7.0, device='cuda')
    got_out, got_idx = fewshot_ops.fewshot_batch(set_, item, m, npoints, perm=perm, slot=slot, out=out, want_idx=True)
    assert got_out is out
    assert torch.equal(got_idx, want_idx)
    assert torch.equal(_bits(out), _bits(want_out))
    if with_perm:          # the row that starts at the (-0, 0, -0) point: chosen as index 0, moved with its signs
        row = int(np.flatnonzero(choice == 0)[0])
        assert torch.signbit(out[SKIP_ROW, row]).tolist() == [True, False, True]
        xyz = set_h[item_h[SKIP_ROW], :, :3]
        assert (xyz[want_idx[SKIP_ROW].cpu().numpy()[1:]] ** 2).sum(1).min() > 1e-3        # no other skipped point
    # idx is optional
    out2 = torch.full((B, npoints, 3), 7.0, device='cuda')
    assert fewshot_ops.fewshot_batch(set_, item, m, npoints, perm=perm, slot=slot, out=out2)[1] is None
    assert torch.equal(_bits(out2), _bits(want_out))


# ---- the kernel against the CPU oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'noperm'])
@pytest.mark.parametrize('shape', ['64x2_padding_lanes', 'multi_wave_slots'])
def test_kernel_equals_the_host_twin_over_the_cpu_oracle(oracle_ops, shape, with_perm):
    from point_dae_amd import fewshot_ops
    s = SHAPES[shape]
    set_h, item_h, perm_h = tie_case(s['P'], s['S'], s['B'], 6, SEED)
    perm_h = perm_h if with_perm else None
    want_idx, want_pts = fewshot_ops.batch_host(set_h, item_h, perm_h, s['m'], oracle_ops.furthest_point_sample)
    out, idx = fewshot_ops.fewshot_batch(torch.from_numpy(set_h).cuda(), torch.from_numpy(item_h).cuda(), s['m'], s['m'],
                                         perm=None if perm_h is None else torch.from_numpy(perm_h).cuda(), want_idx=True)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(out.cpu().numpy().view(np.int32), np.ascontiguousarray(want_pts).view(np.int32))


# ---- bad indices ---------------------------------------------------------------------------------------------------------------

def _small_case():
    s = SHAPES['multi_wave_slots']
    set_h, item_h, perm_h = tie_case(s['P'], s['S'], s['B'], 3, SEED)
    return s, torch.from_numpy(set_h).cuda(), torch.from_numpy(item_h).cuda(), torch.from_numpy(perm_h).cuda()


@pytest.mark.parametrize('bad', [99, -1, 5])
def test_item_out_of_range_marks_its_row_and_leaves_the_others_exact(bad):
    from point_dae_amd import fewshot_ops
    s, set_, item, perm = _small_case()
    m = s['m']
    good_out, good_idx = fewshot_ops.fewshot_batch(set_, item, m, m, perm=perm, want_idx=True)
    item2 = item.clone()
    item2[1] = bad                                         # (5 == S: the first index behind the set)
    out, idx = fewshot_ops.fewshot_batch(set_, item2, m, m, perm=perm, want_idx=True)
    torch.cuda.synchronize()
    assert torch.isnan(out[1]).all() and (idx[1] == -1).all()
    for b in (0, 2):
        assert torch.equal(idx[b], good_idx[b]) and torch.equal(_bits(out[b]), _bits(good_out[b]))


def test_perm_entry_out_of_range_counts_as_a_skipped_point():
    from point_dae_amd import fewshot_ops
    s, set_, item, perm = _small_case()
    P, m = s['P'], s['m']
    perm2 = perm.clone()
    perm2[GRID_ROW, 5], perm2[GRID_ROW, 200], perm2[2, 64] = P, -3, 2 ** 31 - 1
    # expected: the existing entry on the shuffle whose positions behind a bad entry hold (0, 0, 0) -- inside the skip
    # radius, so never selected
    from point_dae_amd.pointnet2_utils import furthest_point_sample
    ok = (perm2 >= 0) & (perm2 < P)
    sh = torch.gather(set_[item.long()], 1, perm2.clamp(0, P - 1).long().unsqueeze(-1).expand(-1, -1, 3))
    sh = (sh * ok.unsqueeze(-1)).contiguous()
    f = furthest_point_sample(sh, m).long()
    out, idx = fewshot_ops.fewshot_batch(set_, item, m, m, perm=perm2, want_idx=True)
    torch.cuda.synchronize()                               # the call returns normally
    assert torch.equal(idx, perm2.long().gather(1, f).to(torch.int32))
    assert torch.equal(_bits(out), _bits(torch.gather(sh, 1, f.unsqueeze(-1).expand(-1, -1, 3))))
    assert bool(ok.gather(1, f).all())                     # no bad position was picked


def test_slot_out_of_range_writes_nothing():
    from point_dae_amd import fewshot_ops
    s, set_, item, perm = _small_case()
    m, npoints = s['m'], s['npoints']
    choice = _choice(m, npoints, SEED + 1)
    slot_h = fewshot_ops.slot_of(choice, m)
    good = fewshot_ops.fewshot_batch(set_, item, m, npoints, perm=perm, slot=torch.from_numpy(slot_h).cuda())[0]
    slot_bad = slot_h.copy()
    rows = [int(slot_h[choice[3]]), int(slot_h[choice[50]])]                 # = 3 and 50
    slot_bad[choice[3]], slot_bad[choice[50]] = npoints, -7
    unused = np.flatnonzero(slot_h == -1)
    slot_bad[unused[0]] = npoints + 1000
    out = torch.full((s['B'], npoints, 3), 7.0, device='cuda')
    fewshot_ops.fewshot_batch(set_, item, m, npoints, perm=perm, slot=torch.from_numpy(slot_bad).cuda(), out=out)
    torch.cuda.synchronize()
    keep = torch.ones(npoints, dtype=torch.bool, device='cuda')
    keep[rows] = False
    assert torch.equal(_bits(out[:, keep]), _bits(good[:, keep]))
    assert (out[:, ~keep] == 7.0).all()


def test_argument_checks():
    from point_dae_amd import fewshot_ops
    s, set_, item, perm = _small_case()
    with pytest.raises(RuntimeError, match='npoints must equal m'):
        fewshot_ops.fewshot_batch(set_, item, 40, 33)
    with pytest.raises(RuntimeError, match='m > p'):
        fewshot_ops.fewshot_batch(set_, item, s['P'] + 1, s['P'] + 1)
    with pytest.raises(RuntimeError, match='8192'):
        fewshot_ops.fewshot_batch(torch.zeros(1, 8193, 3, device='cuda'), item[:1], 8, 8)
    with pytest.raises(RuntimeError, match='c >= 3'):
        fewshot_ops.fewshot_batch(torch.zeros(1, 64, 2, device='cuda'), item[:1], 8, 8)
    with pytest.raises(RuntimeError, match='int32'):
        fewshot_ops.fewshot_batch(set_, item.long(), 8, 8)


# ---- the two backends on a synthetic episode --------------------------------------------------------------------------------------

def _loader(subset, bs, seed=SEED):
    from point_dae_amd import datasets  # noqa: F401
    from point_dae_amd.registry import DATASETS
    return DATASETS.build(dict(NAME='ModelNetFewShot', DATA_PATH='no_such_directory', N_POINTS=1300, NUM_CATEGORY=40,
                               USE_NORMALS=False, subset=subset, bs=bs, way=3, shot=4, fold=0, seed=seed, device='cuda'))


def test_backends_make_bit_identical_training_batches():
    from point_dae_amd import runner_finetune

    def epochs(backend):
        with _backend(backend):
            np.random.seed(SEED)
            loader = _loader('train', 4)
            got = []
            for _ in range(2):
                for _, _, data in loader:
                    got.append((runner_finetune.fewshot_train_points(loader, data, 1024).clone(), data[2].clone()))
            return got, np.random.random()
    (hip, next_hip), (ref, next_ref) = epochs('hip'), epochs('torch')
    assert len(hip) == len(ref) == 6 and next_hip == next_ref             # the same host draws were consumed
    for (a, la), (b, lb) in zip(hip, ref):
        assert tuple(a.shape) == (4, 1024, 3) and torch.equal(_bits(a), _bits(b)) and torch.equal(la, lb)
    assert not torch.equal(hip[0][0], hip[3][0])                          # the second epoch is another shuffle


def test_hip_path_writes_the_step_input_in_place():
    from point_dae_amd import runner_finetune
    with _backend('hip'):
        loader = _loader('train', 4)
        data = next(iter(loader))[2]
        buf = torch.full((4, 1024, 3), float('nan'), device='cuda')
        assert runner_finetune.fewshot_train_points(loader, data, 1024, out=buf) is buf
        assert torch.isfinite(buf).all()


# ---- the validation point sets -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def scratch():
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    config = cfg_from_yaml_file(CFG)
    config.model.depth = 2
    torch.manual_seed(0)
    model = builder.model_builder(config.model)
    model.load_model_from_ckpt(None, log=lambda *a: None)
    return config, model.cuda().eval()


@pytest.mark.parametrize('backend', ['hip', 'torch'])
def test_validation_point_sets_equal_fps_of_the_test_batches(scratch, backend, monkeypatch):
    from point_dae_amd import runner_finetune
    from point_dae_amd.misc import fps
    config, model = scratch
    loader = _loader('test', 16)                                          # 60 clouds: three batches of 16 and one of 12
    with _backend(backend), torch.no_grad():
        sets = runner_finetune.fewshot_point_sets(loader, config.npoints)
        assert [tuple(p.shape) for p, _ in sets] == [(16, 1024, 3)] * 3 + [(12, 1024, 3)]
        for (points, label), (_, _, data) in zip(sets, loader):
            assert torch.equal(_bits(points), _bits(fps(data[0], config.npoints)[1])) and torch.equal(label, data[1])
        want_pred, want_label = runner_finetune._predict(model, loader, config)
        kept = []
        pred, label = runner_finetune._predict(model, loader, config, point_sets=kept)
        assert len(kept) == 4 and torch.equal(pred, want_pred) and torch.equal(label, want_label)
        # the second pass runs only the forward: no FPS of either kind

        def no_fps(*a, **k):
            raise AssertionError('FPS ran again')
        monkeypatch.setattr(runner_finetune, 'fps', no_fps)
        monkeypatch.setattr(runner_finetune, 'fewshot_point_sets', no_fps)
        pred2, _ = runner_finetune._predict(model, loader, config, point_sets=kept)
        assert torch.equal(pred2, want_pred)


# ---- main ------------------------------------------------------------------------------------------------------------------------

def _small_config(tmp_path):
    raw = yaml.safe_load(open(CFG))
    base = dict(NAME='ModelNetFewShot', DATA_PATH='no_such_directory', N_POINTS=1300, NUM_CATEGORY=40, USE_NORMALS=False)
    for subset in ('train', 'val', 'test'):
        raw['dataset'][subset] = dict(_base_=dict(base), others=dict(raw['dataset'][subset]['others']))
    raw['model']['depth'] = 2
    raw['max_epoch'] = 1
    raw['total_bs'] = 4
    cfg = tmp_path / 'fewshot.yaml'
    yaml.safe_dump(raw, open(cfg, 'w'))
    return cfg


def test_main_runs_a_fold_end_to_end(tmp_path):
    import proc_util
    cfg = _small_config(tmp_path)
    cmd = [sys.executable, '-m', 'point_dae_amd.main', '--config', str(cfg), '--scratch_model', '--way', '3', '--shot', '4',
           '--fold', '0', '--exp_name', 'f']
    env = {k: v for k, v in os.environ.items() if k != 'PDAE_FEWSHOT'}
    r = proc_util.run(cmd, 300, cwd=str(tmp_path), env=dict(env, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    lines = out.splitlines()
    assert 'args.way : 3' in lines and 'args.shot : 4' in lines and 'args.fold : 0' in lines
    assert 'Few-shot backend: hip' in out
    losses = [float(line.split('Loss = ')[1].split()[0]) for line in lines if line.startswith('[Epoch ') and 'Loss = ' in line]
    assert len(losses) == 2 and all(np.isfinite(losses)), out                # epochs 0 and 1, three batches each
    assert '[Batch 3/3]' in out
    assert out.count('[Validation] EPOCH: 0  acc = ') == 1 and out.count('[Validation] EPOCH: 1  acc = ') == 1
    acc = float(out.split('[Validation] EPOCH: 1  acc = ')[1].split()[0])
    assert 0.0 <= acc <= 100.0
    assert list(tmp_path.glob('experiments/*/*/f/ckpt-last.pth'))


def test_main_without_fold_fails_in_the_parser(tmp_path, monkeypatch):
    from point_dae_amd import main
    cfg = _small_config(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    with pytest.raises(ValueError, match='--way, --shot and --fold together'):
        main.main(['--config', str(cfg), '--scratch_model', '--way', '3', '--shot', '4'])
