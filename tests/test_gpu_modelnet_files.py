"""datasets.ModelNet on the reference's processed files, on the GPU: pdae_resident_batch (csrc/fewshot.hip) bit for bit
against the chain it replaces -- item select, permutation gather, pdae_pipeline_norm_affine, pdae_fewshot_batch --, against
pdae_fewshot_batch when it gets no maps and against the host twin over the CPU oracle's FPS; its handling of bad indices and
arguments; the two backends of resident_ops on a written .dat file, the kept validation point sets, and main end to end.

Nothing here has a tolerance: every comparison of coordinates and indices is exact (indices with torch.equal, coordinates on
their int32 views, signed zeros included).
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_modelnet_files_cpu import write_dat  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features.yaml')
SEED = 0

# the few-shot ladder's shapes -- P: the T x P branch it reaches; m, npoints, S clouds in the set; B = 4 rows everywhere, so
# that the rows' map counts are 0, 1, 2 and 3
SHAPES = {'64x2_padding_lanes': dict(P=70, m=40, npoints=33, S=5),
          'multi_wave_slots': dict(P=300, m=120, npoints=100, S=5),
          '512x4': dict(P=1300, m=1200, npoints=1024, S=4),
          '1024x8_lds_limit': dict(P=8192, m=40, npoints=32, S=3)}
B = 4
NMAPS = [2, 0, 3, 1]


def _bits(t):
    return t.contiguous().view(torch.int32)


@contextlib.contextmanager
def _backend(name):
    old = os.environ.get('PDAE_MODELNET')
    os.environ['PDAE_MODELNET'] = name
    try:
        yield
    finally:
        if old is None:
            del os.environ['PDAE_MODELNET']
        else:
            os.environ['PDAE_MODELNET'] = old


def _case(P, S, C, seed=SEED):
    """set (S,P,C) whose cloud 0 lies on the grid {-4..4}/4 (exact ties in d2 under a scale map too) and whose cloud 1 has a
    tenth of its points inside the skip radius, one of them (-0, 0, -0); item = [1, 0, 1, 2]; perm (4,P); nmaps = NMAPS and
    maps (4,3,12) drawn as the loader draws them -- scale, rotate (a dense M), translate."""
    from point_dae_amd.datasets import draw_affine_map
    rng = np.random.default_rng(seed)
    set_ = rng.uniform(-1, 1, (S, P, C)).astype(np.float32)
    set_[0, :, :3] = rng.integers(-4, 5, (P, 3)).astype(np.float32) / 4
    small = rng.choice(P, max(P // 10, 2), False)
    set_[1, small, :3] = rng.uniform(-0.01, 0.01, (small.size, 3)).astype(np.float32)
    set_[1, small[0], :3] = np.array([-0.0, 0.0, -0.0], np.float32)
    item = np.array([1, 0, 1, 2], np.int32)
    perm = np.stack([rng.permutation(P) for _ in range(B)]).astype(np.int32)
    maps = np.zeros((B, 3, 12), np.float32)
    maps[:, :, 0] = maps[:, :, 4] = maps[:, :, 8] = 1.0
    for b in range(B):
        for q, name in enumerate(('aug_scale', 'aug_rotate', 'aug_translate')[:NMAPS[b]]):
            M, t = draw_affine_map(rng, name)
            maps[b, q, :9], maps[b, q, 9:] = M.reshape(-1), t
    return tuple(torch.from_numpy(a).cuda() for a in (set_, item, perm, np.array(NMAPS, np.int32), maps))


def _choice(m, npoints, seed):
    choice = np.random.default_rng(seed).permutation(m)[:npoints]
    if 0 not in choice:
        choice[0] = 0
    return choice


def _chain(set_, item, perm, nmaps, maps, m, npoints, slot, bad=None, out=None):
    """The entries the kernel replaces: item select, permutation gather, pdae_pipeline_norm_affine(normalise = 0),
    pdae_fewshot_batch on the result.  bad (B,P) bool: positions that read as an unmapped (0,0,0).
    -> (out (B,npoints,3), idx (B,m) int32, mapped (B,P,3))."""
    from point_dae_amd import fewshot_ops
    from point_dae_amd.datasets import pipeline_norm_affine
    sh = set_.index_select(0, item.long())[:, :, :3]
    if perm is not None:
        P = set_.shape[1]
        sh = torch.gather(sh, 1, perm.clamp(0, P - 1).long().unsqueeze(-1).expand(-1, -1, 3))
    sh = sh.contiguous()
    if nmaps is not None:
        sh = pipeline_norm_affine(sh, False, (nmaps, maps))
    if bad is not None:
        sh = torch.where(bad.unsqueeze(-1), torch.zeros_like(sh), sh)
    rows = torch.arange(sh.shape[0], dtype=torch.int32, device=sh.device)
    out, f = fewshot_ops.fewshot_batch(sh, rows, m, npoints, slot=slot, out=out, want_idx=True)
    idx = f if perm is None else perm.gather(1, f.long())
    return out, idx, sh


# ---- the kernel against the chain ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_slot', [True, False], ids=['slot', 'noslot'])
@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'noperm'])
@pytest.mark.parametrize('C', [3, 6])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_kernel_equals_the_chain(shape, C, with_perm, with_slot):
    from point_dae_amd import fewshot_ops, resident_ops
    s = SHAPES[shape]
    m = s['m']
    set_, item, perm, nmaps, maps = _case(s['P'], s['S'], C)
    perm = perm if with_perm else None
    if with_slot:
        npoints = s['npoints']
        slot = torch.from_numpy(fewshot_ops.slot_of(_choice(m, npoints, SEED + 1), m)).cuda()
    else:
        npoints, slot = m, None
    want, want_idx, _ = _chain(set_, item, perm, nmaps, maps, m, npoints, slot, out=torch.full((B, npoints, 3), 7.0, device='cuda'))
    out = torch.full((B, npoints, 3), 7.0, device='cuda')
    got_out, got_idx = resident_ops.resident_batch(set_, item, m, npoints, perm=perm, nmaps=nmaps, maps=maps, slot=slot,
                                                   out=out, want_idx=True)
    assert got_out is out
    assert torch.equal(got_idx, want_idx)
    assert torch.equal(_bits(out), _bits(want))
    # the maps decide the picks: rows 0 and 2 (the cloud with skipped points, two and three maps) choose other points
    # than the unmapped FPS does, row 1 (no maps) the same
    plain = fewshot_ops.fewshot_batch(set_, item, m, m, perm=perm, want_idx=True)[1]
    assert torch.equal(got_idx[1], plain[1]) and not torch.equal(got_idx[0], plain[0])
    # idx is optional
    out2 = torch.full((B, npoints, 3), 7.0, device='cuda')
    assert resident_ops.resident_batch(set_, item, m, npoints, perm=perm, nmaps=nmaps, maps=maps, slot=slot, out=out2)[1] is None
    assert torch.equal(_bits(out2), _bits(want))


@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'noperm'])
def test_translate_across_the_skip_ball(with_perm):
    """Row 0's one map is a translate by t.  Stored point 5 = -t + (0.01, 0, 0) lands inside the skip ball (|.|^2 = 1e-4 <=
    1e-3) and is never selected; stored point 9 = (0.001, 0, 0), skipped as stored, lands at ~t and is selected.  With m = the
    number of selectable points (+ the first one), FPS picks every selectable point: the picked SET says who was skipped."""
    from point_dae_amd import resident_ops
    P, S = 70, 3
    rng = np.random.default_rng(7)
    t = np.array([0.5, 0.3, -0.4], np.float32)
    set_h = rng.uniform(-1, 1, (S, P, 3)).astype(np.float32)
    set_h[2, 5] = -t + np.array([0.01, 0, 0], np.float32)
    set_h[2, 9] = np.array([0.001, 0, 0], np.float32)
    item = torch.tensor([2, 2], dtype=torch.int32).cuda()
    nmaps = torch.tensor([1, 0], dtype=torch.int32).cuda()
    maps_h = np.zeros((2, 3, 12), np.float32)
    maps_h[:, :, 0] = maps_h[:, :, 4] = maps_h[:, :, 8] = 1.0
    maps_h[0, 0, 9:] = t
    maps, set_ = torch.from_numpy(maps_h).cuda(), torch.from_numpy(set_h).cuda()
    perm_h = np.stack([rng.permutation(P) for _ in range(2)]).astype(np.int32)
    for row in perm_h:                                         # position 0 holds neither of the two points
        at = int(np.flatnonzero(row == 0)[0])
        row[[0, at]] = row[[at, 0]]
    perm = torch.from_numpy(perm_h).cuda() if with_perm else None
    mag_moved = ((set_h[2].astype(np.float64) + t) ** 2).sum(1)
    mag_stored = (set_h[2].astype(np.float64) ** 2).sum(1)
    assert mag_moved[5] < 5e-4 and mag_moved[9] > 0.1 and mag_stored[9] < 5e-4 and mag_stored[5] > 0.1
    assert (np.delete(mag_moved, 5) > 2e-3).all() and (np.delete(mag_stored, 9) > 2e-3).all()   # nobody else near the ball
    m = P - 1
    want_out, want_idx, _ = _chain(set_, item, perm, nmaps, maps, m, m, None)
    out, idx = resident_ops.resident_batch(set_, item, m, m, perm=perm, nmaps=nmaps, maps=maps, want_idx=True)
    assert torch.equal(idx, want_idx) and torch.equal(_bits(out), _bits(want_out))
    assert sorted(idx[0].tolist()) == sorted(set(range(P)) - {5})             # moved into the ball: skipped
    assert sorted(idx[1].tolist()) == sorted(set(range(P)) - {9})             # the same cloud unmapped: the stored one is
    at9 = idx[0].tolist().index(9)
    assert torch.equal(out[0, at9], torch.from_numpy(set_h[2, 9] + t).cuda())  # out holds the mapped coordinates


@pytest.mark.parametrize('with_slot', [True, False], ids=['slot', 'noslot'])
@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'noperm'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_without_maps_it_is_the_fewshot_entry(shape, with_perm, with_slot):
    from point_dae_amd import fewshot_ops, resident_ops
    s = SHAPES[shape]
    m = s['m']
    set_, item, perm, _, maps = _case(s['P'], s['S'], 6)
    perm = perm if with_perm else None
    npoints = s['npoints'] if with_slot else m
    slot = torch.from_numpy(fewshot_ops.slot_of(_choice(m, npoints, SEED + 1), m)).cuda() if with_slot else None
    want = torch.full((B, npoints, 3), 7.0, device='cuda')
    _, want_idx = fewshot_ops.fewshot_batch(set_, item, m, npoints, perm=perm, slot=slot, out=want, want_idx=True)
    for given in (None, maps):                                  # maps without nmaps: no maps
        out = torch.full((B, npoints, 3), 7.0, device='cuda')
        _, idx = resident_ops.resident_batch(set_, item, m, npoints, perm=perm, maps=given, slot=slot, out=out, want_idx=True)
        assert torch.equal(idx, want_idx) and torch.equal(_bits(out), _bits(want))
    # and a row of zero maps among mapped rows is that row of the few-shot entry
    zeros = torch.zeros(B, dtype=torch.int32, device='cuda')
    out = torch.full((B, npoints, 3), 7.0, device='cuda')
    _, idx = resident_ops.resident_batch(set_, item, m, npoints, perm=perm, nmaps=zeros, maps=maps, slot=slot, out=out, want_idx=True)
    assert torch.equal(idx, want_idx) and torch.equal(_bits(out), _bits(want))


# ---- the kernel against the CPU oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'noperm'])
@pytest.mark.parametrize('shape', ['64x2_padding_lanes', 'multi_wave_slots'])
def test_kernel_equals_the_host_twin_over_the_cpu_oracle(oracle_ops, shape, with_perm):
    from point_dae_amd import resident_ops
    s = SHAPES[shape]
    m = s['m']
    set_, item, perm, nmaps, maps = _case(s['P'], s['S'], 6)
    perm = perm if with_perm else None
    want_idx, want_pts = resident_ops.batch_host(set_.cpu().numpy(), item.cpu().numpy(),
                                                 None if perm is None else perm.cpu().numpy(), nmaps.cpu().numpy(),
                                                 maps.cpu().numpy(), m, oracle_ops.furthest_point_sample)
    out, idx = resident_ops.resident_batch(set_, item, m, m, perm=perm, nmaps=nmaps, maps=maps, want_idx=True)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(out.cpu().numpy().view(np.int32), np.ascontiguousarray(want_pts).view(np.int32))


# ---- bad indices ---------------------------------------------------------------------------------------------------------------

def _small_case():
    s = SHAPES['multi_wave_slots']
    return (s,) + _case(s['P'], s['S'], 3)


@pytest.mark.parametrize('what,bad', [('item', 99), ('item', -1), ('item', 5), ('nmaps', 4), ('nmaps', -1), ('nmaps', 2 ** 31 - 1)])
def test_item_or_nmaps_out_of_range_marks_its_row_and_leaves_the_others_exact(what, bad):
    from point_dae_amd import resident_ops
    s, set_, item, perm, nmaps, maps = _small_case()
    m = s['m']
    good_out, good_idx = resident_ops.resident_batch(set_, item, m, m, perm=perm, nmaps=nmaps, maps=maps, want_idx=True)
    item2, nmaps2 = item.clone(), nmaps.clone()
    (item2 if what == 'item' else nmaps2)[2] = bad             # (5 == S: the first index behind the set)
    out, idx = resident_ops.resident_batch(set_, item2, m, m, perm=perm, nmaps=nmaps2, maps=maps, want_idx=True)
    torch.cuda.synchronize()
    assert torch.isnan(out[2]).all() and (idx[2] == -1).all()
    for b in (0, 1, 3):
        assert torch.equal(idx[b], good_idx[b]) and torch.equal(_bits(out[b]), _bits(good_out[b]))


def test_perm_entry_out_of_range_reads_as_an_unmapped_origin_and_is_never_selected():
    from point_dae_amd import resident_ops
    s, set_, item, perm, nmaps, maps = _small_case()
    P, m = s['P'], s['m']
    perm2 = perm.clone()
    perm2[0, 5], perm2[0, 200], perm2[2, 64], perm2[3, 17] = P, -3, 2 ** 31 - 1, -2 ** 31
    ok = (perm2 >= 0) & (perm2 < P)
    # rows 0, 2 and 3 carry a translate: a MAPPED origin would lie outside the skip ball and be selectable
    want_out, want_idx, _ = _chain(set_, item, perm2, nmaps, maps, m, m, None, bad=~ok)
    out, idx = resident_ops.resident_batch(set_, item, m, m, perm=perm2, nmaps=nmaps, maps=maps, want_idx=True)
    torch.cuda.synchronize()                                   # the call returns normally
    assert torch.equal(idx, want_idx)                          # (= perm2 at the picked positions)
    assert torch.equal(_bits(out), _bits(want_out))
    assert bool(((idx >= 0) & (idx < P)).all())                # no bad position was picked


def test_slot_out_of_range_writes_nothing():
    from point_dae_amd import fewshot_ops, resident_ops
    s, set_, item, perm, nmaps, maps = _small_case()
    m, npoints = s['m'], s['npoints']
    choice = _choice(m, npoints, SEED + 1)
    slot_h = fewshot_ops.slot_of(choice, m)
    good = resident_ops.resident_batch(set_, item, m, npoints, perm=perm, nmaps=nmaps, maps=maps,
                                       slot=torch.from_numpy(slot_h).cuda())[0]
    slot_bad = slot_h.copy()
    rows = [int(slot_h[choice[3]]), int(slot_h[choice[50]])]                 # = 3 and 50
    slot_bad[choice[3]], slot_bad[choice[50]] = npoints, -7
    slot_bad[np.flatnonzero(slot_h == -1)[0]] = npoints + 1000
    out = torch.full((B, npoints, 3), 7.0, device='cuda')
    resident_ops.resident_batch(set_, item, m, npoints, perm=perm, nmaps=nmaps, maps=maps,
                                slot=torch.from_numpy(slot_bad).cuda(), out=out)
    torch.cuda.synchronize()
    keep = torch.ones(npoints, dtype=torch.bool, device='cuda')
    keep[rows] = False
    assert torch.equal(_bits(out[:, keep]), _bits(good[:, keep]))
    assert (out[:, ~keep] == 7.0).all()


def test_argument_checks_launch_nothing():
    from point_dae_amd import resident_ops
    s, set_, item, perm, nmaps, maps = _small_case()
    out = torch.full((B, 8, 3), 7.0, device='cuda')
    with pytest.raises(RuntimeError, match='nmaps without maps'):
        resident_ops.resident_batch(set_, item, 8, 8, nmaps=nmaps, out=out)
    with pytest.raises(RuntimeError, match='npoints must equal m'):
        resident_ops.resident_batch(set_, item, 40, 8, nmaps=nmaps, maps=maps, out=out)
    with pytest.raises(RuntimeError, match='m > p'):
        resident_ops.resident_batch(set_, item, s['P'] + 1, s['P'] + 1, nmaps=nmaps, maps=maps)
    with pytest.raises(RuntimeError, match='8192'):
        resident_ops.resident_batch(torch.zeros(1, 8193, 3, device='cuda'), item[:1], 8, 8, nmaps=nmaps[:1], maps=maps[:1])
    with pytest.raises(RuntimeError, match='c >= 3'):
        resident_ops.resident_batch(torch.zeros(1, 64, 2, device='cuda'), item[:1], 8, 8, nmaps=nmaps[:1], maps=maps[:1])
    with pytest.raises(RuntimeError, match='int32'):
        resident_ops.resident_batch(set_, item, 8, 8, nmaps=nmaps.long(), maps=maps)
    with pytest.raises(ValueError, match='maps'):
        resident_ops.resident_batch(set_, item, 8, 8, nmaps=nmaps, maps=maps[:, :2].contiguous())
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- the loader on a written file: the two backends --------------------------------------------------------------------------

N_FILE = 1280


def _write_files(root):
    """16 training and 10 test clouds of 1280 points x 6, un-normalised, labels below 40."""
    rng = np.random.default_rng(3)
    train = [(rng.normal(size=(N_FILE, 6)) * 2 + 0.5).astype(np.float32) for _ in range(16)]
    test = [(rng.normal(size=(N_FILE, 6)) * 2 - 0.5).astype(np.float32) for _ in range(10)]
    write_dat(root, train, [(7 * k) % 40 for k in range(16)], 'train', 40, N_FILE)
    write_dat(root, test, [(11 * k) % 40 for k in range(10)], 'test', 40, N_FILE)


def _loader(root, subset, bs=4, seed=SEED, **kw):
    from point_dae_amd import datasets  # noqa: F401
    from point_dae_amd.registry import DATASETS
    c = dict(NAME='ModelNet', DATA_PATH=str(root), N_POINTS=N_FILE, NUM_CATEGORY=40, USE_NORMALS=False, subset=subset,
             npoints=N_FILE, bs=bs, seed=seed, device='cuda',
             aug_type=['norm', 'scale', 'translate'] if subset == 'train' else ['norm'])
    c.update(kw)
    return DATASETS.build(c)


def test_backends_make_bit_identical_training_batches(tmp_path):
    from point_dae_amd import runner_finetune
    _write_files(tmp_path)

    def epochs(backend):
        np.random.seed(SEED)
        loader = _loader(tmp_path, 'train')
        assert loader.listed and loader.resident and len(loader) == 4
        got = []
        for _ in range(2):
            if backend == 'hip':                               # the runner's two ways through a batch
                for _, _, data in loader.iter_draws():
                    buf = torch.full((4, 1024, 3), float('nan'), device='cuda')
                    assert runner_finetune.resident_train_points(loader, data, 1024, out=buf) is buf   # written in place
                    got.append((buf, data[4].clone()))
            else:
                for _, _, data in loader:
                    got.append((runner_finetune.resample(data[0], 1024), data[1].clone()))
        return got, np.random.random()
    (hip, next_hip), (ref, next_ref) = epochs('hip'), epochs('torch')
    assert len(hip) == len(ref) == 8 and next_hip == next_ref             # the same host draws were consumed
    for (a, la), (b, lb) in zip(hip, ref):
        assert tuple(a.shape) == (4, 1024, 3) and torch.isfinite(a).all()
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(la, lb)
    assert not torch.equal(hip[0][0], hip[4][0])                          # the second epoch is another shuffle
    assert sorted(torch.cat([l for _, l in hip[:4]]).tolist()) == sorted((7 * k) % 40 for k in range(16))


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
def test_kept_validation_point_sets_equal_fps_of_the_test_batches(scratch, backend, tmp_path, monkeypatch):
    from point_dae_amd import runner_finetune
    from point_dae_amd.misc import fps
    config, model = scratch
    _write_files(tmp_path)
    loader = _loader(tmp_path, 'test')                                    # 10 clouds: two batches of 4 and one of 2
    assert loader.listed and runner_finetune.fps_cacheable(loader)
    monkeypatch.setenv('PDAE_FEWSHOT', 'torch' if backend == 'hip' else 'hip')     # (not this loader's switch)
    with _backend(backend), torch.no_grad():
        sets = runner_finetune.fewshot_point_sets(loader, config.npoints)
        assert [tuple(p.shape) for p, _ in sets] == [(4, 1024, 3)] * 2 + [(2, 1024, 3)]
        for (points, label), (_, _, data) in zip(sets, loader):
            assert torch.equal(_bits(points), _bits(fps(data[0], config.npoints)[1])) and torch.equal(label, data[1])
        want_pred, want_label = runner_finetune._predict(model, loader, config)
        kept = []
        pred, label = runner_finetune._predict(model, loader, config, point_sets=kept)
        assert len(kept) == 3 and torch.equal(pred, want_pred) and torch.equal(label, want_label)
    # a train loader's augmentation is drawn per access: nothing of it may be kept
    assert not runner_finetune.fps_cacheable(_loader(tmp_path, 'train'))


# ---- main ------------------------------------------------------------------------------------------------------------------------

def _small_config(tmp_path):
    raw = yaml.safe_load(open(CFG))
    base = dict(NAME='ModelNet', DATA_PATH=str(tmp_path / 'data'), N_POINTS=N_FILE, NUM_CATEGORY=40, USE_NORMALS=False)
    for subset in ('train', 'val', 'test'):
        raw['dataset'][subset] = dict(_base_=dict(base), others=dict(raw['dataset'][subset]['others']))
    raw['model']['depth'] = 2
    raw['max_epoch'] = 1
    raw['total_bs'] = 4
    cfg = tmp_path / 'modelnet.yaml'
    yaml.safe_dump(raw, open(cfg, 'w'))
    return cfg


def test_main_trains_on_a_written_file_and_both_backends_print_the_same_losses(tmp_path):
    import proc_util
    _write_files(tmp_path / 'data')
    cfg = _small_config(tmp_path)
    outs = {}
    # --deterministic: the step's atomic reductions become ordered ones, so that two runs fed the same batches print the
    # same figures at all (without it AdamW's first updates amplify the reductions' order noise from run to run)
    for backend in ('hip', 'torch'):
        cmd = [sys.executable, '-m', 'point_dae_amd.main', '--config', str(cfg), '--scratch_model', '--steps_per_epoch', '3',
               '--deterministic', '--exp_name', backend]
        env = {k: v for k, v in os.environ.items() if k != 'PDAE_MODELNET'}
        if backend == 'torch':
            env['PDAE_MODELNET'] = 'torch'
        r = proc_util.run(cmd, 300, cwd=str(tmp_path), env=dict(env, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out = outs[backend] = r.stdout
        assert 'ModelNet backend: %s' % backend in out
        assert 'ModelNet train source: %s' % (tmp_path / 'data' / ('modelnet40_train_%dpts_fps.dat' % N_FILE)) in out
        assert '(12 clouds of %d points, 3 channels)' % N_FILE in out          # --steps_per_epoch 3 x total_bs 4
        assert 'ModelNet test source: %s' % (tmp_path / 'data' / ('modelnet40_test_%dpts_fps.dat' % N_FILE)) in out
        assert '(10 clouds of %d points, 3 channels)' % N_FILE in out
        assert '[Batch 3/3]' in out
        assert out.count('[Validation] EPOCH: 0  acc = ') == 1 and out.count('[Validation] EPOCH: 1  acc = ') == 1
        assert list(tmp_path.glob('experiments/*/*/%s/ckpt-last.pth' % backend))

    def figures(out, key):
        return [line.split(key)[1].split()[0] for line in out.splitlines() if key in line and not line.startswith('args.')]
    losses = figures(outs['hip'], 'Loss = ')
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses), outs['hip']
    assert figures(outs['torch'], 'Loss = ') == losses
    assert figures(outs['torch'], ' acc = ') == figures(outs['hip'], ' acc = ')
