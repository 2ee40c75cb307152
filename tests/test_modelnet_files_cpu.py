"""datasets.ModelNet on the reference's processed ModelNet40 files, without a GPU: what the loader holds of a written .dat
pickle (device='cpu'), the untouched synthetic fallback, the epoch's item order (datasets.epoch_items), the two ways to
iterate a listed train loader, and the host twin of pdae_resident_batch's load phase (resident_ops.apply_maps_host), which
tests/test_gpu_modelnet_files.py pins the kernel against."""
import os
import pickle

import numpy as np
import pytest
import torch

S, P = 7, 64


def write_dat(root, clouds, labels, subset='train', num_category=40, n_points=P):
    """The reference's processed file (ModelNetDataset.py:93, :117-118): [list_of_points, list_of_labels]."""
    os.makedirs(str(root), exist_ok=True)
    path = os.path.join(str(root), 'modelnet%d_%s_%dpts_fps.dat' % (num_category, subset, n_points))
    with open(path, 'wb') as f:
        pickle.dump([list(clouds), [np.array([k], np.int32) for k in labels]], f)
    return path


def make_clouds(count=S, points=P, seed=5):
    """Un-normalised clouds (off-centre, radius ~3) of six channels and labels that are not their positions."""
    rng = np.random.default_rng(seed)
    clouds = [(rng.normal(size=(points, 6)) * 3 + 1.5).astype(np.float32) for _ in range(count)]
    return clouds, [(3 * k + 1) % 10 for k in range(count)]


def build(root, subset='train', bs=2, device='cpu', **kw):
    from point_dae_amd import datasets  # noqa: F401
    from point_dae_amd.registry import DATASETS
    c = dict(NAME='ModelNet', DATA_PATH=str(root), N_POINTS=P, NUM_CATEGORY=40, USE_NORMALS=False, subset=subset, bs=bs,
             npoints=P, seed=0, device=device, aug_type=['norm', 'scale', 'translate'])
    c.update(kw)
    return DATASETS.build(c)


def _ref_normalize(pc):
    centroid = np.mean(pc, axis=0)
    pc = pc - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    return pc / m


# ---- the file is what the loader holds -------------------------------------------------------------------------------------

@pytest.mark.parametrize('count', [None, 5])
@pytest.mark.parametrize('num_category', [10, 40])
@pytest.mark.parametrize('use_normals', [False, True, 'true'])
@pytest.mark.parametrize('aug', [['norm', 'scale', 'translate'], ['clean'], ['norm']], ids=['norm_maps', 'clean', 'norm'])
def test_the_file_is_what_the_loader_holds(tmp_path, aug, use_normals, num_category, count):
    clouds, labels = make_clouds()
    write_dat(tmp_path, clouds, labels, 'train', num_category)
    # a file of another name in the same directory is not this loader's
    write_dat(tmp_path, [c + 1 for c in clouds], labels, 'test', num_category)
    kw = {} if count is None else dict(count=count)
    ds = build(tmp_path, 'train', aug_type=aug, USE_NORMALS=use_normals, NUM_CATEGORY=num_category, **kw)
    n = S if count is None else count
    C = 3 if use_normals is False else 6
    assert ds.listed and tuple(ds.set.shape) == (n, P, C) and ds.set.dtype == torch.float32
    assert ds.labels.dtype == torch.int64 and ds.labels.tolist() == labels[:n]
    want = np.stack(clouds[:n]).copy()
    if aug[0] == 'norm':
        for k in range(n):
            want[k, :, :3] = _ref_normalize(clouds[k][:, :3])
    assert want.dtype == np.float32
    assert np.array_equal(ds.set.numpy().view(np.int32), np.ascontiguousarray(want[:, :, :C]).view(np.int32))   # bit for bit
    assert ds.resident and len(ds) == n // 2
    assert 'modelnet%d_train_%dpts_fps.dat' % (num_category, P) in ds.source
    # the stored clouds were not written to
    again, _ = make_clouds()
    assert all(np.array_equal(a, b) for a, b in zip(clouds, again))


def test_an_absent_file_gives_todays_synthetic_arrays(tmp_path):
    from point_dae_amd.synthetic import labelled_clouds
    clouds, labels = make_clouds()
    write_dat(tmp_path, clouds, labels, 'train', 40, n_points=P + 1)           # (another N_POINTS: not this loader's file)
    for root in (tmp_path, tmp_path / 'nowhere', ''):
        for subset, offset in (('train', 1000), ('test', 2000)):
            ds = build(root, subset, bs=4, seed=3, count=10, npoints=32, N_POINTS=P)
            assert not ds.listed and not ds.resident and 'synthetic' in ds.source
            x, y = labelled_clouds(10, 32, seed=3 + offset, classes=3)
            assert torch.equal(ds.x, torch.from_numpy(x)) and torch.equal(ds.y, torch.from_numpy(y))
            assert ds.aug_type == ['norm', 'scale', 'translate'] and len(ds) == (2 if subset == 'train' else 3)
            # the same draws: the generator behind `augment` is where it was
            want = np.random.default_rng(3 + offset + 17).uniform(size=4)
            assert np.array_equal(ds.rng.uniform(size=4), want)
    # no augmentation: no generator, as before; the sharded fallback is the old one too
    assert build('', 'test', aug_type=['clean'], count=10).rng is None
    ds = build('', 'test', bs=4, seed=3, count=10, npoints=32, rank=1, world=4)
    x, y = labelled_clouds(10, 32, seed=2003, classes=3)
    sel = np.resize(np.arange(10), 12)[1::4]
    assert torch.equal(ds.x, torch.from_numpy(x[sel])) and torch.equal(ds.y, torch.from_numpy(y[sel]))


def test_other_subsets_yield_the_file_in_order_with_the_short_last_batch(tmp_path):
    clouds, labels = make_clouds()
    write_dat(tmp_path, clouds, labels, 'test')
    ds = build(tmp_path, 'test', bs=3, aug_type=['norm'], USE_NORMALS=True)
    assert ds.listed and not ds.resident and len(ds) == 3
    got = list(ds)
    assert [tuple(d[0].shape) for _, _, d in got] == [(3, P, 6), (3, P, 6), (1, P, 6)]
    assert torch.equal(torch.cat([d[0] for _, _, d in got]), ds.set)
    assert torch.equal(torch.cat([d[1] for _, _, d in got]), ds.labels) and ds.labels.tolist() == labels
    with pytest.raises(RuntimeError):
        ds.iter_draws()
    # the rank sharding of today: wrap-padded to a multiple of world, every world-th cloud
    shard = build(tmp_path, 'test', bs=3, aug_type=['norm'], rank=1, world=2)
    sel = np.resize(np.arange(S), 8)[1::2]
    assert shard.labels.tolist() == [labels[k] for k in sel]
    assert torch.equal(shard.set, build(tmp_path, 'test', bs=3, aug_type=['norm']).set[torch.from_numpy(sel)])


def test_maps_the_fused_path_does_not_take(tmp_path):
    clouds, labels = make_clouds()
    write_dat(tmp_path, clouds, labels, 'train')
    for aug in (['scale', 'norm'], ['norm', 'scale', 'translate', 'rotate_z', 'rotate'], ['norm', 'scale', 'norm']):
        ds = build(tmp_path, 'train', aug_type=aug)
        assert ds.listed and not ds.resident
        assert np.array_equal(ds.set.numpy(), np.stack(clouds)[:, :, :3])       # nothing is applied at load
        with pytest.raises(RuntimeError):
            ds.iter_draws()
    assert build(tmp_path, 'train', aug_type=['norm', 'scale', 'translate', 'rotate']).resident
    assert build(tmp_path, 'train', aug_type=['scale', 'translate']).resident
    with pytest.raises(NotImplementedError):
        build(tmp_path, 'train', aug_type=['norm', 'jitter'])


# ---- the epoch's items -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('count,world,bs', [(23, 1, 4), (23, 2, 4), (23, 4, 2), (24, 3, 8), (5, 4, 1)])
def test_epoch_items(count, world, bs):
    from point_dae_amd.datasets import epoch_items
    seed, epoch = 11, 3
    shared = np.random.default_rng([seed, epoch]).permutation(count)
    assert sorted(shared.tolist()) == list(range(count))
    per_rank = -(-count // world)
    padded = np.resize(shared, per_rank * world)
    got = [epoch_items(count, seed, epoch, r, world, bs) for r in range(world)]
    for r, items in enumerate(got):
        # every rank derives the same permutation and takes its own stride of it; only full batches are kept
        assert items.shape == (per_rank // bs, bs) and items.dtype == np.int64
        assert np.array_equal(items.reshape(-1), padded[r::world][:(per_rank // bs) * bs])
    if per_rank % bs == 0:                                   # nothing dropped: the shards cover the padded permutation
        assert sorted(np.concatenate([g.reshape(-1) for g in got]).tolist()) == sorted(padded.tolist())
    if world * per_rank == count:                            # nothing padded: the shards are disjoint
        flat = np.concatenate([g.reshape(-1) for g in got])
        assert len(set(flat.tolist())) == flat.size
    for r in range(world):
        assert np.array_equal(epoch_items(count, seed, epoch, r, world, bs), got[r])
    if count > 5:
        assert not np.array_equal(epoch_items(count, seed, epoch + 1, 0, world, bs), got[0])
        assert not np.array_equal(epoch_items(count, seed + 1, epoch, 0, world, bs), got[0])


def test_the_loader_takes_its_epochs_from_epoch_items(tmp_path):
    from point_dae_amd.datasets import epoch_items
    clouds, labels = make_clouds(count=11)
    write_dat(tmp_path, clouds, labels, 'train')
    # _loader passes seed + rank: ranks 0 and 1 of a run with seed 5
    for rank in (0, 1):
        ds = build(tmp_path, 'train', bs=2, seed=5 + rank, rank=rank, world=2)
        assert tuple(ds.set.shape) == (11, P, 3) and len(ds) == 3                # the whole set on every rank
        for epoch in (0, 1):                                                    # without set_epoch: counted from 0
            items = torch.stack([d[0] for _, _, d in ds.iter_draws()])
            assert np.array_equal(items.numpy(), epoch_items(11, 5, epoch, rank, 2, 2))
        ds.set_epoch(7)
        items = torch.stack([d[0] for _, _, d in ds.iter_draws()])
        assert np.array_equal(items.numpy(), epoch_items(11, 5, 7, rank, 2, 2))
        items = torch.stack([d[0] for _, _, d in ds.iter_draws()])
        assert np.array_equal(items.numpy(), epoch_items(11, 5, 8, rank, 2, 2))


# ---- the two ways to iterate ---------------------------------------------------------------------------------------------------

def host_norm_affine(x, normalise=False, maps=None, **kw):
    """pipeline_norm_affine's maps on the host (there is no GPU here): resident_ops.apply_maps_host on the packed pair."""
    from point_dae_amd import resident_ops
    assert not normalise and isinstance(maps, tuple) and not kw
    return torch.from_numpy(resident_ops.apply_maps_host(x.numpy(), maps[0].numpy(), maps[1].numpy()))


@pytest.mark.parametrize('use_normals', [False, True])
def test_iter_and_iter_draws_consume_the_draws_identically(tmp_path, monkeypatch, use_normals):
    from point_dae_amd import datasets, resident_ops
    monkeypatch.setattr(datasets, 'pipeline_norm_affine', host_norm_affine)
    clouds, labels = make_clouds()
    write_dat(tmp_path, clouds, labels, 'train')
    a = build(tmp_path, 'train', bs=3, seed=4, USE_NORMALS=use_normals)
    b = build(tmp_path, 'train', bs=3, seed=4, USE_NORMALS=use_normals)
    C = 6 if use_normals else 3
    seen = []
    for epoch in range(2):
        batches, draws = list(a), list(b.iter_draws())
        assert len(batches) == len(draws) == 2
        for (tax, _, (points, lab)), (tax2, key, (item, perm, nmaps, maps, lab2)) in zip(batches, draws):
            assert tax == tax2 == 'ModelNet' and key == 'sample'
            assert item.dtype == perm.dtype == nmaps.dtype == torch.int32 and maps.dtype == torch.float32
            assert tuple(item.shape) == (3,) and tuple(perm.shape) == (3, P) and tuple(maps.shape) == (3, 3, 12)
            assert nmaps.tolist() == [2, 2, 2]
            for row in perm:
                assert sorted(row.tolist()) == list(range(P))
            assert torch.equal(lab, lab2) and torch.equal(lab, b.labels[item.long()]) and lab.dtype == torch.int64
            # the materialised batch is the draws applied on the host
            sel = b.set.numpy()[item.numpy()]
            want = sel.copy()
            want[:, :, :3] = resident_ops.apply_maps_host(sel[:, :, :3], nmaps.numpy(), maps.numpy())
            want = np.take_along_axis(want, perm.numpy().astype(np.int64)[:, :, None], 1)
            assert tuple(points.shape) == (3, P, C) and points.is_contiguous()
            assert np.array_equal(points.numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))
            seen.append((item.clone(), perm.clone(), maps.clone()))
    assert not torch.equal(seen[0][1], seen[2][1]) and not torch.equal(seen[0][2], seen[2][2])   # the second epoch draws afresh
    # both generators are where the other loader's are
    assert torch.equal(torch.rand(4, generator=a.gen), torch.rand(4, generator=b.gen))
    assert np.array_equal(a.rng.uniform(size=4), b.rng.uniform(size=4))
    # another seed: other draws
    c = build(tmp_path, 'train', bs=3, seed=5, USE_NORMALS=use_normals)
    first = next(iter(c.iter_draws()))[2]
    assert not torch.equal(first[1], seen[0][1]) and not torch.equal(first[3], seen[0][2])


def test_draw_ranges(tmp_path):
    clouds, labels = make_clouds()
    write_dat(tmp_path, clouds, labels, 'train')
    ds = build(tmp_path, 'train', bs=7)
    eye = np.eye(3, dtype=np.float32).reshape(-1)
    for _ in range(30):
        nmaps, maps = ds.draw_maps(7)
        assert nmaps.dtype == np.int32 and nmaps.tolist() == [2] * 7 and maps.dtype == np.float32 and maps.shape == (7, 3, 12)
        scale, translate, unused = maps[:, 0], maps[:, 1], maps[:, 2]
        diag = scale[:, [0, 4, 8]]
        assert (diag >= np.float32(2 / 3)).all() and (diag <= np.float32(1.5)).all()         # PointcloudScale U(2/3, 3/2)^3
        assert (scale[:, [1, 2, 3, 5, 6, 7]] == 0).all() and (scale[:, 9:] == 0).all()
        assert (np.abs(translate[:, 9:]) <= np.float32(0.2)).all()                           # PointcloudTranslate U(-.2, .2)^3
        assert (translate[:, :9] == eye).all()
        assert (unused[:, :9] == eye).all() and (unused[:, 9:] == 0).all()
        assert len(np.unique(diag)) == 21 and len(np.unique(translate[:, 9:])) == 21        # a fresh draw per cloud and axis


# ---- the host twin of the load phase ----------------------------------------------------------------------------------------------

def test_apply_maps_host_against_float64():
    """|coordinate| <= 2, maps [scale, translate, scale] with scale in [2/3, 3/2] and |translate| <= 0.2.  A scale or a
    translate map multiplies by exact zeros and ones and adds exact zeros everywhere but in ONE operation per coordinate,
    so each map rounds once: |x| <= 3.2 < 4 behind the first two maps (half an ulp: 2^-23 = 1.2e-7 each), the last scale
    stretches what came before by <= 1.5 and rounds a value < 8 (2.4e-7): 1.5 * 2.4e-7 + 2.4e-7 = 6e-7 <= 1e-6."""
    from point_dae_amd import resident_ops
    from point_dae_amd.datasets import draw_affine_map
    rng = np.random.default_rng(0)
    B, n = 8, 500
    x = rng.uniform(-2, 2, (B, n, 3)).astype(np.float32)
    nmaps = np.array([0, 1, 2, 3, 3, 2, 1, 3], np.int32)
    maps = np.zeros((B, 3, 12), np.float32)
    for b in range(B):
        for q, name in enumerate(('aug_scale', 'aug_translate', 'aug_scale')):
            M, t = draw_affine_map(rng, name)
            maps[b, q, :9], maps[b, q, 9:] = M.reshape(-1), t
    got = resident_ops.apply_maps_host(x, nmaps, maps)
    assert got.dtype == np.float32 and got.shape == x.shape
    for b in range(B):
        want = x[b].astype(np.float64)
        for q in range(nmaps[b]):
            want = want @ maps[b, q, :9].astype(np.float64).reshape(3, 3) + maps[b, q, 9:].astype(np.float64)
        assert np.abs(got[b] - want).max() <= 1e-6, b
    assert np.array_equal(got[0], x[0]) and not np.array_equal(got[1], x[1])
    assert np.array_equal(resident_ops.apply_maps_host(x, None, None), x)
    with pytest.raises(ValueError):
        resident_ops.apply_maps_host(x, np.full(B, 4), maps)


def test_host_twin_is_the_fewshot_twin_on_the_mapped_clouds(oracle_ops):
    from point_dae_amd import fewshot_ops, resident_ops
    rng = np.random.default_rng(2)
    set_ = rng.uniform(-1, 1, (4, 70, 6)).astype(np.float32)
    item = np.array([2, 0, 2], np.int32)
    perm = np.stack([rng.permutation(70) for _ in range(3)]).astype(np.int32)
    nmaps = np.array([2, 0, 1], np.int32)
    maps = np.zeros((3, 3, 12), np.float32)
    maps[:, :, [0, 4, 8]] = rng.uniform(0.7, 1.4, (3, 3, 3))
    maps[:, :, 9:] = rng.uniform(-0.2, 0.2, (3, 3, 3))
    idx, pts = resident_ops.batch_host(set_, item, perm, nmaps, maps, 40, oracle_ops.furthest_point_sample)
    mapped = resident_ops.apply_maps_host(set_[item][:, :, :3], nmaps, maps)
    assert np.array_equal(idx[:, 0], perm[:, 0]) and idx.dtype == np.int32
    assert np.array_equal(pts, np.take_along_axis(mapped, idx[:, :, None].astype(np.int64), 1))
    # no maps: the few-shot twin itself
    idx0, pts0 = resident_ops.batch_host(set_, item, perm, None, None, 40, oracle_ops.furthest_point_sample)
    want_idx, want_pts = fewshot_ops.batch_host(set_, item, perm, 40, oracle_ops.furthest_point_sample)
    assert np.array_equal(idx0, want_idx) and np.array_equal(pts0, want_pts)
    assert not np.array_equal(idx[0], idx0[0]) and np.array_equal(idx[1], idx0[1])         # the anisotropic scale moves the picks


def test_backend_reads_the_environment(monkeypatch):
    from point_dae_amd import resident_ops
    monkeypatch.delenv('PDAE_MODELNET', raising=False)
    assert resident_ops.backend() == 'hip'
    monkeypatch.setenv('PDAE_MODELNET', 'torch')
    assert resident_ops.backend() == 'torch'
    monkeypatch.setenv('PDAE_MODELNET', 'eager')
    with pytest.raises(ValueError):
        resident_ops.backend()
