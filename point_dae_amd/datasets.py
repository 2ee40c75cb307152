"""ShapeNet-55 pretraining set with the loader-side pipeline ON THE DEVICE.

Reference item (datasets/ShapeNet55Dataset.py:90-119): read an 8192-point cloud (datasets/io.py),
`augment_data` ('norm' = centre + scale to the unit sphere, corrupt_util.py:7-17), clean = random
subset of `npoints`; corrupted = `corrupt_data(whole cloud, corrupt_type)` (corrupt_util.py:1046-1096:
'affine_r3' = 1-3 of translate / scale_nonorm / rotate / reflection / shear in random order,
'dropout_local' :590-612) followed by another random subset.  The reference does this per item in 8
DataLoader worker processes; at the ~9 k clouds/s of the training step on one MI355X that is 60 k
argsorts of 8192-point clouds per second on host cores.

Here the stored clouds are resident in HBM (ShapeNet-55's 41 952 training clouds x 8192 x 3 fp32 =
4.1 GB of the 288 GB) and a batch is gathered, normalised, corrupted and sub-sampled by the kernels of
csrc/pipeline.hip -- norm + affine maps + jitter in one launch, add_global / add_local / nonuniform_density /
dropout_local one launch each, the random subset one launch -- each a pure function of the clouds and of
random draws, pinned on the LIVE reference's `ShapeNet.__getitem__` with its draws recorded
(tests/golden/make_loader_fixtures.py, tests/test_pipeline.py).  In production the host draws the
small parameters (maps, levels, cluster sizes: a few hundred numbers per batch) with the reference's
distributions and the device draws the bulk noise / keys.  Random streams are this module's own (numpy
Generator seeded with seed + rank, torch device generator): the reference's per-worker global numpy /
python generators are not reproducible across worker counts either.

Sources: a directory of .npy clouds listed by `<DATA_PATH>/<subset>.txt` (the reference layout), else
synthetic ShapeNet-shaped clouds (there is no dataset in the image).
"""
import functools
import math
import os

import numpy as np
import torch

from . import _lib
from .registry import DATASETS
from .synthetic import labelled_clouds, shapenet_like_clouds

AFFINE = ('translate', 'scale_nonorm', 'rotate', 'reflection', 'shear')
AFFINE_V2 = ('translate', 'scale_nonorm', 'rotate_level1', 'reflection', 'shear_1p')        # corrupt_util.py:1043
# 'affine_rN[_v2]' of corrupt_util.corrupt_data (:1053-1088): 1..N distinct maps of the pool in random order
_AFFINE_SETS = {'affine_r3': (AFFINE, 3), 'affine_r5': (AFFINE, 5), 'affine_r3_v2': (AFFINE_V2, 3), 'affine_r5_v2': (AFFINE_V2, 5)}
# the single maps of the reference's `corruptions` table (corrupt_util.py:984-1038) as (kind, parameter); the parameter
# ranges are pinned on the live functions' recorded draws (tests/golden/make_loader_variant_fixtures.py)
_MAP_PARAMS = {
    'translate': ('translate', 0.5), 'translate_tiny': ('translate', 0.1), 'translate_middle': ('translate', 0.3),
    'translate_too_large': ('translate', 0.8),                                              # x + U(-s, s)^3       :130-177
    'scale_nonorm': ('scale', 2.0), 'scale_nonorm_1p5': ('scale', 1.5), 'scale_nonorm_4': ('scale', 4.0),
    'scale_nonorm_10': ('scale', 10.0),                                                     # x * U(1/s, s)^3      :82-128
    'rotate': ('rotate', math.pi),                                                          # Rz Ry Rx, U(-c, c)^3 :241-263
    'rotate_level0': ('rotate', math.pi / 5), 'rotate_level1': ('rotate', 2 * math.pi / 5),
    'rotate_level2': ('rotate', 3 * math.pi / 5), 'rotate_level3': ('rotate', 4 * math.pi / 5),
    'rotate_level4': ('rotate', math.pi),                                                   # c = pi / 5 (l + 1)   :265-388
    'rotate_z': ('rotate_z_level', math.pi / 5),                                            # c = pi / 5 (level+1) :537-570
    'reflection': ('reflection', None),                                                     # diag(+-1)            :390-409
    'shear': ('shear', 0.5), 'shear_p1': ('shear', 0.1), 'shear_p3': ('shear', 0.3), 'shear_p8': ('shear', 0.8),
    'shear_1p': ('shear', 1.0), 'shear_2p': ('shear', 2.0),                                 # off-diagonals U(-c, c) :412-518
    'shear_small': ('shear_level', 0.02),                                                   # c = 0.02 (level + 1) :520-535
    # augment_data (:1105-1175): PointcloudScale U(2/3, 3/2)^3, PointcloudTranslate U(-.2, .2)^3, full-circle rotations
    'aug_scale': ('scale', 1.5), 'aug_translate': ('translate', 0.2), 'aug_rotate_z': ('rotate_z', math.pi),
    'aug_rotate': ('rotate', math.pi),
}
_JITTER = {'jitter': None, 'jitter_p01': 0.01, 'jitter_p03': 0.03, 'jitter_p05': 0.05, 'jitter_p1': 0.1}   # :179-239
# dropout_local variants (:590-828): (drop ratio or None = U(.1, .5), exclusive upper bound of randint(1, hi) clusters or
# 0 = exactly one cluster without a draw)
_DROPOUT_LOCAL = {'dropout_local': (None, 8), 'dropout_local_c5d1': (0.1, 5), 'dropout_local_c5d3': (0.3, 5),
                  'dropout_local_c5d5': (0.5, 5), 'dropout_local_c5d7': (0.7, 5), 'dropout_local_c5d9': (0.9, 5),
                  'dropout_local_c1d3': (0.3, 0), 'dropout_local_c2d3': (0.3, 2), 'dropout_local_c3d3': (0.3, 3),
                  'dropout_local_c8d3': (0.3, 8)}
_SCALE_SINGLE = (1.6, 1.7, 1.8, 1.9, 2.0)                                                   # :71-80, by level
_PASS = ('clean', 'dropout_patch_pointmae', 'Drop-Patch')
_AUGS = ('clean', 'norm', 'scale', 'translate', 'rotate_z', 'rotate')          # corrupt_util.augment_data :1155-1175
_CORRUPTIONS = (tuple(_AFFINE_SETS) + tuple(n for n in _MAP_PARAMS if not n.startswith('aug_')) + tuple(_JITTER)
                + tuple(_DROPOUT_LOCAL) + ('scale', 'scale_single', 'add_global', 'add_local', 'nonuniform_density'))
# names some reference YAMLs carry that the reference's own dispatcher does not know (a KeyError there too)
_UNKNOWN_UPSTREAM = ('affine_r3_tiny', 'affine_r3_middle', 'scan')


def _rot(a):
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def map_needs_level(name):
    return _MAP_PARAMS[name][0] in ('rotate_z_level', 'shear_level')


def affine_map_from_draw(name, draw):
    """(M, tr) of the map `name` for the values the numpy version draws (one uniform / choice call, corrupt_util.py)."""
    kind = _MAP_PARAMS[name][0]
    kind = kind[:-6] if kind.endswith('_level') else kind
    draw = np.asarray(draw, np.float64).reshape(-1)
    M, tr = np.eye(3), np.zeros(3)
    if kind == 'translate':
        tr = draw
    elif kind in ('scale', 'reflection'):
        M = np.diag(draw)
    elif kind == 'rotate':
        M = _rot(draw)
    elif kind == 'rotate_z':
        a = draw[0]
        M = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    elif kind == 'shear':
        M = np.array([[1, draw[0], draw[1]], [draw[2], 1, draw[3]], [draw[4], draw[5], 1]])
    return M, tr


def draw_affine_map(rng, name, level=None):
    """One map x -> x M + tr of the table above with the numpy versions' parameters (corrupt_util.py); `level` (0..4,
    the dispatcher's random.choice, :1090-1092) only matters to 'rotate_z' and 'shear_small' and is drawn here when
    not given."""
    if name not in _MAP_PARAMS:
        raise NotImplementedError(name)
    kind, par = _MAP_PARAMS[name]
    if kind.endswith('_level'):
        level = int(rng.integers(0, 5)) if level is None else int(level)
        kind, par = kind[:-6], par * (level + 1)
    if kind == 'translate':
        draw = rng.uniform(-par, par, 3)
    elif kind == 'scale':
        draw = rng.uniform(1.0 / par, par, 3)
    elif kind == 'rotate':
        draw = rng.uniform(-par, par, 3)
    elif kind == 'rotate_z':
        draw = rng.uniform(-par, par, 1)
    elif kind == 'reflection':
        draw = rng.choice(np.array([1.0, -1.0]), 3)
    else:
        draw = rng.uniform(-par, par, 6)
    return affine_map_from_draw(name, draw)


def draw_affine(rng, B, names_of):
    """Per cloud the composition of the maps `names_of(rng)` lists -> A (B,3,3), t (B,3), y = x @ A + t."""
    A = np.tile(np.eye(3), (B, 1, 1))
    t = np.zeros((B, 3))
    for b in range(B):
        for name in names_of(rng):
            M, tr = draw_affine_map(rng, name)
            A[b] = A[b] @ M                  # y = (x A + t) M + tr
            t[b] = t[b] @ M + tr
    return A.astype(np.float32), t.astype(np.float32)


def draw_affine_set(rng, B, item='affine_r3'):
    """'affine_r3' / 'affine_r5' / '..._v2' of corrupt_util.corrupt_data (:1053-1088) for B clouds: per cloud 1-N distinct
    maps of the pool in random order."""
    pool, most = _AFFINE_SETS[item]

    def names(r):
        number = int(r.integers(1, most + 1))
        return [pool[int(i)] for i in r.choice(len(pool), size=number, replace=False)]
    return draw_affine(rng, B, names)


def draw_affine_r3(rng, B):
    return draw_affine_set(rng, B, 'affine_r3')



def sphere_points(rng, B, n):
    """n points uniform in the unit ball per cloud (corrupt_util._sample_points_inside_unit_sphere :42-56)."""
    r = np.power(rng.uniform(0.0, 1.0, (B, n, 1)), 1.0 / 3.0)
    theta = np.arccos(rng.uniform(-1.0, 1.0, (B, n, 1)))
    phi = rng.uniform(0.0, 2.0 * np.pi, (B, n, 1))
    return np.concatenate([r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi), r * np.cos(theta)],
                          axis=2).astype(np.float32)


def draw_dropout_local(rng, B, P, item='dropout_local'):
    """The draws of corrupt_dropout_local (:590-612) and its _cXdY variants (:614-828) for B clouds of P points: ratio
    U(.1,.5) or the variant's constant, 1..hi-1 clusters, sizes = counts of `total` uniform cluster labels, and per
    cluster the seed as a rank among the survivors (a shuffle's first element).
    -> nclusters (B,), seed_rank (B,8), sizes (B,8) int32."""
    ratio, hi = _DROPOUT_LOCAL[item]
    ncl = np.zeros(B, np.int32)
    rank = np.zeros((B, 8), np.int32)
    sizes = np.zeros((B, 8), np.int32)
    for b in range(B):
        total = int(P * (rng.uniform(0.1, 0.5) if ratio is None else ratio))
        n = int(rng.integers(1, hi)) if hi else 1
        counts = np.bincount(rng.integers(0, n, total), minlength=n)
        alive = P
        ncl[b] = n
        for c in range(n):
            sizes[b, c] = counts[c]
            rank[b, c] = int(rng.integers(0, alive))
            alive -= int(counts[c])
    return ncl, rank, sizes


def dropout_local(x, ncl, rank, sizes):
    """x (B,P,3) on the device + host draws -> alive (B,P) bool (csrc/pipeline.hip)."""
    B, P, _ = x.shape
    dev = x.device
    alive = torch.empty((B, P), dtype=torch.uint8, device=dev)
    n_d, r_d, s_d = (_dev(a, dev) for a in (ncl, rank, sizes))
    _lib.call('pdae_dropout_local', x, B, P, _lib.ptr(x.contiguous()), _lib.ptr(n_d), _lib.ptr(r_d), _lib.ptr(s_d),
              _lib.ptr(alive))
    return alive.bool()


def _dev(a, device, dtype=None):
    """Host draws -> device WITHOUT blocking the host: a pageable source makes .to() a synchronous, stream-ordered copy,
    i.e. the host would wait for everything queued on the stream (the previous optimisation step) at every small
    parameter tensor of a batch.  Pinned staging (torch's caching host allocator keeps the block until the copy ran)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    if torch.device(device).type != 'cuda':
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def pipeline_norm_affine(x, normalise=False, maps=None, sigma=None, noise=None, stride=None):
    """x (B,P,3) -> y (B,stride,3) with rows [0,P) = jitter(affine maps(norm(x))) (csrc/pipeline.hip norm_affine).
    maps: list per cloud of up to three (M (3,3), t (3,)) pairs applied in order, y = x M + t; sigma (B,) and
    noise (B,P,3) on the device: y += sigma * noise.  maps may also be the packed pair (nmaps (B,) int32,
    maps (B,3,12) float32: M row-major, then t) already on the device."""
    B, P, _ = x.shape
    stride = P if stride is None else stride
    dev = x.device
    y = torch.empty((B, stride, 3), device=dev)
    nm = mp = None
    if isinstance(maps, tuple):
        nm, mp = maps
        if tuple(nm.shape) != (B,) or nm.dtype != torch.int32 or tuple(mp.shape) != (B, 3, 12) or mp.dtype != torch.float32:
            raise ValueError('pipeline_norm_affine: packed maps are nmaps (B,) int32 and maps (B,3,12) float32')
        nm, mp = nm.contiguous(), mp.contiguous()
    elif maps is not None:
        packed = np.zeros((B, 3, 12), np.float32)
        packed[:, :, 0] = packed[:, :, 4] = packed[:, :, 8] = 1.0
        counts = np.zeros(B, np.int32)
        for b, ms in enumerate(maps):
            counts[b] = len(ms)
            for q, (M, t) in enumerate(ms):
                packed[b, q, :9], packed[b, q, 9:] = np.asarray(M, np.float64).reshape(-1), np.asarray(t, np.float64)
        nm, mp = _dev(counts, dev), _dev(packed, dev)
    _lib.call('pdae_pipeline_norm_affine', x, B, P, stride, int(bool(normalise)), _lib.ptr(x.contiguous()), _lib.ptr(nm),
              _lib.ptr(mp), _lib.ptr(sigma), _lib.ptr(noise), _lib.ptr(y))
    return y


def pipeline_add_global(y, p0, count, u):
    """append count[b] points uniform in the unit ball behind row p0 of every cloud; u (B,nmax,3) uniforms."""
    B, stride, _ = y.shape
    _lib.call('pdae_pipeline_add_global', y, B, u.shape[1], stride, p0, _lib.ptr(count), _lib.ptr(u), _lib.ptr(y))


def pipeline_add_local(y, p0, count, seed, sigma, noise):
    """append count[b] cluster points: cloud point seed[b,j] + sigma[b,j] * noise[b,j], pulled inside the unit sphere."""
    B, stride, _ = y.shape
    _lib.call('pdae_pipeline_add_local', y, B, seed.shape[1], stride, p0, _lib.ptr(count), _lib.ptr(seed), _lib.ptr(sigma),
              _lib.ptr(noise), _lib.ptr(y))


def pipeline_density(y, p, view, gate, r, alive):
    """alive[b,k] &= normalised distance to view[b] * gate[b] < r[b,k] for the first p rows."""
    B, stride, _ = y.shape
    _lib.call('pdae_pipeline_density', y, B, p, stride, _lib.ptr(y), _lib.ptr(view), _lib.ptr(gate), _lib.ptr(r),
              _lib.ptr(alive))


def pipeline_subset(y, p, n, keys, alive=None):
    """-> (B,n,3): the n alive points with the smallest keys among the first p rows, in key order."""
    B, stride, _ = y.shape
    out = torch.empty((B, n, 3), device=y.device)
    _lib.call('pdae_pipeline_subset', y, B, p, stride, n, _lib.ptr(y), _lib.ptr(alive), _lib.ptr(keys), _lib.ptr(out))
    return out


def draw_affine_maps(rng, names):
    """[(M, t)] for the named maps, in order (draw_affine_map's parameter ranges)."""
    return [draw_affine_map(rng, n) for n in names]



def load_npy_clouds(pc_path, data_path, subset, whole=False, limit=None):
    """The reference's file layout: `<data_path>/<subset>.txt` lists `<taxonomy>-<model>.npy` files
    under `pc_path` (ShapeNet55Dataset.py:37-62).  -> (clouds (num,P,>=3) float32, [(taxonomy, model)])."""
    lines = open(os.path.join(data_path, '%s.txt' % subset)).read().split()
    if whole:
        lines += open(os.path.join(data_path, 'test.txt')).read().split()
    if limit:
        lines = lines[:limit]
    ids, clouds = [], []
    for line in lines:
        tax = line.split('-')[0]
        ids.append((tax, line[len(tax) + 1:].split('.')[0]))
        clouds.append(np.load(os.path.join(pc_path, line)).astype(np.float32))
    return np.stack(clouds, 0), ids


@DATASETS.register_module()
class ShapeNet:
    def __init__(self, config):
        self.npoints = config.get('npoints', 1024)
        self.dense = config.get('N_POINTS', 8192)
        self.bs = config.get('bs', 128)
        # batches per epoch: given, else the reference's len(DataLoader) = ceil(len(set) / (bs * world)) once a listed
        # set is loaded (DistributedSampler shards it, builder.py:19), else 50 synthetic batches
        self.steps = config.get('steps_per_epoch', None)
        self.shared_seed = config.get('shared_seed', None)
        self.rank, self.world = int(config.get('rank', 0)), max(int(config.get('world', 1)), 1)
        self.seed = config.get('seed', 0)
        self.device = config.get('device', 'cuda')
        self.pool = config.get('pool', 4)
        self.aug_type = list(config.get('aug_type', ['clean']))
        self.corrupt_type = list(config.get('corrupt_type', ['clean']))
        self.subset = config.get('subset', 'train')
        self.pc_path, self.data_path = config.get('PC_PATH'), config.get('DATA_PATH')
        self.whole = bool(config.get('whole', False))
        for item in self.corrupt_type:
            if item in _UNKNOWN_UPSTREAM:
                raise NotImplementedError('loader-side corruption %r: the reference\'s own dispatcher (corrupt_util.py:984-1096) '
                                          'has no such entry either (KeyError there)' % item)
            if not (item in _PASS or 'dropout_global' in item or item in _CORRUPTIONS):
                raise NotImplementedError('loader-side corruption %r (implemented: %s)' % (item, ', '.join(_CORRUPTIONS)))
        for item in self.aug_type:
            if item not in _AUGS:
                raise NotImplementedError('augmentation %r (implemented: %s)' % (item, ', '.join(_AUGS)))
        self.rng = np.random.default_rng(self.seed)
        self.gen = None
        self._clouds, self.ids = None, None

    def _materialise(self):
        listed = self.pc_path and self.data_path and os.path.exists(os.path.join(str(self.data_path), '%s.txt' % self.subset))
        if listed:
            clouds, self.ids = load_npy_clouds(self.pc_path, self.data_path, self.subset, self.whole)
            clouds = clouds[:, :, :3]
        else:
            n = self.bs * self.pool
            clouds = shapenet_like_clouds(n, self.dense, seed=self.seed, dense=max(self.dense, 8192))
            self.ids = [('synthetic', str(i)) for i in range(n)]
        self._clouds = torch.from_numpy(np.ascontiguousarray(clouds)).to(self.device)
        self.gen = torch.Generator(device=self._clouds.device)
        self.gen.manual_seed(self.seed)
        self.listed = bool(listed)
        if self.steps is None:
            if listed:
                per_rank = -(-clouds.shape[0] // self.world)        # DistributedSampler pads to ceil(N / world)
                # tools/builder.py:21,28: drop_last = (subset == 'train') => floor for the training loader, ceil otherwise
                self.steps = max(per_rank // self.bs, 1) if self.subset == 'train' else -(-per_rank // self.bs)
            else:
                self.steps = 50

    def __len__(self):
        if self.steps is None:
            self._materialise()
        return self.steps

    def batch(self, index):
        """-> (corrupted (B,npoints,3), clean (B,npoints,3)) on the device, every stage on csrc/pipeline.hip:
        ShapeNet.__getitem__ (:90-119) = augment_data -> random_sample -> corrupt_data -> random_sample."""
        x = self._clouds.index_select(0, index)
        B, P, _ = x.shape
        dev, rng = x.device, self.rng
        # ---- augment_data (:1155-1175), strictly in the configured order.  The kernel normalises FIRST and applies its
        # (<= 3) maps second, so a 'norm' is folded into the launch of the maps that FOLLOW it; maps drawn before a
        # 'norm' are flushed (normalise off, three per pass) before that 'norm' gets its own launch.
        aug = [a for a in self.aug_type if a != 'clean']
        maps = [[] for _ in range(B)]
        norm_pending = False

        def flush(x, norm_pending, maps):
            """apply [norm?] + the pending maps in order, three maps per pass -> x"""
            while norm_pending or any(maps):
                x = pipeline_norm_affine(x, norm_pending, [m[:3] for m in maps] if any(maps) else None)
                maps, norm_pending = [m[3:] for m in maps], False
            return x
        for item in aug:
            if item == 'norm':
                x = flush(x, norm_pending, maps)                     # everything drawn so far comes before this norm
                maps, norm_pending = [[] for _ in range(B)], True
                continue
            for b in range(B):
                maps[b].append(draw_affine_map(rng, 'aug_' + item))
        data = flush(x, norm_pending, maps) if (norm_pending or any(maps)) else pipeline_norm_affine(x, False, None)
        clean = pipeline_subset(data, P, self.npoints, torch.rand((B, P), device=dev, generator=self.gen))
        # ---- corrupt_data (:1046-1096) on the whole cloud
        items = [c for c in self.corrupt_type if not (c in _PASS or 'dropout_global' in c)]   # those run in the model's forward
        if not items:
            return clean, clean
        n_add = int(P * 0.5) if any(c in ('add_global', 'add_local') for c in items) else 0   # level <= 4: at most +50 %
        stride = P + n_add
        maps = [[] for _ in range(B)]
        sigma = noise = None
        tail = []
        for item in items:                                          # the affine maps and jitter of the list: one launch
            if item in _AFFINE_SETS or item in _MAP_PARAMS:
                if noise is not None or tail:
                    raise NotImplementedError('an affine map behind jitter / an add / a drop in one corrupt_type list')
                for b in range(B):
                    if item in _AFFINE_SETS:
                        pool, most = _AFFINE_SETS[item]
                        number = int(rng.integers(1, most + 1))
                        for i in rng.choice(len(pool), size=number, replace=False):
                            maps[b].append(draw_affine_map(rng, pool[int(i)]))
                    else:
                        maps[b].append(draw_affine_map(rng, item))
            elif item in _JITTER and not tail and noise is None:
                # sigma = 0.01 (level + 1), level in 0..4 (:179-191, :1090-1092), or the variant's constant
                fixed = _JITTER[item]
                sig = 0.01 * (rng.integers(0, 5, B) + 1.0) if fixed is None else np.full(B, fixed)
                sigma = _dev(sig.astype(np.float32), dev)
                noise = torch.randn((B, P, 3), device=dev, generator=self.gen)
            elif item in _JITTER:
                raise NotImplementedError('jitter behind an add / a drop / another jitter in one corrupt_type list')
            else:
                tail.append(item)
        y = data
        if any(maps) or noise is not None or stride != P:
            passes = max(1, -(-max(len(m) for m in maps) // 3))      # three maps per launch ('affine_r5': up to two)
            for c in range(passes):
                last = c == passes - 1
                part = [m[3 * c:3 * c + 3] for m in maps]
                y = pipeline_norm_affine(y, False, part if any(part) else None, sigma if last else None,
                                         noise if last else None, stride if last else None)
        cur, alive = P, None                                        # rows in use; survivors
        for item in tail:
            if item in ('add_global', 'add_local') and (alive is not None or cur != P):
                raise NotImplementedError('%s after a drop / another add in one corrupt_type list' % item)
            if item == 'add_global':                                # int(P (level + 1) 0.1) ball points (:830-841)
                count = (P * (rng.integers(0, 5, B) + 1) * 0.1).astype(np.int32)
                if getattr(self, '_ball_affine', None) is None:       # (radius, cos theta, phi) ranges of the three uniforms
                    self._ball_affine = (_dev(np.array([1.0, 2.0, 2.0 * math.pi], np.float32), dev),
                                         _dev(np.array([0.0, 1.0, 0.0], np.float32), dev))
                pipeline_add_global(y, P, _dev(count, dev), torch.rand((B, n_add, 3), device=dev, generator=self.gen)
                                    * self._ball_affine[0] - self._ball_affine[1])
                cur, added = P + n_add, count
            elif item == 'add_local':                               # 1-7 Gaussian clusters on random cloud points (:844-870)
                count = (P * (rng.integers(0, 5, B) + 1) * 0.1).astype(np.int32)
                seed = np.zeros((B, n_add), np.int32)
                sig = np.zeros((B, n_add), np.float32)
                for b in range(B):
                    ncl = int(rng.integers(1, 8))
                    sizes = np.bincount(rng.integers(0, ncl, int(count[b])), minlength=ncl)
                    pts = rng.choice(P, ncl, replace=False)         # the first ncl points of a shuffle
                    seed[b, :count[b]] = np.repeat(pts, sizes)
                    sig[b, :count[b]] = np.repeat(rng.uniform(0.075, 0.125, ncl), sizes)
                pipeline_add_local(y, P, _dev(count, dev), _dev(seed, dev), _dev(sig, dev),
                                   torch.randn((B, n_add, 3), device=dev, generator=self.gen))
                cur, added = P + n_add, count
            elif item == 'nonuniform_density':                      # (:875-897) gate = level / 4 + 0.1, level in 0..4
                if alive is None:
                    alive = torch.ones((B, stride), dtype=torch.uint8, device=dev)
                v = rng.normal(0.0, 1.0, (B, 3))
                v = v / np.linalg.norm(v, axis=1, keepdims=True)
                gate = rng.integers(0, 5, B) / 4.0 + 0.1
                pipeline_density(y, cur, _dev(v.astype(np.float32), dev), _dev(gate.astype(np.float32), dev),
                                 torch.rand((B, cur), device=dev, generator=self.gen), alive)
            elif item in _DROPOUT_LOCAL:
                if cur != P or stride != P or alive is not None:
                    raise NotImplementedError('%s after an add / another drop in one corrupt_type list' % item)
                alive = dropout_local(y, *draw_dropout_local(rng, B, P, item)).to(torch.uint8)
            elif item in ('scale', 'scale_single'):
                # 'scale' U(.5,2)^3 (:59-69); 'scale_single' ONE factor U(1/s, s), s by level (:71-80); both re-normalised
                if cur != P or stride != P or alive is not None:
                    raise NotImplementedError('%s after an add / a drop in one corrupt_type list' % item)
                if item == 'scale':
                    ms = [[draw_affine_map(rng, 'scale_nonorm')] for _ in range(B)]
                else:
                    ms = []
                    for b in range(B):
                        s_ = _SCALE_SINGLE[int(rng.integers(0, 5))]
                        ms.append([(np.eye(3) * rng.uniform(1.0 / s_, s_), np.zeros(3))])
                y = pipeline_norm_affine(pipeline_norm_affine(y, False, ms), True)
            else:
                raise NotImplementedError(item)
        if cur != P:                                                # rows behind P + added[b] are not part of cloud b
            if alive is None:
                alive = torch.ones((B, stride), dtype=torch.uint8, device=dev)
            alive &= (torch.arange(stride, device=dev).view(1, -1) < (P + _dev(added, dev)).view(-1, 1)).to(torch.uint8)
        corrupted = pipeline_subset(y, cur, self.npoints, torch.rand((B, stride), device=dev, generator=self.gen), alive)
        return corrupted, clean

    def set_epoch(self, epoch):
        """DistributedSampler.set_epoch: the next iteration draws epoch `epoch`'s shared permutation (resume-safe)."""
        self._epoch, self._epoch_set = int(epoch), True

    def __iter__(self):
        if self._clouds is None:
            self._materialise()
        n = self._clouds.shape[0]
        if self.listed and self.world > 1:
            # DistributedSampler semantics: ONE permutation per epoch shared by the ranks (seeded without the
            # rank), padded by wrapping to a multiple of world, rank r takes every world-th index
            # `shared_seed` (config; the runner passes args.seed) is the rank-independent base; without it the constructor's
            # seed is taken to be base + rank (main.py:81 seeds rank r with seed + r).  set_epoch(e) names the epoch
            # (the reference calls sampler.set_epoch(epoch), runner_pretrain.py:115); otherwise epochs count from 0.
            if getattr(self, '_epoch_set', None) is None:
                self._epoch = getattr(self, '_epoch', -1) + 1
            self._epoch_set = None
            base = self.shared_seed if self.shared_seed is not None else self.seed - self.rank
            shared = np.random.default_rng([base, self._epoch]).permutation(n)
            total = -(-n // self.world) * self.world
            order = np.resize(shared, total)[self.rank::self.world]
            n = order.shape[0]
        else:
            order = self.rng.permutation(n)
        # The pipeline's launches sit in front of the step on the same stream; what matters is that the HOST never waits:
        # every small parameter tensor goes through pinned staging (_dev), so the host runs ahead of the GPU and the
        # pipeline's few small kernels are the only cost (measured end to end through main.py, 300-step epochs: 10 030-10 060
        # clouds/s = the bare step's rate; with pageable copies the host waited for the previous step at each of them:
        # 9 500.  Producing the next batch on a side stream as well changed nothing.)
        dev = self._clouds.device
        for i in range(self.steps):
            sel = order[(np.arange(self.bs) + i * self.bs) % order.shape[0]]
            corrupted, clean = self.batch(_dev(sel, dev))
            yield self.ids[int(sel[0])][0], i, corrupted, clean


def taxonomy_ranks(data_path):
    """{taxonomy id: label} of a listed set: the rank of the id among the sorted distinct taxonomy ids of
    `<data_path>/train.txt` and `<data_path>/test.txt` together (whichever exist)."""
    ids = set()
    for subset in ('train', 'test'):
        path = os.path.join(str(data_path), '%s.txt' % subset)
        if os.path.exists(path):
            with open(path) as f:
                ids.update(line.split('-')[0] for line in f.read().split())
    return {tax: rank for rank, tax in enumerate(sorted(ids))}


@DATASETS.register_module()
class ShapeNetClass(ShapeNet):
    """ShapeNet with class labels, for the task-affinity protocol (datasets/ShapeNet55Dataset.py ShapeNetClass of the
    reference): yields (taxonomy, model_id, (points (B, npoints, 3), labels (B,))) in list order.  The points are the
    `corrupted` output of ShapeNet.batch -- augment_data, corrupt_data on the whole cloud, random_sample(npoints) --, first
    three columns.  The `train` subset drops a short last batch (tools/builder.py: drop_last), the others keep it.

    Labels of a listed set: the rank of a file's taxonomy id among the sorted distinct taxonomy ids of train.txt and
    test.txt together (taxonomy_ranks).  The reference maps its 55 synset ids through a table in ascending order, so the
    two agree whenever all 55 classes are present in the lists; with classes missing the ranks close the gaps.
    Without files, labelled synthetic clouds stand in (synthetic.labelled_clouds; `count` clouds of `classes` classes), as
    for datasets.ModelNet.

    A corrupt_type item that ShapeNet.batch leaves to the model's forward (dropout_patch_pointmae, Drop-Patch,
    dropout_global*) is refused: nothing would apply it in this protocol."""

    def __init__(self, config):
        super().__init__(config)
        for item in self.corrupt_type:
            if (item in _PASS and item != 'clean') or 'dropout_global' in item:
                raise NotImplementedError('ShapeNetClass: corruption %r is applied in the model\'s forward by the pretraining '
                                          'models; nothing applies it in this protocol' % item)
        self.bs = config.get('bs', 64)
        self.count = config.get('count', 256)
        self.classes = int(config.get('classes', 3))
        self.labels = None

    def _materialise(self):
        listed = self.pc_path and self.data_path and os.path.exists(os.path.join(str(self.data_path), '%s.txt' % self.subset))
        if listed:
            clouds, self.ids = load_npy_clouds(self.pc_path, self.data_path, self.subset)
            clouds = clouds[:, :, :3]
            ranks = taxonomy_ranks(self.data_path)
            labels = np.array([ranks[tax] for tax, _ in self.ids], np.int64)
        else:
            seed = self.seed + (1000 if self.subset == 'train' else 2000)
            clouds, labels = labelled_clouds(self.count, max(self.dense, 2 * self.npoints), seed=seed, classes=self.classes)
            self.ids = [('synthetic', str(i)) for i in range(self.count)]
        self.count = clouds.shape[0]
        self._clouds = torch.from_numpy(np.ascontiguousarray(clouds)).to(self.device)
        self.labels = torch.from_numpy(labels).to(self.device)
        self.gen = torch.Generator(device=self._clouds.device)
        self.gen.manual_seed(self.seed)
        self.listed = bool(listed)
        self.steps = self.count // self.bs if self.subset == 'train' else -(-self.count // self.bs)

    def __iter__(self):
        if self._clouds is None:
            self._materialise()
        dev = self._clouds.device
        end = self.steps * self.bs if self.subset == 'train' else self.count
        for i in range(0, end, self.bs):
            sel = np.arange(i, min(i + self.bs, end))
            corrupted, _ = self.batch(_dev(sel, dev))
            tax, model_id = self.ids[i]
            yield tax, model_id, (corrupted[:, :, :3], self.labels[i:i + len(sel)])


@DATASETS.register_module()
class ModelNet:
    """Labelled clouds for the classification protocols (datasets/ModelNetDataset.py of the reference yields
    (taxonomy, model_id, (points, label))), resident on the device, batches of `bs`.  The `train` subset drops a short
    last batch, as the reference's train loader does (tools/builder.py: drop_last).

    Source: the reference's processed file `<DATA_PATH>/modelnet<NUM_CATEGORY>_<subset>_<N_POINTS>pts_fps.dat`
    (ModelNetDataset.py:93) -- a pickle of [list_of_points, list_of_labels], every cloud (N_POINTS, 6) float32, every
    label an int32 array of one element -- when it exists (`listed`); else labelled synthetic clouds
    (synthetic.labelled_clouds, `count` of them), exactly as before the file was ever looked for.  The first-run
    .txt -> .dat conversion and ModelNet_Official (HDF5) are not read.

    A listed set: `count` keeps the file's first clouds; USE_NORMALS false keeps columns 0..2; a leading 'norm' of
    aug_type is applied once per cloud at load with pc_normalize (a pure function of the stored cloud: what the
    reference's default run computes on every access), the remaining items are per-access maps.  set (S,P,C) f32 and
    labels (S,) i64 live on the device, on every rank.  Its `train` subset does on every access what the reference's
    loader does (ModelNetDataset.py:127-158, tools/builder.py:17-31): the items are shuffled once per epoch
    (epoch_items), every cloud gets fresh maps and a fresh shuffle of its points.  Two ways to iterate it, which consume
    the generators identically:
        iter_draws()  ('ModelNet', 'sample', (item (bs,) i32, perm (bs,P) i32, nmaps (bs,) i32, maps (bs,3,12) f32, labels))
                      -- resident_ops turns the draws into the step's input in one launch; offered when `resident`
        __iter__      ('ModelNet', i, (points (bs,P,C), labels)): the same draws as framework ops -- item select, the
                      maps through pipeline_norm_affine, the permutation gather
    More than three per-access maps, or a 'norm' that is not first, go through `augment` inside __iter__; `resident` is
    then False.  The other subsets yield every cloud in file order, the short last batch kept."""

    def __init__(self, config):
        self.npoints = config.get('npoints', 1024)
        self.bs = config.get('bs', 32)
        self.subset = config.get('subset', 'test')
        self.device = config.get('device', 'cuda')
        self.listed, self.resident = False, False
        path = None
        if config.get('DATA_PATH'):
            path = os.path.join(str(config.get('DATA_PATH')), 'modelnet%d_%s_%dpts_fps.dat' % (
                int(config.get('NUM_CATEGORY', 40)), self.subset, int(config.get('N_POINTS', self.npoints))))
        if path is not None and os.path.exists(path):
            self._init_listed(config, path)
            return
        self.source = 'synthetic stand-in (no %s)' % (path if path is not None else 'DATA_PATH')
        self.count = config.get('count', 256)
        seed = config.get('seed', 0) + (1000 if self.subset == 'train' else 2000)
        # `classes`: how many of the NUM_CATEGORY labels the synthetic clouds use (default 3)
        classes = int(config.get('classes', min(3, config.get('NUM_CATEGORY', 3))))
        x, y = labelled_clouds(self.count, self.npoints, seed=seed, classes=classes)
        rank, world = int(config.get('rank', 0)), max(int(config.get('world', 1)), 1)
        if world > 1:      # DistributedSampler(shuffle=False): wrap-padded to a multiple of world, every world-th item
            sel = np.resize(np.arange(self.count), -(-self.count // world) * world)[rank::world]
            x, y = x[sel], y[sel]
            self.count = len(sel)
        self.x, self.y = torch.from_numpy(x).to(self.device), torch.from_numpy(y).to(self.device)
        # augment_data (corrupt_util.py:1155-1175) of every batch, in the configured order, as ModelNetDataset does for the
        # fine-tuning configs ('norm', 'scale', 'translate'); 'clean' (the probe configs) and no key leave the clouds as they are
        self.aug_type = [a for a in config.get('aug_type', ['clean']) if a != 'clean']
        for item in self.aug_type:
            if item not in _AUGS:
                raise NotImplementedError('augmentation %r (implemented: %s)' % (item, ', '.join(_AUGS)))
        self.rng = np.random.default_rng(seed + 17) if self.aug_type else None
        self.access = self.aug_type

    def _init_listed(self, config, path):
        """The reference's processed file: the set and its labels on the device, a leading 'norm' applied at load."""
        import pickle
        with open(path, 'rb') as f:
            points, labels = pickle.load(f)
        count = config.get('count', None)
        if count is not None:
            points, labels = points[:int(count)], labels[:int(count)]
        use_normals = config.get('USE_NORMALS', False)
        use_normals = use_normals.lower() == 'true' if isinstance(use_normals, str) else bool(use_normals)
        self.aug_type = [a for a in config.get('aug_type', ['clean']) if a != 'clean']
        for item in self.aug_type:
            if item not in _AUGS:
                raise NotImplementedError('augmentation %r (implemented: %s)' % (item, ', '.join(_AUGS)))
        # per-access items: what is left behind a leading 'norm'.  Up to three maps and no further 'norm' is what one launch
        # of norm_affine / pdae_resident_batch takes; anything else keeps the whole list for `augment`
        rest = self.aug_type[1:] if self.aug_type[:1] == ['norm'] else self.aug_type
        fused = len(rest) <= 3 and 'norm' not in rest
        self.access = rest if fused else self.aug_type
        norm_at_load = fused and self.aug_type[:1] == ['norm']
        clouds = []
        for pts in points:
            pts = np.array(pts, np.float32)                              # (a copy: the pickle's list keeps the stored cloud)
            if norm_at_load:
                pts[:, 0:3] = pc_normalize(pts[:, 0:3])
            clouds.append(pts if use_normals else pts[:, 0:3])
        x = np.ascontiguousarray(np.stack(clouds, 0))
        y = np.array([int(np.asarray(label).reshape(-1)[0]) for label in labels], np.int64)
        self.seed = int(config.get('seed', 0))
        self.rank, self.world = int(config.get('rank', 0)), max(int(config.get('world', 1)), 1)
        if self.subset != 'train' and self.world > 1:   # DistributedSampler(shuffle=False), as for the synthetic clouds
            sel = np.resize(np.arange(len(x)), -(-len(x) // self.world) * self.world)[self.rank::self.world]
            x, y = x[sel], y[sel]
        self.count = len(x)
        self.set = self.x = torch.from_numpy(x).to(self.device)
        self.labels = self.y = torch.from_numpy(y).to(self.device)
        self.listed = True
        self.resident = self.subset == 'train' and fused
        self.source = '%s (%d clouds of %d points, %d channels)' % (path, self.count, x.shape[1], x.shape[2])
        self.rng = np.random.default_rng(self.seed + (1000 if self.subset == 'train' else 2000) + 17)
        self.gen = torch.Generator(device=self.set.device)
        self.gen.manual_seed(self.seed)
        self._epoch, self._epoch_set = -1, False

    def __len__(self):
        if self.listed and self.subset == 'train':       # DistributedSampler pads to ceil(S / world); drop_last
            return -(-self.count // self.world) // self.bs
        if self.subset == 'train':                       # the reference's train loader: drop_last (tools/builder.py)
            return self.count // self.bs
        return (self.count + self.bs - 1) // self.bs

    def set_epoch(self, epoch):
        """DistributedSampler.set_epoch: the next iteration of a listed train subset draws epoch `epoch`'s permutation;
        without it the epochs count from 0."""
        self._epoch, self._epoch_set = int(epoch), True

    def draw_maps(self, B):
        """The per-access maps of B clouds, draw_affine_map(rng, 'aug_' + item) cloud by cloud, in pdae_pipeline_norm_affine's
        layout -> (nmaps (B,) int32, maps (B,3,12) float32: M 3x3 row-major then t; unused entries the identity), host."""
        packed = np.zeros((B, 3, 12), np.float32)
        packed[:, :, 0] = packed[:, :, 4] = packed[:, :, 8] = 1.0
        for b in range(B):
            for q, item in enumerate(self.access):
                M, t = draw_affine_map(self.rng, 'aug_' + item)
                packed[b, q, :9], packed[b, q, 9:] = M.reshape(-1), t
        return np.full(B, len(self.access), np.int32), packed

    def iter_draws(self):
        """One epoch of a listed train subset as draws: ('ModelNet', 'sample', (item, perm, nmaps, maps, labels)), all on
        the device.  The batch is T_b(set[item[b]][perm[b]]) with T_b row b's nmaps[b] maps in order."""
        if not self.resident:
            raise RuntimeError('ModelNet.iter_draws: a listed train subset whose per-access augmentation is at most three '
                               'maps (resident) is required')
        return self._draws()

    def _draws(self):
        dev, P = self.set.device, self.set.shape[1]
        if not self._epoch_set:
            self._epoch += 1
        self._epoch_set = False
        items = epoch_items(self.count, self.seed - self.rank, self._epoch, self.rank, self.world, self.bs)
        for row in items:
            item = _dev(row.astype(np.int32), dev)
            perm = torch.rand((self.bs, P), generator=self.gen, device=dev).argsort(1).to(torch.int32)
            if self.resident:
                nmaps, maps = self.draw_maps(self.bs)
                nmaps, maps = _dev(nmaps, dev), _dev(maps, dev)
            else:
                nmaps = maps = None
            yield 'ModelNet', 'sample', (item, perm, nmaps, maps, self.labels.index_select(0, item.long()))

    def _mapped(self, x, fn):
        """fn on the coordinates of x (B,P,C), the other channels untouched."""
        if x.shape[2] == 3:
            return fn(x.contiguous())
        return torch.cat([fn(x[:, :, :3].contiguous()), x[:, :, 3:]], 2)

    def augment(self, x):
        """augment_data of one batch on csrc/pipeline.hip: a 'norm' normalises everything drawn before it first (the kernel
        normalises before it applies its <= 3 maps), every other item is one affine map per cloud."""
        B = x.shape[0]
        maps, norm_pending = [[] for _ in range(B)], False

        def flush(x, norm_pending, maps):
            while norm_pending or any(maps):
                x = pipeline_norm_affine(x, norm_pending, [m[:3] for m in maps] if any(maps) else None)
                maps, norm_pending = [m[3:] for m in maps], False
            return x
        for item in self.access:
            if item == 'norm':
                x = flush(x, norm_pending, maps)
                maps, norm_pending = [[] for _ in range(B)], True
                continue
            for b in range(B):
                maps[b].append(draw_affine_map(self.rng, 'aug_' + item))
        return flush(x, norm_pending, maps)

    def __iter__(self):
        if self.listed and self.subset == 'train':
            # the draws of iter_draws as framework ops: item select, the maps, the permutation gather
            C = self.set.shape[2]
            for i, (_, _, (item, perm, nmaps, maps, labels)) in enumerate(self._draws()):
                x = self.set.index_select(0, item.long())
                if self.resident:
                    x = self._mapped(x, lambda xyz: pipeline_norm_affine(xyz, False, (nmaps, maps)))
                elif self.access:
                    x = self._mapped(x, self.augment)
                x = torch.gather(x, 1, perm.long().unsqueeze(-1).expand(-1, -1, C)).contiguous()
                yield 'ModelNet', i * self.bs, (x, labels)
            return
        # a train subset yields only full batches, as the reference's DataLoader(drop_last=True) does; every other
        # subset yields every cloud, its last batch short
        end = len(self) * self.bs if self.subset == 'train' else self.count
        for i in range(0, end, self.bs):
            x = self.x[i:i + self.bs]
            if self.access:
                x = self._mapped(x, self.augment) if self.listed else self.augment(x)
            yield 'ModelNet', i, (x, self.y[i:i + self.bs])


def epoch_items(count, seed, epoch, rank, world, bs):
    """The items of one epoch of a listed train loader on one rank, as DistributedSampler(shuffle=True) + DataLoader(
    drop_last=True) arrange them (tools/builder.py:17-31): ONE permutation of 0..count-1 from a generator seeded with
    (seed, epoch) -- `seed` is the one all ranks share --, wrap-padded to a multiple of world, rank r takes [r::world],
    floor(n / bs) full batches.  -> (batches, bs) int64."""
    shared = np.random.default_rng([int(seed), int(epoch)]).permutation(int(count))
    world = max(int(world), 1)
    mine = np.resize(shared, -(-int(count) // world) * world)[int(rank)::world]
    full = len(mine) // int(bs)
    return mine[:full * bs].reshape(full, bs).astype(np.int64)


def pc_normalize(pc):
    """datasets/ModelNetDatasetFewShot.py:21-26, the reference's numpy expression in the array's own precision."""
    centroid = np.mean(pc, axis=0)
    pc = pc - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    pc = pc / m
    return pc


@functools.lru_cache(maxsize=2)                 # (the train and the test loader of a run ask for the same episode)
def synthetic_episode(seed, way, shot, fold, n_points, eval_sample=20):
    """An episode built the way datasets/generate_few_shot_data.py builds one, from synthetic.labelled_clouds: `way`
    classes, `shot` training and `eval_sample` test clouds of each, labels 0..way-1, both lists shuffled; a function of
    (seed, way, shot, fold).  labelled_clouds knows three primitive families: class i is family i % 3, flattened along z
    by 1 / (1 + i // 3) and normalised again, so that classes of one family still differ.
    -> {'train': [(points (n_points,3) f32, label, key)], 'test': [...]}, the reference's pickle format."""
    rng = np.random.default_rng([int(seed), int(way), int(shot), int(fold)])
    need = shot + eval_sample
    lists = {'train': [], 'test': []}
    for i in range(way):
        got = []
        while len(got) < need:
            x, y = labelled_clouds(3 * need, n_points, seed=int(rng.integers(1 << 31)), classes=3)
            got += list(x[y == i % 3])
        for n, pts in enumerate(got[:need]):
            pts = pts * np.array([1.0, 1.0, 1.0 / (1 + i // 3)], np.float32)
            lists['train' if n < shot else 'test'].append((pc_normalize(pts).astype(np.float32), i, i))
    return {k: [v[j] for j in rng.permutation(len(v))] for k, v in lists.items()}


@DATASETS.register_module()
class ModelNetFewShot:
    """One few-shot episode (datasets/ModelNetDatasetFewShot.py of the reference), resident on the device.

    Source: `<DATA_PATH>/<way>way_<shot>shot/<fold>.pkl`, the reference's pickle -- {'train' / 'test': [(points (P, 3 or
    6), label, key)]} -- when it exists, else synthetic_episode.  pc_normalize runs once per cloud at load, on the host
    (the reference's workers re-fork from the un-normalised parent every epoch, so once per cloud is what its default
    run computes); USE_NORMALS false keeps three channels.  way, shot or fold of -1: RuntimeError, as there.  The
    config's aug_type is accepted and ignored, as in the reference's class.

    `train` yields ('ModelNet', 'sample', (item (bs,) i32, perm (bs, P) i32, labels (bs,) i64)) -- the batch is
    self.set[item] with row b's points in the order perm[b]; fewshot_ops turns it into the step's input: the items of an
    epoch are torch.randperm on the seeded device generator, floor(S / bs) full batches, and per batch
    torch.rand(bs, P).argsort(1) is the point shuffle.  `test` yields ('ModelNet', 'sample', (points (b, P, C), labels
    (b,))) in list order, the short last batch kept, nothing drawn."""

    fewshot = True

    def __init__(self, config):
        self.subset = config.get('subset', 'train')
        self.bs = config.get('bs', 32)
        self.device = config.get('device', 'cuda')
        self.seed = int(config.get('seed', 0))
        self.way, self.shot, self.fold = (int(config.get(k, -1)) for k in ('way', 'shot', 'fold'))
        if self.way == -1 or self.shot == -1 or self.fold == -1:
            raise RuntimeError('ModelNetFewShot: --way, --shot and --fold are required')
        use_normals = config.get('USE_NORMALS', False)
        use_normals = use_normals.lower() == 'true' if isinstance(use_normals, str) else bool(use_normals)
        path = os.path.join(str(config.get('DATA_PATH', '')), '%dway_%dshot' % (self.way, self.shot), '%d.pkl' % self.fold)
        self.listed = os.path.exists(path)
        if self.listed:
            import pickle
            with open(path, 'rb') as f:
                items = pickle.load(f)[self.subset]
        else:
            n_points = int(config.get('N_POINTS', config.get('npoints', 8192)))
            items = synthetic_episode(self.seed, self.way, self.shot, self.fold, n_points)[self.subset]
        clouds = []
        for points, _, _ in items:
            points = np.array(points)                                   # (a copy: the list keeps the stored cloud)
            points[:, 0:3] = pc_normalize(points[:, 0:3])
            clouds.append((points if use_normals else points[:, 0:3]).astype(np.float32))
        self.set = torch.from_numpy(np.ascontiguousarray(np.stack(clouds, 0))).to(self.device)
        self.labels = torch.from_numpy(np.array([int(np.asarray(label).reshape(-1)[0]) for _, label, _ in items],
                                                np.int64)).to(self.device)
        self.count = self.set.shape[0]
        self.aug_type = ['norm']              # (runner_finetune.fps_cacheable: the clouds are the same on every pass)
        self.gen = torch.Generator(device=self.set.device)
        self.gen.manual_seed(self.seed)

    def __len__(self):
        if self.subset == 'train':
            return self.count // self.bs
        return (self.count + self.bs - 1) // self.bs

    def __iter__(self):
        dev, P = self.set.device, self.set.shape[1]
        if self.subset != 'train':
            for i in range(0, self.count, self.bs):
                yield 'ModelNet', 'sample', (self.set[i:i + self.bs], self.labels[i:i + self.bs])
            return
        order = torch.randperm(self.count, generator=self.gen, device=dev)
        for i in range(len(self)):
            item = order[i * self.bs:(i + 1) * self.bs]
            perm = torch.rand((self.bs, P), generator=self.gen, device=dev).argsort(1).to(torch.int32)
            yield 'ModelNet', 'sample', (item.to(torch.int32), perm, self.labels.index_select(0, item))


def read_shapenetpart(root, split):
    """The file list of segmentation/dataset.py:65-122 (PartNormalDataset.__init__) -> (categories [(name, directory)] in
    the order of synsetoffset2category.txt, items [(category index, path)] category by category, file names sorted)."""
    import json
    cats = []
    with open(os.path.join(root, 'synsetoffset2category.txt')) as f:
        for line in f:
            ls = line.strip().split()
            if ls:
                cats.append((ls[0], ls[1]))
    ids = {}
    for part in ('train', 'val', 'test'):
        with open(os.path.join(root, 'train_test_split', 'shuffled_%s_file_list.json' % part)) as f:
            ids[part] = set(str(d.split('/')[2]) for d in json.load(f))
    wanted = {'trainval': ids['train'] | ids['val'], 'train': ids['train'], 'val': ids['val'], 'test': ids['test']}
    if split not in wanted:
        raise ValueError('ShapeNetPart: unknown split %r (trainval, train, val, test)' % (split,))
    items = []
    for k, (_, directory) in enumerate(cats):
        for fn in sorted(os.listdir(os.path.join(root, directory))):
            if fn[0:-4] in wanted[split]:
                items.append((k, os.path.join(root, directory, os.path.splitext(fn)[0] + '.txt')))
    return cats, items


def synthetic_part_shapes(count, npoints, seed):
    """The stand-in of ShapeNetPart: `count` seeded shapes in the unit ball (synthetic.labelled_clouds' primitives), each
    of npoints .. 1.25 npoints points; the categories are drawn as shuffled rounds of the 16, so every 16 consecutive
    shapes cover them all; part labels inside the category's range by a geometric rule -- equal slabs along x -- so any
    point's label, seg[i, 0] included, identifies the category.  -> (clouds [(P_i, 3) f32], cls (count,) i64, segs [(P_i,) i32])."""
    from .partseg_ops import label_tables
    _, lo, hi = label_tables()
    rng = np.random.default_rng(seed)
    rounds = -(-count // len(lo))
    cls = np.concatenate([rng.permutation(len(lo)) for _ in range(rounds)])[:count].astype(np.int64)
    clouds, segs = [], []
    for i in range(count):
        P = int(rng.integers(npoints, npoints + npoints // 4 + 1))
        x, _ = labelled_clouds(1, P, seed=int(rng.integers(1 << 31)), classes=3)
        x = x[0]
        n = int(hi[cls[i]] - lo[cls[i]] + 1)
        t = (x[:, 0] - x[:, 0].min()) / max(float(x[:, 0].max() - x[:, 0].min()), 1e-12)
        segs.append((lo[cls[i]] + np.minimum((t * n).astype(np.int32), n - 1)).astype(np.int32))
        clouds.append(x)
    return clouds, cls, segs


@DATASETS.register_module()
class ShapeNetPart:
    """Shapes with per-point part labels for part segmentation (segmentation/dataset.py:65-167 PartNormalDataset of the
    reference yields (point_set (npoints, 3), cls (1,), seg (npoints,))), resident on the device as ONE ragged buffer --
    points (sum P_i, 3) f32, seg (sum P_i,) i32 -- plus offsets; batches of `bs`: (points (B, N, 3), cls (B,) i64,
    seg (B, N) i32).  Splits trainval / train / val / test (`subset`).  Columns 0:3 and the last column of every file
    are read (normals are not), pc_normalize is applied once per shape at load (a pure function of the stored shape:
    what the reference computes on every access).  Per access the reference's np.random.choice(P_i, npoints,
    replace=True) is drawn on the host generator and the gather runs on the device; the reference draws inside its
    loader's worker processes, so the distribution is matched, not its draws.  Every shape in file order, the short last
    batch kept.  Where DATA_PATH does not exist: synthetic_part_shapes (`count` of them)."""

    def __init__(self, config):
        self.npoints = int(config.get('npoints', 2048))
        self.bs = int(config.get('bs', 16))
        self.subset = config.get('subset', 'test')
        self.device = config.get('device', 'cuda')
        self.seed = int(config.get('seed', 0))
        root = config.get('DATA_PATH')
        self.listed = bool(root) and os.path.isdir(str(root))
        if self.listed:
            self.categories, items = read_shapenetpart(str(root), self.subset)
            count = config.get('count', None)
            if count is not None:
                items = items[:int(count)]
            clouds, segs = [], []
            for _, path in items:
                data = np.loadtxt(path, ndmin=2).astype(np.float32)
                clouds.append(pc_normalize(data[:, 0:3]).astype(np.float32))
                segs.append(data[:, -1].astype(np.int32))
            cls = np.array([k for k, _ in items], np.int64)
            self.paths = [p for _, p in items]
            self.source = '%s (%s: %d shapes of %d categories)' % (root, self.subset, len(items), len(self.categories))
        else:
            self.source = 'synthetic stand-in (no %s)' % (root if root else 'DATA_PATH')
            clouds, cls, segs = synthetic_part_shapes(int(config.get('count', 64)), self.npoints,
                                                      self.seed + {'test': 2000, 'val': 3000}.get(self.subset, 1000))
        self.count = len(clouds)
        self.offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        cat = (lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, np.float32))
        self.points = torch.from_numpy(np.ascontiguousarray(cat(clouds, (0, 3)), np.float32)).to(self.device)
        self.seg = torch.from_numpy(np.ascontiguousarray(cat(segs, (0,))).astype(np.int32)).to(self.device)
        self.cls = torch.from_numpy(cls).to(self.device)
        self.rng = np.random.default_rng(self.seed + 29)

    def __len__(self):
        return (self.count + self.bs - 1) // self.bs

    def draw(self, items):
        """The per-access resampling of `items`: flat rows (len(items), npoints) int64 into the ragged buffer, host."""
        rows = np.empty((len(items), self.npoints), np.int64)
        for j, i in enumerate(items):
            P = int(self.offsets[i + 1] - self.offsets[i])
            rows[j] = self.offsets[i] + self.rng.choice(P, self.npoints, replace=True)
        return rows

    def __iter__(self):
        for i in range(0, self.count, self.bs):
            items = range(i, min(i + self.bs, self.count))
            rows = torch.from_numpy(self.draw(items)).to(self.points.device)
            flat = rows.reshape(-1)
            pts = self.points.index_select(0, flat).reshape(len(items), self.npoints, 3)
            seg = self.seg.index_select(0, flat).reshape(len(items), self.npoints)
            yield 'ShapeNetPart', i, (pts, self.cls[i:i + len(items)], seg)
