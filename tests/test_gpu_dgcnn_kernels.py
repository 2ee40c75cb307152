"""csrc/dgcnn.hip kernel by kernel against fp64: the EdgeConv and cloud-pool entry points called one at a time through
point_dae_amd._lib exactly as point_cae_dgcnn._Encoder calls them, at every width the argument checks accept, on graphs
the kNN never builds (hubs, isolated points, no self-loops), with planted exact ties and with point ids >= 32768.
tests/test_gpu_dgcnn.py holds the encoder as a whole to relative L2 tolerances; here every output ELEMENT is held either
bit for bit or to a forward error bound that is derived where it is used.

Conventions of the bounds: u = 2^-24 (fp32 unit roundoff; the library is built with -ffp-contract=off, so every fp32
operation rounds once), (1 + u)^m - 1 is taken as m u (m^2 u << 1 at every size used here), and "A" is the reference
expression with every LEAF term (p, q, mean, g, c1, ...) replaced by its absolute value.  Inputs are the fp32 numbers the
kernels read, so the fp64 references start from exactly the same values.  Sums the kernels keep in fp64 get
kF64 = 1e-13 relative to the sum of absolute values: at most a few hundred sequential fp64 additions per chain
(count x 2^-53 < 1e-13 for count < 900) plus the pairwise error of the reference's own fp64 sum.

Section 6 (one EdgeConv layer / the pool as the product chains the kernels, against autograd in fp64) has no derived
bound.  Its yardstick is the same dense formulation in fp32 PyTorch on the GPU, measured in the same test; the
tolerances are 4 x the largest yardstick error recorded on an MI355X per output kind (two bits for the kernels'
different summation order: fp32 partials per row, then fp64).  Seven cases, all on their first seed (fp32 runs on a CPU
had suggested a yardstick of 3.2e-7, a tolerance of 1.3e-6):

    output kind      fp32 PyTorch, max over the cases     kernels, max over the cases     tolerance (4 x yardstick)
    out              1.610e-7                             1.61e-7                         6.440e-7
    dpq / dy         1.787e-7                             1.51e-7                         7.148e-7
    dgamma           1.897e-7                             1.23e-7                         7.588e-7
    dbeta            0.741e-7                             0.37e-7                         2.964e-7
    running          1.562e-7                             0.85e-7                         6.248e-7
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
kF64 = 1e-13
EPS = 1e-5
BAND = 16 * U          # |y64| below BAND (|e scale| + |shift|): the fp32 y may fall on either side of LeakyReLU's kink
DEV = 'cuda'
YARDSTICK = {'out': 1.610e-7, 'dx': 1.787e-7, 'dgamma': 1.897e-7, 'dbeta': 0.741e-7, 'running': 1.562e-7}     # the table above
CHAIN_TOL = {kind: 4 * y for kind, y in YARDSTICK.items()}


def _L():
    from point_dae_amd import _lib
    return _lib


def _t(a):
    return torch.from_numpy(a) if isinstance(a, np.ndarray) else a


def _up(a):
    return _t(a).to(DEV).contiguous()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def _written(*tensors):
    for t in tensors:
        assert torch.isfinite(t).all(), 'an output buffer kept its NaN fill'


def _within(got, ref, bound, what):
    err = (_t(got).double() - ref).abs()
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err[bad] / bound[bad].clamp_min(1e-30)).max()))


def _err(a, ref):
    """tests/test_gpu_block.py _close's measure: max |a - ref| / max |ref|."""
    return (a.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item() / (ref.abs().max().item() + 1e-12)


# ---- inputs -------------------------------------------------------------------------------------------------------
def _values(rng, rows, C):
    """ordinary value ranges: per-channel std in [0, 2], per-channel mean within +-1 std"""
    std = rng.uniform(0.0, 2.0, C)
    mean = rng.uniform(-1.0, 1.0, C) * std
    return (rng.standard_normal((rows, C)) * std + mean).astype(np.float32)


def _gamma(C):
    g = np.linspace(-1.0, 1.5, C).astype(np.float32)           # as test_encoder_equals_the_dense_edge_formulation:
    g[::7] = 0.0                                               # negative, positive and exactly-zero entries
    return g


def _beta(C):
    # (not the encoder test's linspace: with two rows xhat = +-1 and y = +-gamma + beta, and the two linspaces cross at
    # |gamma| = |beta| in one channel, which puts that element ON the kink by construction)
    return (0.3 * np.sin(1.0 + 0.7 * np.arange(C))).astype(np.float32)


def _bn_like(x2d, gamma, beta):
    """scale, shift, mean, invstd (fp32) of a training-mode BatchNorm over the rows of x2d"""
    x = x2d.astype(np.float64)
    mean = x.mean(0).astype(np.float32)
    invstd = (1.0 / np.sqrt(x.var(0) + EPS)).astype(np.float32)
    scale = (gamma * invstd).astype(np.float32)
    shift = (beta - mean * scale).astype(np.float32)
    return scale, shift, mean, invstd


def _graph(kind, B, N, k, rng):
    """(B, N, k) int32 neighbour ids, distinct within a row.  self: a random k-subset with the point itself at position
    0 (the kNN shape); noself: a random k-subset without the point; hub: noself with position 0 one of points 0..3
    (in-degree about N / 4 on four points, many points with in-degree 0)."""
    key = rng.random((B, N, N))
    r = np.arange(N)
    if kind == 'self':
        key[:, r, r] = -1.0
    else:
        assert k <= N - 1 and N >= 4
        key[:, r, r] = 2.0
        if kind == 'hub':
            h = rng.integers(0, 4, size=(B, N))
            h = np.where(h == r[None, :], (h + 1) % 4, h)
            key[np.arange(B)[:, None], r[None, :], h] = -1.0
    return np.argsort(key, axis=2, kind='stable')[:, :, :k].astype(np.int32)


def _graph_big(N, split, rng):
    """one cloud of N > 32768 points, k = 3: the point itself and two others of ITS side of `split`, in random order --
    every row >= split lists only ids >= split, which a signed 16-bit winner id cannot hold"""
    r = np.arange(N)
    base = np.where(r < split, 0, split)
    size = np.where(r < split, split, N - split)
    assert N - split > 6000
    d1, d2 = rng.integers(1, 3000, N), rng.integers(3000, 6000, N)
    idx = np.stack([r, base + (r - base + d1) % size, base + (r - base + d2) % size], 1)
    idx = np.take_along_axis(idx, np.argsort(rng.random((N, 3)), 1), 1)
    return idx[None].astype(np.int32)


def _plant_ties(pq, idx, co, rng, want=300):
    """copy the p half of one neighbour's row onto a LATER neighbour's row of the same point: two edges of that point then
    have identical e in every channel.  A row that took part is not written again, so every planted tie survives."""
    B, N, k = idx.shape
    planted = []
    if k < 2:
        return planted
    frozen = np.zeros(B * N, dtype=bool)
    for r in rng.permutation(B * N)[:4 * want]:
        a, c = sorted(rng.choice(k, size=2, replace=False))
        b = r // N
        s, t = b * N + idx[b, r % N, a], b * N + idx[b, r % N, c]
        if frozen[t]:
            continue
        pq[t, :co] = pq[s, :co]
        frozen[s] = frozen[t] = True
        planted.append((int(r), int(a), int(c)))
        if len(planted) >= want:
            break
    return planted


def _flat(idx):
    B, N, k = idx.shape
    return torch.from_numpy((idx.astype(np.int64) + (np.arange(B, dtype=np.int64) * N)[:, None, None]).reshape(B * N, k))


# ---- the entry points, called as point_cae_dgcnn._Encoder calls them: host tensors in, host tensors out --------------
def run_gather(pq, idx, gamma, co):
    L = _L()
    B, N, k = idx.shape
    R = B * N
    pq, idx, gamma = _up(pq), _up(idx), _up(gamma)
    esel, psum = _nan((R, co)), _nan((R, co))
    sel = torch.full((R, co), -1, dtype=torch.int16, device=DEV)               # 65535: no valid id (n <= 65535)
    part = _nan((L.lib().pdae_edge_parts(), 2 * co), torch.float64)             # _parts() of point_cae_dgcnn
    sums = _nan((2 * co,), torch.float64)
    L.call('pdae_edge_gather_stats', pq, B, N, k, co, pq.data_ptr(), idx.data_ptr(), gamma.data_ptr(), esel.data_ptr(),
           sel.data_ptr(), psum.data_ptr(), part.data_ptr(), sums.data_ptr())
    _written(esel, psum, part, sums)
    return esel.cpu(), sel.cpu(), psum.cpu(), sums.cpu()


def run_bn_rows(e, scale, shift, wide=None, off=0):
    """-> out (, the wider tensor after the call when `wide` (R, ld2) is given: out2 = its columns off .. off + C)"""
    L = _L()
    R, C = e.shape
    e, scale, shift = _up(e), _up(scale), _up(shift)
    out = _nan((R, C))
    w = _up(wide) if wide is not None else None
    L.call('pdae_bn_lrelu_rows', e, R, C, e.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(),
           w.data_ptr() + 4 * off if w is not None else None, w.shape[1] if w is not None else 0)
    _written(out)
    return (out.cpu(), w.cpu()) if w is not None else out.cpu()


def run_bn_backward(d1, d2wide, off, e, scale, shift, mean, invstd, with_param_grads=True):
    """d2wide: None or a (R, ld2) tensor whose columns off .. off + C are d2 -> g, sums, dgamma, dbeta"""
    L = _L()
    R, C = e.shape
    e, scale, shift, mean, invstd = _up(e), _up(scale), _up(shift), _up(mean), _up(invstd)
    d1 = _up(d1) if d1 is not None else None
    w = _up(d2wide) if d2wide is not None else None
    g = _nan((R, C))
    part = _nan((L.lib().pdae_edge_parts(), 2 * C), torch.float64)
    sums = _nan((2 * C,), torch.float64)
    dgamma, dbeta = (_nan((C,)), _nan((C,))) if with_param_grads else (None, None)
    L.call('pdae_bn_lrelu_backward_reduce', e, R, C, L.ptr(d1), w.data_ptr() + 4 * off if w is not None else None,
           w.shape[1] if w is not None else 0, e.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
           invstd.data_ptr(), g.data_ptr(), part.data_ptr(), sums.data_ptr(), L.ptr(dgamma), L.ptr(dbeta))
    _written(g, sums)
    if with_param_grads:
        _written(dgamma, dbeta)
        return g.cpu(), sums.cpu(), dgamma.cpu(), dbeta.cpu()
    return g.cpu(), sums.cpu(), None, None


def run_reverse(idx):
    """rev_start (B, N + 1), rev_src (B, N k): pdae_knn_reverse (tests/test_gpu_dgcnn.py guards it); clouds it refuses
    (n > 4096): built here as that test builds its expectation"""
    B, N, k = idx.shape
    if N > 4096:
        start, src = np.empty((B, N + 1), np.int32), np.empty((B, N * k), np.int32)
        rows = np.repeat(np.arange(N), k)
        for b in range(B):
            tgt = idx[b].reshape(-1)
            src[b] = rows[np.lexsort((rows, tgt))]
            start[b] = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=N))])
        return torch.from_numpy(start), torch.from_numpy(src)
    L = _L()
    t = _up(idx)
    start = torch.full((B, N + 1), -1, dtype=torch.int32, device=DEV)
    src = torch.full((B, N * k), -1, dtype=torch.int32, device=DEV)
    L.call('pdae_knn_reverse', t, B, N, k, t.data_ptr(), start.data_ptr(), src.data_ptr())
    assert start.min().item() >= 0 and src.min().item() >= 0
    return start.cpu(), src.cpu()


def run_edge_backward(dims, g, pq, sel, psum, rev_start, rev_src, scale, mean, invstd, sums):
    L = _L()
    B, N, k, co = dims
    g, pq, sel, psum, rev_start, rev_src = _up(g), _up(pq), _up(sel), _up(psum), _up(rev_start), _up(rev_src)
    scale, mean, invstd, sums = _up(scale), _up(mean), _up(invstd), _up(sums)
    dpq = _nan((B * N, 2 * co))
    L.call('pdae_edge_backward', g, B, N, k, co, g.data_ptr(), pq.data_ptr(), sel.data_ptr(), psum.data_ptr(),
           rev_start.data_ptr(), rev_src.data_ptr(), scale.data_ptr(), mean.data_ptr(), invstd.data_ptr(), sums.data_ptr(),
           dpq.data_ptr())
    _written(dpq)
    return dpq.cpu()


def pool_splits(B, n):
    return _L().lib().pdae_cloud_pool_splits(B, n)


def run_pool_stats(y, gamma):
    """y (B, n, C) -> ysel, arow (B, C), sums (2 C)"""
    L = _L()
    B, n, C = y.shape
    rs = pool_splits(B, n)
    y, gamma = _up(y), _up(gamma)
    ysel, arow = _nan((B, C)), torch.full((B, C), -1, dtype=torch.int32, device=DEV)
    pv, pr = _nan((B, rs, C)), torch.full((B, rs, C), -1, dtype=torch.int32, device=DEV)
    part, sums = _nan((B * rs, 2 * C), torch.float64), _nan((2 * C,), torch.float64)
    L.call('pdae_cloud_pool_stats', y, B, n, C, y.data_ptr(), gamma.data_ptr(), ysel.data_ptr(), arow.data_ptr(),
           pv.data_ptr(), pr.data_ptr(), part.data_ptr(), sums.data_ptr())
    _written(ysel, pv, part, sums)
    for rows in (arow, pr):
        assert rows.min().item() >= 0 and rows.max().item() < n
    return ysel.cpu(), arow.cpu(), sums.cpu()


def run_pool_backward(y, g, arow, scale, mean, invstd, sums):
    L = _L()
    B, n, C = y.shape
    y, g, arow, scale, mean, invstd, sums = _up(y), _up(g), _up(arow), _up(scale), _up(mean), _up(invstd), _up(sums)
    dy = _nan((B * n, C))
    L.call('pdae_cloud_pool_backward', y, B, n, C, y.data_ptr(), g.data_ptr(), arow.data_ptr(), scale.data_ptr(),
           mean.data_ptr(), invstd.data_ptr(), sums.data_ptr(), dy.data_ptr())
    _written(dy)
    return dy.cpu().view(B, n, C)


class _Norm:
    """what rows.bn_finalize reads of a BatchNorm module"""

    def __init__(self, gamma, beta):
        C = len(gamma)
        self.weight, self.bias = _up(gamma), _up(beta)
        self.running_mean, self.running_var = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        self.num_batches_tracked = torch.zeros((), dtype=torch.long, device=DEV)
        self.eps, self.momentum, self.track_running_stats = EPS, 0.1, True


def run_finalize(gamma, beta, rows, sums):
    """rows.bn_finalize on fresh running estimates -> scale, shift, mean, invstd, running_mean, running_var"""
    from point_dae_amd.rows import bn_finalize
    bn = _Norm(gamma, beta)
    out = bn_finalize(bn, rows, bn.weight, stats64=_up(sums))
    assert bn.num_batches_tracked.item() == 1
    return tuple(t.cpu() for t in out) + (bn.running_mean.cpu(), bn.running_var.cpu())


def run_weights(name, cos, cins, kps, srcs, multi):
    """pdae_edge_weight_stack / _unstack over lists: one _multi launch, or one single call per job -> the outputs"""
    L = _L()
    unstack = 'unstack' in name
    srcs = [_up(s) for s in srcs]
    dsts = [_nan((co, 2 * cin)) if unstack else _nan((2 * co, kp)) for co, cin, kp in zip(cos, cins, kps)]
    if multi:
        L.edge_weights_multi(name + '_multi', srcs[0], cos, cins, kps, srcs, dsts)
    else:
        for co, cin, kp, s, d in zip(cos, cins, kps, srcs, dsts):
            L.call(name, s, co, cin, kp, s.data_ptr(), d.data_ptr())
    _written(*dsts)
    return [d.cpu() for d in dsts]


def run_rows_pad(x, cp):
    L = _L()
    R, c = x.shape
    x = _up(x)
    out = _nan((R, cp))
    L.call('pdae_rows_pad', x, R, c, cp, x.data_ptr(), out.data_ptr())
    _written(out)
    return out.cpu()


# ---- the EdgeConv cases: inputs and the forward kernel's records, made once ------------------------------------------
EDGE_CASES = [(1, 21, 20, 64, 'self'),          # k close to N
              (3, 100, 20, 16, 'noself'),
              (8, 40, 7, 32, 'hub'),            # exactly 8 clouds (the XCD-aware row order: clouds x, x + 8, ...)
              (9, 64, 20, 128, 'hub'),          # more than 8 clouds, no multiple of 8
              (17, 33, 5, 256, 'self'),
              (2, 77, 20, 512, 'noself'),
              (2, 50, 3, 1024, 'hub'),
              (1, 1, 1, 64, 'self'),            # n = k = 1
              (1, 40000, 3, 16, 'big')]         # ids >= 32768: a signed-16 slip shows in sel
_edge_cache = {}


def _edge_case(case):
    if case not in _edge_cache:
        B, N, k, co, kind = case
        rng = np.random.default_rng([B, N, k, co])
        idx = _graph_big(N, 32768, rng) if kind == 'big' else _graph(kind, B, N, k, rng)
        pq = _values(rng, B * N, 2 * co)
        planted = _plant_ties(pq, idx, co, rng)
        gamma = _gamma(co)
        esel, sel, psum, sums = run_gather(pq, idx, gamma, co)
        _edge_cache[case] = dict(idx=idx, pq=pq, planted=planted, gamma=gamma, esel=esel, sel=sel, psum=psum, sums=sums)
    return _edge_cache[case]


def _edges32(c, co):
    """e32 = p32[idx] + q32 (R, k, co): ONE fp32 addition per edge, done by torch -- bit for bit what the kernel adds"""
    pq = torch.from_numpy(c['pq'])
    P = pq[:, :co][_flat(c['idx'])]
    return P, P + pq[:, co:].unsqueeze(1)


def _first_winner(e, gamma):
    """numpy's first-occurrence argmax of +-e over axis 1 (the sign of gamma picks max or min), 0 where gamma == 0:
    torch.max's rule on lrelu(bn(e)), which is monotone in e"""
    j = (e * np.sign(gamma)).argmax(axis=1)
    j[:, gamma == 0] = 0
    return j


# ---- 1. edge_gather_stats -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', EDGE_CASES, ids=str)
def test_edge_gather_stats_winners_bit_exact_and_sums_within_the_summation_bound(case):
    B, N, k, co, kind = case
    R = B * N
    c = _edge_case(case)
    idx, gamma = c['idx'], c['gamma']
    P, e32 = _edges32(c, co)
    e = e32.numpy()
    for r, a, b in c['planted']:                                       # the planted ties are exact, in every channel
        assert np.array_equal(e[r, a], e[r, b])
    j = _first_winner(e, gamma)
    if c['planted']:
        rows = np.array([p[0] for p in c['planted']])
        first = np.array([p[1] for p in c['planted']])
        decisive = (j[rows] == first[:, None]) & (gamma != 0)[None, :]
        assert decisive.any(), 'no planted tie is a winner: the case cannot tell > from >='
    if k >= 2 and R >= 8:
        assert len(c['planted']) >= min(300, R // 8)
    want_e = np.take_along_axis(e, j[:, None, :], 1)[:, 0]
    want_sel = idx.reshape(R, k).astype(np.int64)[np.arange(R)[:, None], j]
    assert torch.equal(c['esel'], torch.from_numpy(want_e))
    got_sel = c['sel'].numpy().view(np.uint16).astype(np.int64)
    assert got_sel.max() < N
    assert np.array_equal(got_sel, want_sel)
    if kind == 'big':
        assert (want_sel[32768:] >= 32768).all()
    # psum = ((p_0 + p_1) + ...) + p_{k-1} in fp32, k - 1 additions (0 + p_0 is exact): recursive summation,
    # |got - sum p| <= ((1 + u)^(k-1) - 1) sum |p| <= k u sum |p|
    P64 = P.double()
    _within(c['psum'], P64.sum(1), k * U * P64.abs().sum(1), 'psum')
    # sums[:co]: the kernel adds a row's k edge values in fp32 (k - 1 additions, as psum: <= (k - 1) u sum_j |e|) and the
    # rows' partials in fp64 (kF64 of the total, inside the one u left over); e itself is the reference's e32, so it
    # carries no error.  sums[co:]: one more rounding per term for the product e e: <= (k + 1) u sum e^2.
    e64 = e32.double()
    s1, s2 = c['sums'][:co], c['sums'][co:]
    _within(s1, e64.sum((0, 1)), k * U * e64.abs().sum((0, 1)), 'sum e')
    _within(s2, e64.square().sum((0, 1)), (k + 1) * U * e64.square().sum((0, 1)), 'sum e^2')


# ---- 2. bn_lrelu_rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,C', [(1, 4), (37, 64), (5, 1024), (20000, 256)], ids=str)   # (20000, 256): > 4096 x 256 float4s,
def test_bn_lrelu_rows_elementwise_and_its_second_copy(R, C):                           # the grid-stride loop laps
    rng = np.random.default_rng([R, C, 2])
    e = _values(rng, R, C)
    scale, shift, _, _ = _bn_like(e, _gamma(C), _beta(C))
    out = run_bn_rows(e, scale, shift)
    # y32 = fl(fl(e scale) + shift): |y32 - y| <= u |e scale| + u (|e scale| + |shift|) <= 2 u S, S = |e scale| + |shift|.
    # LeakyReLU is 1-Lipschitz, so |lrelu(y32) - lrelu(y)| <= 2 u S on either side of the kink; the negative branch
    # multiplies by the fp32 constant 0.2f (0.6 u from 0.2) and rounds once more: 0.2 |y32| 1.6 u < u S.  Total 3 u S.
    es = torch.from_numpy(e).double() * torch.from_numpy(scale).double()
    sh = torch.from_numpy(shift).double()
    _within(out, F.leaky_relu(es + sh, 0.2), 3 * U * (es.abs() + sh.abs()), 'out')
    ld2, off = C + 12, 8
    wide = torch.from_numpy(rng.standard_normal((R, ld2)).astype(np.float32))
    out_b, after = run_bn_rows(e, scale, shift, wide, off)
    assert torch.equal(out_b.view(torch.int32), out.view(torch.int32))
    assert torch.equal(after[:, off:off + C].contiguous().view(torch.int32), out.view(torch.int32))
    assert torch.equal(after[:, :off], wide[:, :off]) and torch.equal(after[:, off + C:], wide[:, off + C:])


# ---- 3. bn_lrelu_backward_reduce ------------------------------------------------------------------------------------
def _check_bn_backward(e, scale, shift, mean, invstd, d32, g, sums):
    """g against the two slopes (the fp64 y decides, either is accepted inside the band), then sums against fp64 sums of
    the kernel's OWN g (so the in-band choices cancel).  -> the in-band share"""
    e64, sc, sh = torch.from_numpy(e).double(), torch.from_numpy(scale).double(), torch.from_numpy(shift).double()
    y = e64 * sc + sh
    band = y.abs() < BAND * ((e64 * sc).abs() + sh.abs())
    pos, neg = d32, d32 * 0.2                                   # fp32: fl(d 0.2f), the kernel's d * kSlope
    eq_pos = g.view(torch.int32) == pos.view(torch.int32)
    eq_neg = g.view(torch.int32) == neg.view(torch.int32)
    eq_pos |= (g == 0) & (pos == 0)                              # (0 + -0 = +0 in the kernel's d1 + d2)
    eq_neg |= (g == 0) & (neg == 0)
    ok = torch.where(band, eq_pos | eq_neg, torch.where(y > 0, eq_pos, eq_neg))
    assert ok.all(), int((~ok).sum())
    # sum g: fp32 values added in fp64: kF64 (beside it the bound's u sum |g| is idle).  sum g xhat: the kernel forms
    # fl(fl(fl(e - mean) invstd) g) in fp32 -- three roundings, 3 u |g xhat| per term -- and adds in fp64.
    g64 = g.double()
    xhat = (e64 - torch.from_numpy(mean).double()) * torch.from_numpy(invstd).double()
    C = e.shape[1]
    _within(sums[:C], g64.sum(0), (U + kF64) * g64.abs().sum(0), 'sum g')
    _within(sums[C:], (g64 * xhat).sum(0), (3 * U + kF64) * (g64 * xhat).abs().sum(0), 'sum g xhat')
    return band.double().mean().item()


@pytest.mark.parametrize('form', ['d1', 'd2', 'both'])
@pytest.mark.parametrize('R,C', [(1, 4), (2, 1024), (37, 16), (40000, 16), (700, 1024), (300, 512), (50, 2048)], ids=str)
def test_bn_lrelu_backward_reduce_slopes_sums_and_output_order(R, C, form):
    rng = np.random.default_rng([R, C, 3])
    e = _values(rng, R, C)
    scale, shift, mean, invstd = _bn_like(e, _gamma(C), _beta(C))
    d1 = torch.from_numpy(_values(rng, R, C)) if form != 'd2' else None
    wide, off = None, 0
    if form != 'd1':
        ld2, off = C + 12, 4
        wide = torch.full((R, ld2), float('nan'))                 # a read outside the d2 columns poisons g
        wide[:, off:off + C] = torch.from_numpy(_values(rng, R, C))
    d32 = d1 if wide is None else (wide[:, off:off + C].contiguous() if d1 is None else d1 + wide[:, off:off + C])
    g, sums, dgamma, dbeta = run_bn_backward(d1, wide, off, e, scale, shift, mean, invstd)
    share = _check_bn_backward(e, scale, shift, mean, invstd, d32, g, sums)
    print(f'in-band share {share:.2e}')
    assert share < 1e-4
    assert torch.equal(dbeta, sums[:C].float()) and torch.equal(dgamma, sums[C:].float())
    g2, sums2, _, _ = run_bn_backward(d1, wide, off, e, scale, shift, mean, invstd, with_param_grads=False)
    assert torch.equal(g2.view(torch.int32), g.view(torch.int32)) and torch.equal(sums2, sums)


@pytest.mark.parametrize('C', [12, 1536, 260])
def test_bn_lrelu_backward_reduce_refuses_widths_its_thread_layout_cannot_tile(C):
    """C / 4 must divide 256, or C be a multiple of 1024: argument checks, nothing is launched."""
    z = np.zeros((2, C), np.float32)
    v = np.zeros(C, np.float32)
    with pytest.raises(RuntimeError, match='bn_lrelu_backward_reduce'):
        run_bn_backward(z, None, 0, z, v, v, v, v)


# ---- 4. edge_backward in closed form (g is an input: no kink) --------------------------------------------------------
@pytest.mark.parametrize('case', EDGE_CASES, ids=str)
def test_edge_backward_equals_the_dense_edge_gradient(case):
    B, N, k, co, kind = case
    R = B * N
    c = _edge_case(case)
    rng = np.random.default_rng([B, N, k, co, 4])
    idx, pq = c['idx'], c['pq']
    flat = _flat(idx)
    P, e32 = _edges32(c, co)
    scale, _, mean, invstd = _bn_like(e32.numpy().reshape(R * k, co), c['gamma'], _beta(co))
    g = _values(rng, R, co)
    sums = rng.standard_normal(2 * co) * 0.3 * R * k                   # c1, c2 of the size of g: the corrections count
    start, src = run_reverse(idx)
    args = ((B, N, k, co), g, pq, c['sel'], c['psum'], start, src, scale, mean, invstd)
    dpq = run_edge_backward(*args, sums)

    sc, mu, inv = (torch.from_numpy(a).double() for a in (scale, mean, invstd))
    c1, c2 = torch.from_numpy(sums[:co] / (R * k)), torch.from_numpy(sums[co:] / (R * k))
    g64 = torch.from_numpy(g).double()
    P64, q64 = P.double(), torch.from_numpy(pq[:, co:]).double().unsqueeze(1)
    sel = torch.from_numpy(c['sel'].numpy().view(np.uint16).astype(np.int64))
    match = (torch.from_numpy(idx.reshape(R, k).astype(np.int64)).unsqueeze(2) == sel.unsqueeze(1)).double()
    assert (match.sum(1) == 1).all()
    dE = sc * (match * g64.unsqueeze(1) - c1 - (P64 + q64 - mu) * inv * c2)
    A = sc.abs() * (match * g64.abs().unsqueeze(1) + c1.abs() + (P64.abs() + q64.abs() + mu.abs()) * inv * c2.abs())
    scatter = lambda x: torch.zeros(R, co, dtype=torch.float64).index_add_(0, flat.reshape(-1), x.reshape(R * k, co))
    deg = torch.bincount(flat.reshape(-1), minlength=R).double().unsqueeze(1)
    # The standard forward bound m u A, m the most roundings any leaf term passes through.  dp[s] = scale (G - deg c1 -
    # c2i (deg (p - mean) + Q)), G and Q sums of deg terms over the arriving edges (deg - 1 additions): a q term is
    # rounded deg - 1 times in Q, then by "+ Q", c2i = fl(fl(c2) invstd) (2), the product, the subtraction and "scale x":
    # deg + 5; p and mean by "p - mean", "deg x", "+ Q" and the same five: 8; a g term deg - 1 in G and 3 after: deg + 2;
    # c1 by its conversion, "deg x", two subtractions and the scale: 5.  So m <= deg + 8.  dq[r] has the same shape with
    # k for deg and the forward kernel's psum (k - 1 roundings of its own) for Q: m <= k + 8.
    _within(dpq[:, :co], scatter(dE), (deg + 8) * U * scatter(A), 'dp')
    _within(dpq[:, co:], dE.sum(1), (k + 8) * U * A.sum(1), 'dq')
    isolated = deg[:, 0] == 0
    if kind == 'hub':                                                  # hubs with hundreds of arriving edges per cloud
        assert deg.max().item() >= N // 8                              # set; with k = 3 also points nobody lists
        assert k > 3 or isolated.sum().item() >= R // 16
    assert (dpq[:, :co][isolated] == 0).all()                          # no arriving edge: every term of dp is 0 x finite
    # eval mode (the product zeroes `sums`): dq = fl(scale g) exactly, dp = scale G with G a sum of deg terms
    dpq0 = run_edge_backward(*args, np.zeros(2 * co))
    assert torch.equal(dpq0[:, co:], torch.from_numpy(scale) * torch.from_numpy(g))
    G = scatter(match * g64.unsqueeze(1))
    _within(dpq0[:, :co], sc * G, deg * U * sc.abs() * scatter(match * g64.abs().unsqueeze(1)), 'dp (sums = 0)')
    assert (dpq0[:, :co][isolated] == 0).all()


# ---- 5. cloud_pool_stats / cloud_pool_backward -------------------------------------------------------------------------
POOL_CASES = [(1, 1024, 1024),      # rs = 16
              (3, 100, 256),        # rs = 2
              (1, 65, 260),         # rs = 2, per = 33; dead lanes; unit = 65
              (130, 70, 12),        # rs = 1; unit = 3
              (2, 3, 4),            # fewer rows than waves
              (1, 1, 1024),
              (2, 2048, 2048),      # R C / 4 = 8192 x 256 exactly: the backward's capped grid, one full lap and no more
              (2, 2049, 2048),      # R C / 4 > 8192 x 256: the backward sweep enters a second lap (unit = 2)
              (1, 33000, 260)]      # the same with unit = 65: a thread keeps its four channels over the laps only because
                                    # the grid (8255 blocks) is a multiple of C / 4 threads; dead lanes; per = 2063
POOL_SPLITS = {(1, 1024, 1024): 16, (3, 100, 256): 2, (1, 65, 260): 2, (130, 70, 12): 1, (2, 3, 4): 1, (1, 1, 1024): 1,
               (2, 2048, 2048): 16, (2, 2049, 2048): 16, (1, 33000, 260): 16}


def _pool_inputs(B, n, C, rs, rng):
    """y with exact ties: whole rows duplicated within a cloud at r, r + 1 (two waves), r, r + 4 (one wave) and across
    every range split, and in a third of the channels both copies set to the channel's extreme of the cloud, so that a
    tie IS the winner (its value stays inside the cloud's own range)"""
    y = _values(rng, B * n, C).reshape(B, n, C)
    gamma = _gamma(C)
    per = (n + rs - 1) // rs
    pairs = [(a, b) for a, b in ([(1, 2), (6, 10), (n - 2, n - 1)] + [(s * per - 1, s * per) for s in range(1, rs)])
             if 0 <= a < b < n]
    used = set()
    kept = []
    for a, b in pairs:
        if a in used or b in used:
            continue
        used |= {a, b}
        kept.append((a, b))
    for i, (a, b) in enumerate(kept):
        for bi in range(B):
            y[bi, b] = y[bi, a]
            ch = np.arange(i % 3, C, 3)
            ext = np.where(gamma[ch] >= 0, y[bi][:, ch].max(0), y[bi][:, ch].min(0))
            y[bi, a, ch] = y[bi, b, ch] = ext
    return y, gamma, kept


_pool_cache = {}


def _pool_case(case):
    if case not in _pool_cache:
        B, n, C = case
        rng = np.random.default_rng([B, n, C, 5])
        rs = pool_splits(B, n)
        y, gamma, pairs = _pool_inputs(B, n, C, rs, rng)
        ysel, arow, sums = run_pool_stats(y, gamma)
        _pool_cache[case] = dict(y=y, gamma=gamma, pairs=pairs, rs=rs, ysel=ysel, arow=arow, sums=sums)
    return _pool_cache[case]


@pytest.mark.parametrize('case', POOL_CASES, ids=str)
def test_cloud_pool_stats_first_occurrence_winners_and_fp64_sums(case):
    B, n, C = case
    c = _pool_case(case)
    assert c['rs'] == POOL_SPLITS[case]
    y, gamma = c['y'], c['gamma']
    for a, b in c['pairs']:
        assert np.array_equal(y[:, a], y[:, b])
    want = np.stack([_first_winner(y[bi][None], gamma)[0] for bi in range(B)])          # (B, C)
    if c['pairs']:
        firsts = np.array([a for a, _ in c['pairs']])
        assert (np.isin(want, firsts) & (gamma != 0)[None, :]).any(), 'no planted tie is a winner'
    assert np.array_equal(c['arow'].numpy().astype(np.int64), want)
    assert torch.equal(c['ysel'], torch.from_numpy(np.take_along_axis(y, want[:, None, :], 1)[:, 0]))
    # the kernel converts every value to fp64 before it adds or squares (the square of an fp32 number is exact in fp64)
    y64 = torch.from_numpy(y).double()
    _within(c['sums'][:C], y64.sum((0, 1)), kF64 * y64.abs().sum((0, 1)), 'sum y')
    _within(c['sums'][C:], y64.square().sum((0, 1)), kF64 * y64.square().sum((0, 1)), 'sum y^2')


@pytest.mark.parametrize('case', POOL_CASES, ids=str)
def test_cloud_pool_backward_equals_the_dense_gradient(case):
    B, n, C = case
    R = B * n
    c = _pool_case(case)
    rng = np.random.default_rng([B, n, C, 55])
    y = c['y']
    scale, _, mean, invstd = _bn_like(y.reshape(R, C), c['gamma'], _beta(C))
    g = _values(rng, B, C)
    sums = rng.standard_normal(2 * C) * 0.3 * R
    dy = run_pool_backward(y, g, c['arow'], scale, mean, invstd, sums)
    sc, mu, inv = (torch.from_numpy(a).double() for a in (scale, mean, invstd))
    c1, c2 = torch.from_numpy(sums[:C] / R), torch.from_numpy(sums[C:] / R)
    y64, g64 = torch.from_numpy(y).double(), torch.from_numpy(g).double().unsqueeze(1)
    match = (torch.arange(n).view(1, n, 1) == c['arow'].long().unsqueeze(1)).double()
    ref = sc * (match * g64 - c1 - (y64 - mu) * inv * c2)
    A = sc.abs() * (match * g64.abs() + c1.abs() + (y64.abs() + mu.abs()) * inv * c2.abs())
    # (every element is compared, so a thread whose channel offset went stale on a later lap of the grid-stride sweep --
    # the kernel forms it once, from its first element -- shows as wrong values in wrong columns)
    # roundings per leaf term of dy = scale ((g or 0) - c1 - fl(fl(y - mean) invstd) c2): y and mean pass "y - mean",
    # "x invstd", the conversion of c2, the product, the subtraction and "scale x": 6; c1 its conversion, two
    # subtractions and the scale: 4; g: 3.  8 u A covers them.
    _within(dy, ref, 8 * U * A, 'dy')


# ---- 6. the chain against autograd in fp64 ----------------------------------------------------------------------------
def _dense_layer(pq, flat, jstar, gamma, beta, t, co):
    """one EdgeConv layer from pq, dense over the edges: gather, add, batch statistics, affine, LeakyReLU, the edge at
    jstar, sum(out t) -- in the dtype and on the device of pq"""
    pq, gamma, beta = (x.clone().requires_grad_(True) for x in (pq, gamma, beta))
    e = pq[:, :co][flat] + pq[:, co:].unsqueeze(1)
    R, k, _ = e.shape
    mean, var = e.mean((0, 1)), e.var((0, 1), unbiased=False)
    scale = gamma * torch.rsqrt(var + EPS)
    shift = beta - mean * scale
    y = e * scale + shift
    out = F.leaky_relu(y, 0.2).gather(1, jstar.unsqueeze(1)).squeeze(1)
    (out * t).sum().backward()
    n = R * k
    res = dict(out=out.detach(), dx=pq.grad, dgamma=gamma.grad, dbeta=beta.grad, rmean=0.1 * mean.detach(),
               rvar=0.9 + 0.1 * var.detach() * n / max(n - 1, 1))
    ew = e.detach().gather(1, jstar.unsqueeze(1)).squeeze(1)
    return res, (ew, scale.detach(), shift.detach())


def _dense_pool(y, jstar, gamma, beta, t):
    """conv5's BatchNorm1d (training) + LeakyReLU + max over the cloud's points from y (B, n, C), the maximum taken at
    jstar, its first occurrence"""
    y, gamma, beta = (x.clone().requires_grad_(True) for x in (y, gamma, beta))
    B, n, C = y.shape
    z = F.leaky_relu(F.batch_norm(y.view(B * n, C), None, None, gamma, beta, True, 0.1, EPS), 0.2).view(B, n, C)
    out = z.gather(1, jstar.unsqueeze(1)).squeeze(1)
    live = gamma.detach() != 0
    assert torch.equal(out.detach()[:, live], z.detach().max(1)[0][:, live])
    (out * t).sum().backward()
    yd = y.detach()
    mean, var = yd.mean((0, 1)), yd.var((0, 1), unbiased=False)
    res = dict(out=out.detach(), dx=y.grad, dgamma=gamma.grad, dbeta=beta.grad, rmean=0.1 * mean,
               rvar=0.9 + 0.1 * var * (B * n) / max(B * n - 1, 1))
    scale = gamma.detach() * torch.rsqrt(var + EPS)
    return res, (yd.gather(1, jstar.unsqueeze(1)).squeeze(1), scale, beta.detach() - mean * scale)


def _usable(kink):
    """the fp64 reference alone decides: no winner within the band of LeakyReLU's kink"""
    ew, scale, shift = kink
    return bool(((ew * scale + shift).abs() >= BAND * ((ew * scale).abs() + shift.abs())).all())


def _compare_chain(tag, got, yard, ref):
    kinds = {'out': 'out', 'dx': 'dx', 'dgamma': 'dgamma', 'dbeta': 'dbeta', 'rmean': 'running', 'rvar': 'running'}
    errs = {name: (_err(got[name], ref[name]), _err(yard[name], ref[name])) for name in kinds}
    for name, (ek, ey) in errs.items():
        print(f'CHAIN {tag} {name}: kernels {ek:.3e}  fp32-pytorch {ey:.3e}')
    for name, (ek, _) in errs.items():
        assert ek <= CHAIN_TOL[kinds[name]], (name, ek, CHAIN_TOL[kinds[name]])


@pytest.mark.parametrize('case', [(3, 100, 20, 64, 'self'), (9, 40, 20, 128, 'hub'), (2, 77, 5, 16, 'hub'),
                                  (2, 30, 7, 512, 'noself')], ids=str)
def test_edgeconv_layer_chain_against_autograd_fp64(case):
    """edge_gather_stats -> bn_finalize -> bn_lrelu_rows -> bn_lrelu_backward_reduce -> knn_reverse -> edge_backward,
    against the dense layer in fp64 with pq as the leaf; tolerances from the fp32 PyTorch yardstick (module docstring)."""
    B, N, k, co, kind = case
    R = B * N
    gamma, beta = _gamma(co), _beta(co)
    for seed in range(8):
        rng = np.random.default_rng([B, N, k, co, 6, seed])
        idx = _graph(kind, B, N, k, rng)
        pq = _values(rng, R, 2 * co)
        t = _values(rng, R, co)
        flat = _flat(idx)
        e32 = (torch.from_numpy(pq)[:, :co][flat] + torch.from_numpy(pq)[:, co:].unsqueeze(1)).numpy()
        jstar = torch.from_numpy(_first_winner(e32, gamma))
        ref, kink = _dense_layer(torch.from_numpy(pq).double(), flat, jstar, torch.from_numpy(gamma).double(),
                                 torch.from_numpy(beta).double(), torch.from_numpy(t).double(), co)
        if _usable(kink):
            break
    else:
        pytest.fail('no seed out of 8 keeps every winner clear of the kink')
    yard, _ = _dense_layer(_up(pq), flat.to(DEV), jstar.to(DEV), _up(gamma), _up(beta), _up(t), co)
    esel, sel, psum, sums = run_gather(pq, idx, gamma, co)
    scale, shift, mean, invstd, rmean, rvar = run_finalize(gamma, beta, R * k, sums)
    out = run_bn_rows(esel, scale, shift)
    g, sums_b, dgamma, dbeta = run_bn_backward(torch.from_numpy(t), None, 0, esel, scale, shift, mean, invstd)
    start, src = run_reverse(idx)
    dpq = run_edge_backward((B, N, k, co), g, pq, sel, psum, start, src, scale, mean, invstd, sums_b)
    got = dict(out=out, dx=dpq, dgamma=dgamma, dbeta=dbeta, rmean=rmean, rvar=rvar)
    _compare_chain(f'layer {case} seed {seed}', got, yard, ref)


@pytest.mark.parametrize('case', [(3, 100, 256), (1, 1024, 64), (1, 65, 256)], ids=str)
def test_cloud_pool_chain_against_autograd_fp64(case):
    """cloud_pool_stats -> bn_finalize -> bn_lrelu_rows -> bn_lrelu_backward_reduce -> cloud_pool_backward against
    BatchNorm1d + LeakyReLU + max over the points in fp64.  (1, 65, 256) keeps rs = 2 and per = 33 of a 65-point cloud at
    a width bn_lrelu_backward_reduce accepts: it refuses C = 260 (65 threads per row do not tile a block of 256; pinned
    by test_bn_lrelu_backward_reduce_refuses_...), so the chain cannot be composed there.  C = 260 runs in section 5."""
    B, n, C = case
    R = B * n
    gamma, beta = _gamma(C), _beta(C)
    for seed in range(8):
        rng = np.random.default_rng([B, n, C, 66, seed])
        y = _values(rng, R, C).reshape(B, n, C)
        t = _values(rng, B, C)
        jstar = torch.from_numpy(np.stack([_first_winner(y[bi][None], gamma)[0] for bi in range(B)]))
        ref, kink = _dense_pool(torch.from_numpy(y).double(), jstar, torch.from_numpy(gamma).double(),
                                torch.from_numpy(beta).double(), torch.from_numpy(t).double())
        if _usable(kink):
            break
    else:
        pytest.fail('no seed out of 8 keeps every winner clear of the kink')
    yard, _ = _dense_pool(_up(y), jstar.to(DEV), _up(gamma), _up(beta), _up(t))
    ysel, arow, sums = run_pool_stats(y, gamma)
    scale, shift, mean, invstd, rmean, rvar = run_finalize(gamma, beta, R, sums)
    out = run_bn_rows(ysel, scale, shift)
    g, sums_b, dgamma, dbeta = run_bn_backward(torch.from_numpy(t), None, 0, ysel, scale, shift, mean, invstd)
    dy = run_pool_backward(y, g, arow, scale, mean, invstd, sums_b)
    got = dict(out=out, dx=dy, dgamma=dgamma, dbeta=dbeta, rmean=rmean, rvar=rvar)
    _compare_chain(f'pool {case} seed {seed}', got, yard, ref)


# ---- 7. the small kernels, bit for bit -----------------------------------------------------------------------------
WEIGHT_SHAPES = [(64, 3, 4), (64, 64, 64), (256, 128, 128), (16, 5, 8)]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('jobs', [1, 4, 8])
def test_edge_weight_stack_and_unstack_single_and_multi(jobs):
    rng = np.random.default_rng([jobs, 7])
    shapes = [WEIGHT_SHAPES[(i + jobs) % 4] for i in range(jobs)]
    cos, cins, kps = ([s[i] for s in shapes] for i in range(3))
    ws_in = [torch.from_numpy(rng.standard_normal((co, 2 * cin)).astype(np.float32)) for co, cin, kp in shapes]
    single = run_weights('pdae_edge_weight_stack', cos, cins, kps, ws_in, multi=False)
    multi = run_weights('pdae_edge_weight_stack', cos, cins, kps, ws_in, multi=True)
    for (co, cin, kp), w, a, b in zip(shapes, ws_in, single, multi):
        want = F.pad(torch.cat([w[:, :cin], w[:, cin:] - w[:, :cin]]), (0, kp - cin))      # [W1; W2 - W1], K padded
        assert _same_bits(a, want) and _same_bits(b, a)
    dws_in = [torch.from_numpy(rng.standard_normal((2 * co, kp)).astype(np.float32)) for co, cin, kp in shapes]
    single = run_weights('pdae_edge_weight_unstack', cos, cins, kps, dws_in, multi=False)
    multi = run_weights('pdae_edge_weight_unstack', cos, cins, kps, dws_in, multi=True)
    for (co, cin, kp), d, a, b in zip(shapes, dws_in, single, multi):
        top, bottom = d[:co, :cin], d[co:, :cin]
        assert _same_bits(a, torch.cat([top - bottom, bottom], dim=1)) and _same_bits(b, a)


@pytest.mark.parametrize('R,c,cp', [(1, 3, 4), (1000, 3, 4), (37, 5, 8), (10, 4, 4)])
def test_rows_pad_equals_f_pad(R, c, cp):
    x = torch.from_numpy(np.random.default_rng([R, c, cp]).standard_normal((R, c)).astype(np.float32))
    assert _same_bits(run_rows_pad(x, cp), F.pad(x, (0, cp - c)))
