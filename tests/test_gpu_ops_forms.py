"""Every size-dispatched form of the sampling / grouping / interpolation kernels, bit for bit against the CPU oracle.

csrc/fps.hip, knn.hip, ball_group.hip and interpolate.hip choose a kernel form from the sizes of the call: a template
instantiation, a points-per-lane count, queries or centres per wave, an LDS copy or global re-reads, an LDS accumulator
or global atomics.  tests/test_gpu_ops.py picks its shapes by workload; this module picks them by DISPATCH: one case on
both sides of every threshold, the refusals at every limit, and inputs built so that what differs between two forms
(padding lanes, the last register slot, the tie rank once `cols` changes, state carried from one query of a wave to the
next) decides the answer.

Every comparison is `assert_array_equal`: there is no tolerance in this module.  Scatter-add gradients, whose summation
order is unspecified, are made exact by construction: the incoming gradient is integer-valued in [-4, 4] (and the
interpolation weights are multiples of 1/4), so every partial sum is an integer (or a multiple of 1/16) far below 2^24
and fp32 adds it without rounding in any order.  tests/test_ops_forms_cpu.py shows that condition on the CPU, and checks
the ladders restated below against the text of the kernels' sources, so a retuned heuristic fails there instead of
quietly moving a case off its edge.  Each case also asserts the form its id names.
"""
import math

import numpy as np
import pytest
import torch

from conftest import make_clouds

pytestmark = pytest.mark.gpu

KIB = 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ====================================================================== host formulas, restated ======================
# csrc/fps.hip pdae_furthest_point_sampling, the `n <= K` ladder :162-171: K -> (threads T, points per lane P);
# above the last K the form is FPS_ABOVE, above FPS_MAX_N the entry refuses (:154)
FPS_LADDER = [(64, (64, 1)), (128, (64, 2)), (256, (128, 2)), (512, (256, 2)), (1024, (256, 4)), (2048, (512, 4)),
              (4096, (1024, 4)), (8192, (1024, 8)), (16384, (512, 32))]
FPS_ABOVE = (1024, 32)
FPS_MAX_N = 32768
FPS_LDS_BYTES = 96 * KIB            # launch_fps :139-140: the cloud is copied to LDS while 12 n bytes fit

# csrc/knn.hip pdae_knn :173-181: K -> points per lane of knn_kernel<PPL>; above the last K knn_stream_kernel
KNN_LADDER = [(64, 1), (128, 2), (256, 4), (512, 8), (1024, 16), (2048, 32)]
KNN_MAX_K = 64
KNN_QPW_WAVES = 2048                # :167-168
BALL_CPW_WAVES = 4096               # csrc/ball_group.hip pdae_ball_query :244-245
BALL_LDS_BYTES = 150 * KIB          # :236-237 (12 n bytes): n <= 12800
GROUP_GRAD_LDS_BYTES = 128 * KIB    # pdae_group_points_grad :285 (4 n bytes): n <= 32768, global atomics above
TNN_TILE = 1024                     # csrc/interpolate.hip :20
INTERP_GRAD_LDS_BYTES = 160 * KIB   # pdae_three_interpolate_grad :140 (4 m bytes): m <= 40960
SA_GRAD_MAX_N, SA_GRAD_MAX_C = 4096, 1024      # pdae_sa_group_rows_grad :331, :342
SA_GRAD_LDS_BYTES = 150 * KIB       # :341-342: 4 (2 N + 1 + np ns) bytes
MAX_GRID_Y = 65535                  # clouds ride on gridDim.y


def fps_form(n):
    for edge, form in FPS_LADDER:
        if n <= edge:
            return form
    return FPS_ABOVE


def fps_uses_lds(n):
    return n * 3 * 4 <= FPS_LDS_BYTES


def ref_block_size(n):
    """csrc/fps.hip ref_block_size :128-134 (cuda_utils.h opt_n_threads): it decides the reference's tie order."""
    return max(1, min(512, 1 << int(math.log(float(n)) / math.log(2.0))))


def knn_form(n):
    for edge, ppl in KNN_LADDER:
        if n <= edge:
            return ppl
    return 'stream'


def knn_qpw(b, g):
    qpw = 8
    while qpw > 1 and b * -(-g // qpw) < KNN_QPW_WAVES:
        qpw >>= 1
    return qpw


def ball_cpw(b, m):
    cpw = 8
    while cpw > 1 and b * -(-m // cpw) < BALL_CPW_WAVES:
        cpw >>= 1
    return cpw


def group_grad_form(n):
    return 'lds' if n * 4 <= GROUP_GRAD_LDS_BYTES else 'atomic'


def sa_grad_lanes(C):
    """sa_group_rows_grad_kernel :205: lanes per row, rows in flight per block."""
    lpr = C // 4
    return lpr, 256 // lpr


def sa_grad_lds_bytes(N, rows):
    return 4 * (2 * N + 1 + rows)


def _edges(ladder):
    return sorted({k for k, _ in ladder} | {k + 1 for k, _ in ladder})


# ====================================================================== FPS ==========================================
# threshold            what changes across it
# 64 .. 16384 (+1)     the instantiation <T, P>: waves per block (1 wave: no LDS slot exchange), register slots per lane,
#                      how many lanes / slots are padding
# 8192 / 8193          LDS copy of the cloud -> global re-read of the last sample
# 512 / 513 and up     the reference's block is 512 wide: `cols` grows, the tie rank rev * cols + column changes
# 32768 / 32769        the last accepted n (16-bit index and rank fields of the key) / refusal
FPS_NS = _edges(FPS_LADDER) + [FPS_MAX_N]
FPS_FORMS = {64: (64, 1), 65: (64, 2), 128: (64, 2), 129: (128, 2), 256: (128, 2), 257: (256, 2), 512: (256, 2),
             513: (256, 4), 1024: (256, 4), 1025: (512, 4), 2048: (512, 4), 2049: (1024, 4), 4096: (1024, 4),
             4097: (1024, 8), 8192: (1024, 8), 8193: (512, 32), 16384: (512, 32), 16385: (1024, 32),
             32768: (1024, 32)}
FPS_FAR, FPS_PLATEAU = -8.0, 4.0


def _bitrev(t, bits):
    return int(format(t, '0{}b'.format(bits))[::-1], 2) if bits else 0


def fps_tie_rank(k, bs):
    """Order in which the reference's block settles equal distances (tests/test_oracle.py _tie_rank)."""
    return (_bitrev(k % bs, bs.bit_length() - 1), k // bs)


def fps_built_cloud(n, variant, seed):
    """One cloud that separates the forms.  Both variants carry a PLATEAU of identical points spread over several
    columns of the reference's block layout, far enough out to be the third sample, so the bit-reversed tie rank decides
    it; the winner is neither the smallest index nor the smallest thread.
      'far_last'   the farthest point of all sits at index n - 1: the last register slot, next to the padding
      'skip_last'  the last L indices (n - 1 included) lie in the origin ball |p|^2 <= 1e-3 and are never sampled; the
                   farthest point is the last index before them
    -> (cloud (n,3), index of the farthest point, plateau indices)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    p[(p * p).sum(1) < 0.05] += np.float32(0.5)          # only the planted run is inside the origin ball
    bs = ref_block_size(n)
    bits, cols = bs.bit_length() - 1, -(-n // bs)
    L = max(2, min(n // 8, 40))
    free_end = n - L - 1                                 # everything planted below stays under this index

    def at(rev, col):
        return _bitrev(rev, bits) + col * bs

    def last_col(rev):
        col = cols - 1
        while at(rev, col) >= free_end:
            col -= 1
        return col
    # (rev 1, last column) must beat (rev 2, column 0): rank rev * cols + column with a wrong `cols` gets that wrong
    plateau = {at(1, last_col(1)), at(2, 0), at(3, 0), at(5, 0), at(2, last_col(2)), at(3, last_col(3))}
    plateau.discard(0)
    plateau = sorted(plateau)
    p[plateau] = FPS_PLATEAU
    if variant == 'far_last':
        far = n - 1
    else:
        far = free_end
        p[n - L:] = rng.uniform(-0.01, 0.01, (L, 3)).astype(np.float32)
    p[far] = FPS_FAR
    return p, far, plateau


def _fps_case(oracle_ops, n, m, variant):
    from point_dae_amd import pointnet2_utils as pu
    x = make_clouds(1000 + n, 2, n, 'uniform')
    x[1], far, plateau = fps_built_cloud(n, variant, 2000 + n)
    want_idx, want_ctr = oracle_ops.furthest_point_sample(x, m, return_centres=True)
    # the built cloud does what it was built for (this is a check of the test's inputs and of the oracle)
    bs = ref_block_size(n)
    assert bs == oracle_ops.opt_n_threads(n)
    if m >= 3:
        winner = min(plateau, key=lambda k: fps_tie_rank(k, bs))
        assert want_idx[1, 1] == far and want_idx[1, 2] == winner and winner != min(plateau)
    if variant == 'skip_last':
        assert not (want_idx[1] > far).any()
    xd = dev(x)
    got = pu.furthest_point_sample(xd, m)                                     # without the fused centres
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(host(got), want_idx)
    idx2, ctr = pu.furthest_point_sample_with_centres(xd, m)                  # with them
    np.testing.assert_array_equal(host(idx2), want_idx)
    np.testing.assert_array_equal(host(ctr), want_ctr)


@pytest.mark.parametrize('variant', ['far_last', 'skip_last'])
@pytest.mark.parametrize('n', FPS_NS, ids=lambda n: 'n{}-T{}xP{}-{}'.format(n, *FPS_FORMS[n], 'lds' if n <= 8192 else 'global'))
def test_fps_every_form(oracle_ops, n, variant):
    assert fps_form(n) == FPS_FORMS[n]
    assert fps_uses_lds(n) == (n <= 8192)
    t, p = fps_form(n)
    assert t * p >= n                                     # the registers hold the cloud
    _fps_case(oracle_ops, n, 12, variant)


@pytest.mark.parametrize('m', [1, 65])
def test_fps_one_sample_and_every_point(oracle_ops, m):
    """m = 1 (no iteration at all) and m = n = 65: once every valid point is taken all distances are 0 and the tie
    rank alone orders the rest; the origin-ball run is never taken."""
    assert fps_form(65) == (64, 2)
    _fps_case(oracle_ops, 65, m, 'skip_last')


def test_fps_refuses_past_its_limit():
    from point_dae_amd import pointnet2_utils as pu
    x = torch.zeros(2, FPS_MAX_N + 1, 3, device='cuda')
    with pytest.raises(RuntimeError, match='not implemented'):
        pu.furthest_point_sample(x, 12)
    with pytest.raises(RuntimeError, match='not implemented'):
        pu.furthest_point_sample_with_centres(x, 12)


# ====================================================================== kNN ==========================================
# threshold                      what changes across it
# 64 .. 2048 (+1)                points per lane of the register form; 2049: the streaming form (global re-reads)
# b * ceil(g / qpw) >= 2048      queries per wave 1 / 2 / 4 / 8: the selection state and the staging ring are reused by
#                                the consecutive queries of a wave; g % (4 qpw) != 0 leaves a ragged last wave and block
# k = 64 / 65, b = 65535 / 65536 the last accepted size / refusal
KNN_NS = _edges(KNN_LADDER)
KNN_FORMS = {64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8, 513: 16, 1024: 16, 1025: 32, 2048: 32,
             2049: 'stream'}


def _knn_check(oracle_ops, x, q, k):
    from point_dae_amd.knn_cuda import knn
    wd, wi, wn = oracle_ops.knn(x, q, k, return_nbr=True)
    d, i, nb = knn(dev(x), dev(q), k, with_neighbourhood=True)
    assert i.dtype == torch.int64
    np.testing.assert_array_equal(host(i), wi)
    np.testing.assert_array_equal(host(d), wd)
    np.testing.assert_array_equal(host(nb), wn)


@pytest.mark.parametrize('kmax', [False, True], ids=['k1', 'kmax'])
@pytest.mark.parametrize('n', KNN_NS, ids=lambda n: 'n{}-ppl{}'.format(n, KNN_FORMS[n]))
def test_knn_every_form(oracle_ops, n, kmax):
    B, g = 2, 7
    k = min(n, KNN_MAX_K) if kmax else 1
    assert knn_form(n) == KNN_FORMS[n] and knn_qpw(B, g) == 1
    if KNN_FORMS[n] != 'stream':
        assert 64 * KNN_FORMS[n] >= n
    x = make_clouds(3000 + n, B, n)
    x[1, n - 3] = x[1, 2]                       # a tie between the first and the last register slots
    q = x[:, :g].copy()
    q[:, 1] += np.float32(0.013)                # queries that are not cloud points
    q[:, 4] = [3.0, -3.0, 3.0]
    q[:, 5] = x[:, n - 1]                       # the last point (padding's neighbour) is the nearest one
    _knn_check(oracle_ops, x, q, k)


@pytest.mark.parametrize('b,g,qpw,n', [(64, 250, 8, 65), (16, 509, 4, 65), (8, 513, 2, 65), (8, 513, 2, 2049)],
                         ids=['qpw8-n65', 'qpw4-n65', 'qpw2-n65', 'qpw2-stream'])
def test_knn_queries_per_wave(oracle_ops, b, g, qpw, n):
    k = 20
    assert knn_qpw(b, g) == qpw and g % (4 * qpw) != 0
    assert knn_form(n) == (2 if n == 65 else 'stream')
    x = make_clouds(3100 + b, b, n)
    x[1, 10:50] = x[1, 10]                      # a block of duplicates: queries near it stage far more candidates
    rng = np.random.default_rng(3200 + b)
    q = rng.uniform(-1, 1, (b, g, 3)).astype(np.float32)
    q[:, ::3] = x[:, np.arange(0, g, 3) % n]    # members of the cloud among the queries
    q[1, 1::2] = x[1, 10] + rng.uniform(-1e-3, 1e-3, (len(range(1, g, 2)), 3)).astype(np.float32)
    q[1, 5::8] = x[1, 10]                       # consecutive queries of a wave: on the block, near it, far from it
    _knn_check(oracle_ops, x, q, k)


def test_knn_refuses_past_its_limits():
    from point_dae_amd.knn_cuda import knn
    x = torch.rand(2, 70, 3, device='cuda')
    with pytest.raises(RuntimeError, match='k > 64 not implemented'):
        knn(x, x[:, :4].contiguous(), KNN_MAX_K + 1)
    many = torch.zeros(MAX_GRID_Y + 1, 1, 3, device='cuda')
    with pytest.raises(RuntimeError, match='b > 65535'):
        knn(many, many, 1)


# ====================================================================== ball query ===================================
# threshold                      what changes across it
# n = 1, 63, 64, 65              one partial step of 64 candidates, one full step, a second (partial) step
# n = 5461 / 5462                the SoA copy of the cloud passes 64 KiB of dynamic LDS
# n = 12800 / 12801              the last accepted cloud (150 KiB) / refusal
# b * ceil(m / cpw) >= 4096      centres per wave 1 / 2 / 4 / 8: cnt / first are per-centre state of one wave
BALL_NS = [1, 63, 64, 65, 5461, 5462, 12800]
BALL_RADIUS = 0.3


def ball_inputs(b, n, m, seed):
    """Cloud 1 has a tight cluster on its first indices and a lone point at index n - 1.  Centre 0 of every cloud has an
    empty ball, centre 1 of cloud 1 sits on the cluster (more hits than a small nsample inside the first 64 candidates),
    centre 2 on the lone last point (one hit: fewer than nsample, padded with it)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (b, n, 3)).astype(np.float32)
    nc = min(40, n - 1)
    a = np.float32([0.2, -0.3, 0.4])
    x[1, :nc] = a + rng.uniform(-0.01, 0.01, (nc, 3)).astype(np.float32)
    x[1, n - 1] = [3.0, 3.0, 3.0]
    c = x[:, rng.integers(0, n, m)].copy()
    c += rng.uniform(-0.05, 0.05, c.shape).astype(np.float32)
    c[:, 0] = [5.0, 5.0, 5.0]
    if m > 2:
        c[1, 1] = a
        c[1, 2] = [3.0, 3.0, 3.05]
    return x, c


def _ball_hits(x, c, r):
    d = c[:, None, :] - x[None, :, :]
    d2 = (d * d).astype(np.float32)
    return ((d2[..., 0] + d2[..., 1]) + d2[..., 2]) < np.float32(r) * np.float32(r)


@pytest.mark.parametrize('ns', [1, 16, 100])
@pytest.mark.parametrize('n', BALL_NS)
def test_ball_query_every_size(oracle_ops, n, ns):
    from point_dae_amd import pointnet2_utils as pu
    B, m = 2, 9
    assert ball_cpw(B, m) == 1 and n * 12 <= BALL_LDS_BYTES
    assert (5461 * 12 <= 64 * KIB < 5462 * 12) and 12800 * 12 == BALL_LDS_BYTES
    x, c = ball_inputs(B, n, m, 4000 + n)
    hits = _ball_hits(x[1], c[1], BALL_RADIUS)
    count = hits.sum(1)
    assert count[0] == 0                                              # an empty ball
    if ns > 1:
        assert ((count > 0) & (count < ns)).any()                     # a short one
    if n >= 64 and ns < 40:
        assert (hits[:, :64].sum(1) > ns).any()                       # more than nsample within the first step
    want = oracle_ops.ball_query(BALL_RADIUS, ns, x, c)
    got = pu.ball_query(BALL_RADIUS, ns, dev(x), dev(c))
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(host(got), want)


@pytest.mark.parametrize('b,m,cpw', [(64, 515, 8), (32, 509, 4), (16, 513, 2)], ids=['cpw8', 'cpw4', 'cpw2'])
def test_ball_query_centres_per_wave(oracle_ops, b, m, cpw):
    from point_dae_amd import pointnet2_utils as pu
    n, ns = 70, 16
    assert ball_cpw(b, m) == cpw and m % (4 * cpw) != 0
    x, c = ball_inputs(b, n, m, 4100 + b)
    c[1, 3::4] = [5.0, 5.0, 5.0]               # empty, crowded and ordinary balls alternate inside one wave
    c[1, 4::4] = x[1, 0]
    want = oracle_ops.ball_query(BALL_RADIUS, ns, x, c)
    np.testing.assert_array_equal(host(pu.ball_query(BALL_RADIUS, ns, dev(x), dev(c))), want)


def test_ball_query_limits_and_empty_cloud():
    from point_dae_amd import pointnet2_utils as pu
    c = torch.zeros(2, 9, 3, device='cuda')
    with pytest.raises(RuntimeError, match='n > 12800 not implemented'):
        pu.ball_query(0.3, 16, torch.zeros(2, 12801, 3, device='cuda'), c)
    many = torch.zeros(MAX_GRID_Y + 1, 1, 3, device='cuda')
    with pytest.raises(RuntimeError, match='b > 65535'):
        pu.ball_query(0.3, 1, many, many)
    got = pu.ball_query(0.3, 16, torch.zeros(2, 0, 3, device='cuda'), c)      # no points: every ball is empty
    assert got.shape == (2, 9, 16) and not host(got).any()


# ====================================================================== group / gather ===============================
# threshold            what changes across it
# n = 32768 / 32769    the gradient's accumulator: 128 KiB of LDS (the largest the LDS form takes) / zero-fill + global
#                      atomics
# np * ns % 4          the forward's 16-byte path (128 = 32 x 4) / its scalar tail (165 = 33 x 5)
GROUP_NS = [32768, 32769]
GROUP_SHAPES = [(32, 4), (33, 5)]
GROUP_INDEX_KINDS = ['random', 'one_point', 'both_ends']


def group_inputs(n, npnt, ns, kind, seed, B=2, C=3):
    """-> features (B,C,n) f32, idx (B,npnt,ns) i32, grad_out (B,C,npnt,ns) f32 with integer values in [-4, 4]."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(B, C, n)).astype(np.float32)
    if kind == 'random':
        idx = rng.integers(0, n, (B, npnt, ns))
    elif kind == 'one_point':                   # every gradient lands on one slot
        idx = np.full((B, npnt, ns), n // 3)
        idx[1] = n - 1
    else:                                       # the first and the last slot of the accumulator, many times each
        idx = rng.choice(np.array([0, n - 1, n // 2, 255, 256]), (B, npnt, ns))
        idx[:, 0, 0], idx[:, -1, -1] = 0, n - 1
    go = rng.integers(-4, 5, (B, C, npnt, ns)).astype(np.float32)
    return f, idx.astype(np.int32), go


def scatter_int64(go, idx, n):
    """The scatter-add of an integer-valued gradient in int64: go (B,C,T) onto idx (B,T) -> (B,C,n)."""
    B, C, T = go.shape
    out = np.zeros((B, C, n), np.int64)
    g = go.astype(np.int64)
    assert np.array_equal(g, go)
    for b in range(B):
        for c in range(C):
            np.add.at(out[b, c], idx[b], g[b, c])
    return out


@pytest.mark.parametrize('kind', GROUP_INDEX_KINDS)
@pytest.mark.parametrize('npnt,ns', GROUP_SHAPES, ids=['int4', 'tail'])
@pytest.mark.parametrize('n', GROUP_NS, ids=['n32768-lds', 'n32769-atomic'])
def test_group_points_every_form(oracle_ops, n, npnt, ns, kind):
    from point_dae_amd import pointnet2_utils as pu
    assert group_grad_form(n) == ('lds' if n == 32768 else 'atomic')
    assert ((npnt * ns) % 4 == 0) == ((npnt, ns) == (32, 4))
    f, idx, go = group_inputs(n, npnt, ns, kind, 5000 + n + ns)
    fd = dev(f).requires_grad_(True)
    out = pu.grouping_operation(fd, dev(idx))
    np.testing.assert_array_equal(host(out), oracle_ops.grouping_operation(f, idx))
    out.backward(dev(go))
    got = host(fd.grad)
    np.testing.assert_array_equal(got, oracle_ops.grouping_operation_grad(go, idx, n))
    np.testing.assert_array_equal(got, scatter_int64(go.reshape(2, 3, -1), idx.reshape(2, -1), n))


@pytest.mark.parametrize('kind', GROUP_INDEX_KINDS)
@pytest.mark.parametrize('npnt', [32, 33], ids=['int4', 'tail'])
@pytest.mark.parametrize('n', GROUP_NS, ids=['n32768-lds', 'n32769-atomic'])
def test_gather_every_form(oracle_ops, n, npnt, kind):
    from point_dae_amd import pointnet2_utils as pu
    assert group_grad_form(n) == ('lds' if n == 32768 else 'atomic')
    f, idx, go = group_inputs(n, npnt, 1, kind, 5100 + n + npnt)
    idx, go = idx[:, :, 0].copy(), go[:, :, :, 0].copy()
    fd = dev(f).requires_grad_(True)
    out = pu.gather_operation(fd, dev(idx))
    np.testing.assert_array_equal(host(out), oracle_ops.gather_operation(f, idx))
    out.backward(dev(go))
    got = host(fd.grad)
    np.testing.assert_array_equal(got, oracle_ops.gather_operation_grad(go, idx, n))
    np.testing.assert_array_equal(got, scatter_int64(go, idx, n))


# ====================================================================== three_nn / three_interpolate =================
# threshold                what changes across it
# m = 1, 2, 3              fewer known points than neighbours: the unused slots stay (+inf, 0)
# m = 1023 / 1024 / 1025   the 1024-point LDS tile of three_nn: one partial tile, one full, a second; 2049: a third
# n = 1, 255, 257          one partial block of unknown points, two blocks with one point in the second
# m = 16384 / 16385        the gradient's accumulator passes 64 KiB of dynamic LDS
# m = 40960 / 40961        the last accepted m (160 KiB: all of a CU's LDS) / refusal
TNN_MS = [1, 2, 3, 1023, 1024, 1025, 2049]
TNN_NS = [1, 255, 257]
INTERP_MS = [3, 16384, 16385, 40960]


@pytest.mark.parametrize('n', TNN_NS)
@pytest.mark.parametrize('m', TNN_MS)
def test_three_nn_every_tile_count(oracle_ops, m, n):
    from point_dae_amd import pointnet2_utils as pu
    B = 2
    assert -(-m // TNN_TILE) == {1: 1, 2: 1, 3: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3}[m]
    rng = np.random.default_rng(6000 + m + n)
    unknown = rng.uniform(-1, 1, (B, n, 3)).astype(np.float32)
    known = rng.uniform(-1, 1, (B, m, 3)).astype(np.float32)
    if m >= 2:
        known[:, m - 1] = known[:, 0]           # a duplicate per cloud: first against last index (across the tiles)
        unknown[:, 0] = known[:, 0]             # ... and an unknown point on it: distance 0 twice
    if m >= 8:
        known[0, 7] = known[0, 3]
    unknown[:, n - 1] = known[:, m // 2] + np.float32(1e-3)
    dist, idx = pu.three_nn(dev(unknown), dev(known))
    d2, widx = oracle_ops.three_nn(unknown, known)
    assert idx.dtype == torch.int32
    np.testing.assert_array_equal(host(idx), widx)
    np.testing.assert_array_equal(host(dist), np.sqrt(d2))


def interp_inputs(m, kind, seed, B=2, c=2, n=300):
    """-> points (B,c,m) f32, idx (B,n,3) i32, weight (B,n,3): permutations of (1/2, 1/4, 1/4), grad_out (B,c,n) with
    integer values in [-4, 4]: every product grad * weight is a multiple of 1/4, every sum of them exact in fp32."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(B, c, m)).astype(np.float32)
    if kind == 'random':
        idx = rng.integers(0, m, (B, n, 3))
        idx[:, 0], idx[:, 1] = [0, m - 1, m // 2], [m - 1, m - 1, 0]
    else:                                       # every neighbour of every point is the same known point
        idx = np.full((B, n, 3), m - 1)
        idx[1] = m // 2
    w = np.float32([0.5, 0.25, 0.25])[rng.permuted(np.tile(np.arange(3), (B, n, 1)), axis=2)]
    g = rng.integers(-4, 5, (B, c, n)).astype(np.float32)
    return pts, idx.astype(np.int32), w, g


def interp_grad_int64(g, idx, w, m):
    """three_interpolate's gradient in int64 on the 4 x scaled weights, back to fp32 (exact: multiples of 1/4)."""
    B, c, n = g.shape
    w4 = (w * 4).astype(np.int64)
    assert np.array_equal(w4, w * 4) and np.array_equal(g.astype(np.int64), g)
    out = np.zeros((B, c, m), np.int64)
    for b in range(B):
        for l in range(c):
            np.add.at(out[b, l], idx[b].reshape(-1), (g[b, l].astype(np.int64)[:, None] * w4[b]).reshape(-1))
    res = (out / 4.0).astype(np.float32)
    assert np.array_equal(res.astype(np.float64) * 4, out)
    return res


@pytest.mark.parametrize('kind', ['random', 'one_point'])
@pytest.mark.parametrize('m', INTERP_MS)
def test_three_interpolate_every_size(oracle_ops, m, kind):
    from point_dae_amd import pointnet2_utils as pu
    assert m * 4 <= INTERP_GRAD_LDS_BYTES and (16384 * 4 <= 64 * KIB < 16385 * 4)
    assert 40960 * 4 == INTERP_GRAD_LDS_BYTES
    pts, idx, w, g = interp_inputs(m, kind, 6100 + m)
    f = dev(pts).requires_grad_(True)
    out = pu.three_interpolate(f, dev(idx), dev(w))
    np.testing.assert_array_equal(host(out), oracle_ops.three_interpolate(pts, idx, w))
    out.backward(dev(g))
    got = host(f.grad)
    np.testing.assert_array_equal(got, oracle_ops.three_interpolate_grad(g, idx, w, m))
    np.testing.assert_array_equal(got, interp_grad_int64(g, idx, w, m))


def test_three_interpolate_grad_refuses_past_its_limit():
    from point_dae_amd import _lib
    B, c, n, m = 1, 1, 4, 40961
    g = torch.zeros(B, c, n, device='cuda')
    idx = torch.zeros(B, n, 3, device='cuda', dtype=torch.int32)
    w = torch.zeros(B, n, 3, device='cuda')
    out = torch.zeros(B, c, m, device='cuda')
    with pytest.raises(RuntimeError, match='more than 40960 known points'):
        _lib.call('pdae_three_interpolate_grad', g, B, c, n, m, _lib.ptr(g), _lib.ptr(idx), _lib.ptr(w), _lib.ptr(out))


# ====================================================================== sa_group_rows / _grad ========================
# threshold                        what changes across it
# N = 4096 / 4097                  the one-wave prefix sum takes N / 64 = 64 entries per lane at the limit / refusal
# C = 1024 / 1028                  C / 4 = 256 lanes per row: one row in flight, the lane group is the whole block / refusal
# C = 12                           3 lanes per row, 85 rows in flight, the block's last lane idle
# 4 (2 N + 1 + np ns) = 150 KiB    the counting sort's LDS exactly at its limit / one more row: refusal
SA_CASES = [(2, 4096, 64, 32, 1024), (2, 4096, 7, 5, 12), (1, 64, 38271, 1, 4)]
SA_LANES = {1024: (256, 1), 12: (3, 85), 4: (1, 256)}


@pytest.mark.parametrize('B,N,npoint,ns,C', SA_CASES, ids=['N4096-C1024', 'N4096-C12', 'rows-at-150KiB'])
def test_sa_group_rows_at_its_limits(B, N, npoint, ns, C):
    """Against the index_select form it replaces (tests/test_gpu_sa.py); dout is integer-valued in [-4, 4], so the feature
    gradient is bit-equal in any summation order, index_add's atomics included."""
    from point_dae_amd.point_cae_pointnetv2 import _GroupRows
    assert N <= SA_GRAD_MAX_N and C <= SA_GRAD_MAX_C and sa_grad_lanes(C) == SA_LANES[C]
    assert sa_grad_lds_bytes(N, npoint * ns) <= SA_GRAD_LDS_BYTES
    if npoint == 38271:
        assert sa_grad_lds_bytes(N, npoint * ns) == SA_GRAD_LDS_BYTES
    g = torch.Generator(device='cuda').manual_seed(B * N + C)
    xyz = torch.rand(B, N, 3, device='cuda', generator=g)
    new_xyz = torch.rand(B, npoint, 3, device='cuda', generator=g)
    idx = torch.randint(0, N, (B, npoint, ns), device='cuda', generator=g, dtype=torch.int32)
    idx[:, :, ns // 2:] = idx[:, :, :1]                                  # duplicates inside a ball
    idx[0, 0] = 0                                                        # an empty ball: all zeros
    idx[0, 1, 0], idx[0, -1, -1] = N - 1, N - 1                          # the last point of the cloud
    feats = torch.randn(B * N, C, device='cuda', generator=g, requires_grad=True)
    out = _GroupRows.apply(xyz, new_xyz, idx, feats)
    flat = (idx.long() + torch.arange(B, device='cuda').view(B, 1, 1) * N).reshape(-1)
    ref_f = feats.detach().clone().requires_grad_(True)
    gx = (xyz.reshape(B * N, 3).index_select(0, flat).reshape(B, npoint, ns, 3) - new_xyz.unsqueeze(2)).reshape(-1, 3)
    ref = torch.cat([gx, gx.new_zeros(gx.shape[0], 1), ref_f.index_select(0, flat)], dim=1)
    assert out.shape == ref.shape and torch.equal(out, ref)
    w = torch.randint(-4, 5, out.shape, device='cuda', generator=g).float()
    out.backward(w)
    ref.backward(w)
    assert torch.equal(feats.grad, ref_f.grad)
    # ... and the int64 scatter of the same integers
    want = torch.zeros(B * N, C, device='cuda', dtype=torch.int64).index_add_(0, flat, w[:, 4:].long())
    assert torch.equal(feats.grad.long(), want) and torch.equal(feats.grad, want.float())


@pytest.mark.parametrize('B,N,npoint,ns,C,msg', [(1, 4097, 1, 1, 4, 'do not fit LDS'), (1, 64, 1, 1, 1028, 'at most 1024'),
                                                 (1, 64, 38272, 1, 4, 'do not fit LDS')],
                         ids=['N4097', 'C1028', 'one-row-too-many'])
def test_sa_group_rows_grad_refuses_past_its_limits(B, N, npoint, ns, C, msg):
    from point_dae_amd import _lib
    assert N > SA_GRAD_MAX_N or C > SA_GRAD_MAX_C or sa_grad_lds_bytes(N, npoint * ns) == SA_GRAD_LDS_BYTES + 4
    idx = torch.zeros(B, npoint, ns, device='cuda', dtype=torch.int32)
    dout = torch.zeros(B * npoint * ns, 4 + C, device='cuda')
    dfeat = torch.zeros(B * N, C, device='cuda')
    with pytest.raises(RuntimeError, match=msg):
        _lib.call('pdae_sa_group_rows_grad', dout, B, N, npoint, ns, C, _lib.ptr(idx), _lib.ptr(dout), _lib.ptr(dfeat))
