"""The Transformer pretraining step's small kernels one by one against fp64: pdae_patch_affine (csrc/corrupt.hip),
pdae_drop_path_keep and pdae_pos_embed_fc1 (csrc/block.hip), pdae_mean_sum2 and pdae_chamfer_backward_mean on every
backward path, and the Chamfer forward's chamfer_fwd_tiled<4> and chamfer_fwd_many kernels on exact ties and ragged last
tiles (csrc/chamfer.hip).  The whole-model tests reach these kernels only through full-step losses and gradients at
relative tolerances; here they are called through point_dae_amd._lib with the wrappers' argument lists, and through the
wrappers, and every output ELEMENT is held bit for bit or to a forward error bound derived where it is used.

Conventions (those of tests/test_gpu_dgcnn_kernels.py): output buffers are NaN-filled and nothing may keep its NaN;
u = 2^-24 (the library is built with -ffp-contract=off, so every fp32 operation rounds once); a leaf term that passes
m roundings carries a relative error of at most gamma(m) = m u / (1 - m u), and "A" is the reference expression with
every leaf replaced by its absolute value.  Inputs are the fp32 numbers the kernels read, so the fp64 references start
from exactly the same values.  The references are plain functions (ref_*); tests/test_pretrain_kernel_refs_cpu.py runs
them against the CPU oracle on a machine without a GPU.

Section 3 has two outputs without a derived bound: h = GELU(z) and gp = GELU'(z) go through the device erff / expf, whose
accuracy the project states nowhere, and pos_embed as a whole (fc1 kernel -> row GEMM -> the two weight-gradient GEMMs)
through the row-GEMM family.  Their yardstick is the same computation in fp32 PyTorch on the GPU against the fp64
reference, measured in the same test with test_gpu_block.py's measure max |err| / max |ref|; the tolerance is 4 x the
largest yardstick error recorded on an MI355X per output kind (two bits for a different, equally legitimate evaluation
order).  Recorded figures, largest over the cases of each test (the kernels' own column in both GEMM arithmetics):

    pdae_pos_embed_fc1   fp32 PyTorch (yardstick)     kernel          tolerance (4 x yardstick)
    h                    1.519e-7                     1.519e-7        6.076e-7
    gp                   1.965e-7                     1.965e-7        7.860e-7

    nn_ops.pos_embed     fp32 PyTorch (yardstick)     kernels         tolerance (4 x yardstick)
    y                    4.279e-7                     2.375e-7        1.712e-6
    dW1                  4.996e-7                     3.024e-7        1.998e-6
    db1                  3.554e-7                     2.504e-7        1.422e-6
    dW2                  4.119e-7                     1.877e-7        1.648e-6
    db2                  1.126e-7                     1.173e-7        4.504e-7
"""
import math
import random
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import make_clouds

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = 'cuda'
FC1_YARDSTICK = {'h': 1.519e-7, 'gp': 1.965e-7}                                                           # the tables above
POS_YARDSTICK = {'y': 4.279e-7, 'dW1': 4.996e-7, 'db1': 3.554e-7, 'dW2': 4.119e-7, 'db2': 1.126e-7}
FC1_TOL = {kind: 4 * y for kind, y in FC1_YARDSTICK.items()}
POS_TOL = {kind: 4 * y for kind, y in POS_YARDSTICK.items()}


def gamma(m):
    """(1 + u)^m - 1 <= m u / (1 - m u): the relative error of a term that passed m fp32 roundings"""
    return m * U / (1.0 - m * U)


def _L():
    from point_dae_amd import _lib
    return _lib


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


def _up(a):
    return _t(a).to(DEV).contiguous()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def _written(*tensors):
    for t in tensors:
        assert torch.isfinite(t).all(), 'an output buffer kept its NaN fill'


def _within(got, ref, bound, what):
    err = (_t(got).detach().double().cpu() - ref).abs()
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err[bad] / bound[bad].clamp_min(1e-300)).max()))


def _err(a, ref):
    """tests/test_gpu_block.py _close's measure: max |a - ref| / max |ref|."""
    return (a.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item() / (ref.abs().max().item() + 1e-12)


# ===================================================================================================================
# 1. pdae_patch_affine
# ===================================================================================================================
def ref_steps_to_rows(steps, B):
    """oracle.model's step list [('mul', (B, 3)) | ('mat', (B, 3, 3))] -> the kernel's (nsteps, B, 10) fp32 rows
    [kind, then the 3 factors or the 9 matrix entries row-major]"""
    rows = torch.zeros(len(steps), B, 10)
    for s, (kind, p) in enumerate(steps):
        if kind == 'mul':
            rows[s, :, 1:4] = p
        else:
            rows[s, :, 0] = 1.0
            rows[s, :, 1:] = p.reshape(B, 9)
    return rows


def ref_rows_to_steps(rows):
    """the inverse: what corrupt_util_tensor.draw_corruption returns -> oracle.model's step list"""
    return [('mul', r[:, 1:4].clone()) if (r[:, 0] == 0).all() else ('mat', r[:, 1:].reshape(-1, 3, 3).clone()) for r in rows]


def ref_patch_affine(nbr, center, steps):
    """fp64: oracle.model.apply_corruption on neighborhood + center and on center -> gt_nbr, t_nbr, t_center as
    PointCAE_transformer.forward leaves them (gt = (nbr + c) - c, t_nbr = P - T, t_center = T)"""
    from oracle.model import apply_corruption
    c = center.double()
    absolute = nbr.double() + c.unsqueeze(2)
    P, T = apply_corruption(absolute, c, [(k, p.double()) for k, p in steps])
    return absolute - c.unsqueeze(2), P - T.unsqueeze(2), T


def ref_patch_affine_magnitudes(a_abs, c_abs, steps):
    """A of the transformed point and centre: apply_corruption with every leaf (coordinates, factors, matrix entries)
    replaced by its absolute value -> (A_P, A_T, cost); cost = the roundings the steps add to a leaf: a multiply step
    one (the product), a matrix step three (out_j = (v_0 R_0j + v_1 R_1j) + v_2 R_2j: the product and two additions for
    the first two terms, the product and one addition for the third)"""
    from oracle.model import apply_corruption
    AP, AT = apply_corruption(a_abs, c_abs, [(k, p.double().abs()) for k, p in steps])
    return AP, AT, sum(1 if k == 'mul' else 3 for k, _ in steps)


def run_patch_affine(nbr, center, rows):
    """rows: (nsteps, B, 10) or None (a null `steps` pointer, nsteps 0) -> gt_nbr, t_nbr, t_center"""
    L = _L()
    B, G, K, _ = nbr.shape
    nd, cd = _up(nbr), _up(center)
    st = _up(rows) if rows is not None else None
    gt, tn, tc = _nan((B, G, K, 3)), _nan((B, G, K, 3)), _nan((B, G, 3))
    L.call('pdae_patch_affine', nd, B, G, K, 0 if rows is None else rows.shape[0], nd.data_ptr(), cd.data_ptr(), L.ptr(st),
           gt.data_ptr(), tn.data_ptr(), tc.data_ptr())
    _written(gt, tn, tc)
    return gt.cpu(), tn.cpu(), tc.cpu()


def _patches(B, G, K, seed):
    """centre-subtracted patches of radius ~0.2 around centres in [-1, 1]^3, as Group.forward makes them"""
    rng = np.random.default_rng([B, G, K, seed])
    center = torch.from_numpy(rng.uniform(-1, 1, (B, G, 3)).astype(np.float32))
    nbr = torch.from_numpy((0.2 * rng.standard_normal((B, G, K, 3))).astype(np.float32))
    return nbr, center, rng


def _random_steps(seq, B, rng):
    """a different map for every sample: factors of either sign in +-[0.5, 2], dense normal matrices"""
    steps = []
    for kind in seq:
        if kind == 'mul':
            p = rng.uniform(0.5, 2.0, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3))
        else:
            p = rng.standard_normal((B, 3, 3))
        steps.append((kind, torch.from_numpy(p.astype(np.float32))))
    return steps


AFFINE_SHAPES = [(3, 5, 7),        # 105 points: one partial block
                 (2, 64, 32),      # 16 full blocks
                 (1, 1, 1),
                 (5, 3, 33)]       # group and sample boundaries inside blocks
AFFINE_SEQS = [(), ('mul',), ('mat',), ('mul', 'mat'), ('mat', 'mul'), ('mul', 'mat', 'mul'), ('mat', 'mul', 'mat')]


@pytest.mark.parametrize('seq', AFFINE_SEQS, ids=lambda s: '-'.join(s) or 'none')
@pytest.mark.parametrize('shape', AFFINE_SHAPES, ids=str)
def test_patch_affine_against_apply_corruption_fp64(shape, seq):
    B, G, K = shape
    nbr, center, rng = _patches(B, G, K, len(seq))
    steps = _random_steps(seq, B, rng)
    gt, tn, tc = run_patch_affine(nbr, center, ref_steps_to_rows(steps, B) if steps else None)
    want_gt, want_tn, want_tc = ref_patch_affine(nbr, center, steps)
    # gt = fl(fl(nbr + c) - c): two fp32 operations, each rounded once -- the same two in torch on the host
    assert torch.equal(gt, (nbr + center.unsqueeze(2)) - center.unsqueeze(2))
    _within(gt, want_gt, gamma(2) * (nbr.double().abs() + 2 * center.double().abs().unsqueeze(2)), 'gt_nbr')
    # the point a = fl(nbr + c) starts with one rounding, the centre with none; the steps add `cost` to both; the final
    # fl(p - t) one more to both: a leaf of p passes 1 + cost + 1 roundings, a leaf of t cost + 1 -- gamma(cost + 2)
    # covers both -- and t_center = t itself `cost`
    AP, AT, cost = ref_patch_affine_magnitudes(nbr.double().abs() + center.double().abs().unsqueeze(2),
                                               center.double().abs(), steps)
    _within(tn, want_tn, gamma(cost + 2) * (AP + AT.unsqueeze(2)), 't_nbr')
    _within(tc, want_tc, gamma(cost) * AT, 't_center')
    if not steps:      # nsteps == 0 with a null `steps` pointer: nothing is applied
        assert torch.equal(tn, gt) and torch.equal(tc, center)


@pytest.mark.parametrize('shape', AFFINE_SHAPES, ids=str)
def test_patch_affine_exact_maps_bit_for_bit(shape):
    B, G, K = shape
    nbr, center, rng = _patches(B, G, K, 11)
    gt, tn0, tc0 = run_patch_affine(nbr, center, None)
    assert torch.equal(tn0, gt) and torch.equal(tc0, center)
    eye = ('mat', torch.eye(3).repeat(B, 1, 1))
    ones = ('mul', torch.ones(B, 3))
    for steps in ([eye], [ones], [ones, eye, ones], [eye, ones, eye]):       # v 1 + v' 0 + v'' 0 = v and v 1 = v, exactly
        _, tn, tc = run_patch_affine(nbr, center, ref_steps_to_rows(steps, B))
        assert torch.equal(tn, gt) and torch.equal(tc, center)
    # a permutation matrix per sample (a different one for neighbouring samples): out_j = v_perm[j] exactly, so the
    # transformed patch is the permuted ground truth fl(a - c) and the transformed centre the permuted centre
    perms = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]]
    perm = torch.tensor([perms[(b + 1) % 6] for b in range(B)])
    Pm = torch.zeros(B, 3, 3)
    for b in range(B):
        for j in range(3):
            Pm[b, perm[b, j], j] = 1.0
    _, tn, tc = run_patch_affine(nbr, center, ref_steps_to_rows([('mat', Pm)], B))
    assert torch.equal(tn, torch.gather(gt, 3, perm.view(B, 1, 1, 3).expand(B, G, K, 3)))
    assert torch.equal(tc, torch.gather(center, 2, perm.view(B, 1, 3).expand(B, G, 3)))
    # t_center is written by the group's first point from the centre alone: it does not depend on K
    steps = _random_steps(('mat', 'mul', 'mat'), B, rng)
    rows = ref_steps_to_rows(steps, B)
    _, _, tc_k = run_patch_affine(nbr, center, rows)
    for K2 in (1, K + 3):
        nbr2 = torch.from_numpy((0.2 * rng.standard_normal((B, G, K2, 3))).astype(np.float32))
        assert torch.equal(run_patch_affine(nbr2, center, rows)[2], tc_k)


@pytest.mark.parametrize('kinds', [['clean'], ['affine_r3']], ids=lambda k: k[0])
def test_corrupt_data_wrapper_against_apply_corruption_fp64(kinds):
    from oracle.model import apply_corruption
    from point_dae_amd import corrupt_util_tensor as cut
    B, G, K = 5, 3, 33
    seen = set()
    for seed in range(8 if kinds == ['affine_r3'] else 1):
        nbr, center, _ = _patches(B, G, K, 100 + seed)
        absolute = nbr + center.unsqueeze(2)                       # the fp32 absolute patches the wrapper is given
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        t_abs, t_c = cut.corrupt_data(_up(absolute), _up(center), kinds)
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        steps = ref_rows_to_steps(cut.draw_corruption(kinds, B))   # the same host draws once more
        seen.add(len(steps))
        _written(t_abs, t_c)
        P, T = apply_corruption(absolute.double(), center.double(), [(k, p.double()) for k, p in steps])
        # the wrapper forms rel = fl(abs - c), the kernel a = fl(rel + c): abs and the first c pass 2 roundings, the
        # second c one, so A_a = |abs| + 2 |c| with m = 2; then the steps (cost), fl(p - t) and the wrapper's
        # fl(t_nbr + t_c): cost + 4 on a leaf of p, at most cost + 2 on the two t, and T counted twice in A
        AP, AT, cost = ref_patch_affine_magnitudes(absolute.double().abs() + 2 * center.double().abs().unsqueeze(2),
                                                   center.double().abs(), steps)
        _within(t_abs, P, gamma(cost + 4) * (AP + 2 * AT.unsqueeze(2)), 'transformed patches')
        _within(t_c, T, gamma(cost) * AT, 'transformed centres')
    assert seen == ({0} if kinds == ['clean'] else {1, 2, 3})     # eight seeds draw every step count of affine_r3


def test_patch_affine_refusals_and_empty_sizes():
    L = _L()
    nbr, center, rng = _patches(2, 3, 4, 12)
    nd, cd, st = _up(nbr), _up(center), _up(ref_steps_to_rows(_random_steps(('mul',), 2, rng), 2))
    gt, tn, tc = _nan((2, 3, 4, 3)), _nan((2, 3, 4, 3)), _nan((2, 3, 3))
    out = (gt.data_ptr(), tn.data_ptr(), tc.data_ptr())
    for size in ((2, 3, 0, 1), (-1, 3, 4, 1), (2, -1, 4, 1), (2, 3, 4, -1)):
        with pytest.raises(RuntimeError, match='patch_affine: bad size'):
            L.call('pdae_patch_affine', nd, *size, nd.data_ptr(), cd.data_ptr(), st.data_ptr(), *out)
    with pytest.raises(RuntimeError, match='patch_affine: null pointer'):
        L.call('pdae_patch_affine', nd, 2, 3, 4, 1, nd.data_ptr(), cd.data_ptr(), None, *out)
    for size in ((0, 3, 4, 1), (2, 0, 4, 1)):                                    # nothing to do: nothing is written
        L.call('pdae_patch_affine', nd, *size, nd.data_ptr(), cd.data_ptr(), st.data_ptr(), *out)
    torch.cuda.synchronize()
    assert torch.isnan(gt).all() and torch.isnan(tn).all() and torch.isnan(tc).all()


# ===================================================================================================================
# 2. pdae_drop_path_keep
# ===================================================================================================================
def ref_drop_path_keep(r, keep):
    """timm 0.4.5 drop_path's factor floor(keep + rand) / keep, in fp32 on the host: r (S, B), keep (S,) or (S, 1).
    The operation is fp32 by definition (one addition, one division, both correctly rounded on either side)."""
    k = keep.reshape(-1, 1).float().cpu()
    return torch.floor(r.float().cpu() + k) / k


def _keeps(S):
    """S distinct keep probabilities in (0, 1], the first exactly 1"""
    return torch.from_numpy((1.0 - 0.9 * np.arange(S) / S).astype(np.float32))


def _planted_draws(S, B, keep, rng):
    """uniform draws (S, B) x as many matrices as it takes to plant in EVERY row: 0, 1 - 2^-24 (the largest draw),
    fl(1 - keep) and its fp32 neighbours on both sides (the lower one clamped to 0: draws are in [0, 1))"""
    edge = (np.float32(1.0) - keep.numpy()).astype(np.float32)
    plants = [np.zeros(S, np.float32), np.full(S, 1.0 - 2.0 ** -24, np.float32), edge,
              np.maximum(np.nextafter(edge, np.float32(-1.0)), np.float32(0.0)), np.nextafter(edge, np.float32(2.0))]
    mats = []
    for q in range((len(plants) + B - 1) // B):
        r = rng.random((S, B), dtype=np.float32)
        for p in range(q * B, min((q + 1) * B, len(plants))):
            r[:, p % B] = plants[p]
        mats.append(torch.from_numpy(r))
    return mats


@pytest.mark.parametrize('S,B', [(1, 1), (2, 3), (32, 128), (48, 37)], ids=str)
def test_drop_path_keep_bit_for_bit_out_of_place_and_in_place(S, B):
    L = _L()
    keep = _keeps(S)
    kd = _up(keep.reshape(S, 1))
    n, pad = S * B, 64
    for r in _planted_draws(S, B, keep, np.random.default_rng([S, B, 2])):
        # (keep < 1: every factor is 0 or fl(1 / keep).  keep = 1, the first row: the largest draw gives
        # fl(1 - 2^-24 + 1) = 2 and the factor 2 -- on both sides; the wrappers hand out no row with keep = 1)
        want = ref_drop_path_keep(r, keep)
        factors = torch.cat([torch.zeros(S, 1), (1.0 / keep).reshape(S, 1)], 1)
        assert ((want.unsqueeze(2) == factors.unsqueeze(1)).any(2))[1:].all()
        rd = _up(r)
        out = _nan((n + pad,))
        L.call('pdae_drop_path_keep', rd, S, B, rd.data_ptr(), kd.data_ptr(), out.data_ptr())
        assert torch.equal(out[:n].cpu().view(S, B), want) and torch.equal(rd.cpu(), r)
        assert torch.isnan(out[n:]).all()                         # nothing beyond the n elements is written
        buf = _nan((n + pad,))
        buf[:n] = rd.reshape(-1)
        L.call('pdae_drop_path_keep', buf, S, B, buf.data_ptr(), kd.data_ptr(), buf.data_ptr())          # out == r
        assert torch.equal(buf[:n].cpu().view(S, B), want) and torch.isnan(buf[n:]).all()


def test_draw_drop_path_wrapper_rows_of_one_draw():
    from point_dae_amd import nn_ops
    probs = [0.0, 0.05, 0.1, 0.0, 0.25]
    B, depth = 37, len(probs)
    keep = nn_ops.drop_path_keep_buffer(probs).to(DEV)
    for seed in (0, 7):
        torch.manual_seed(seed)
        got = nn_ops.draw_drop_path(B, probs, True, keep)
        torch.manual_seed(seed)
        r = torch.rand((2 * depth, B), dtype=torch.float32, device=DEV)
        want = ref_drop_path_keep(r, keep)
        assert torch.equal(torch.floor(r + keep) / keep, want.to(DEV))       # fp32 torch on the device: the same two operations
        for i, p in enumerate(probs):
            if p == 0.0:
                assert got[i] == (None, None)
                continue
            assert torch.equal(got[i][0].cpu(), want[2 * i]) and torch.equal(got[i][1].cpu(), want[2 * i + 1])
            inv = (1.0 / keep[2 * i]).item()
            assert all(((f == 0) | (f == inv)).all() for f in got[i])          # every factor is 0 or fl(1 / keep)
    assert nn_ops.draw_drop_path(B, probs, False, keep) == [(None, None)] * depth
    assert nn_ops.draw_drop_path(B, [0.0] * 3, True, nn_ops.drop_path_keep_buffer([0.0] * 3).to(DEV)) == [(None, None)] * 3


def test_predraw_drop_path_hands_each_stack_its_rows_of_one_draw(monkeypatch):
    from point_dae_amd import nn_ops
    monkeypatch.setattr(nn_ops, 'PREDRAW', True)

    def stack(probs):
        return types.SimpleNamespace(blocks=[types.SimpleNamespace(drop_prob=p) for p in probs], training=True,
                                     dp_keep=nn_ops.drop_path_keep_buffer(probs).to(DEV))
    enc, dec = stack([0.0, 0.04, 0.08, 0.12]), stack([0.3, 0.0])
    B = 23
    torch.manual_seed(3)
    nn_ops.predraw_drop_path(B, [enc, dec])
    torch.manual_seed(3)
    keep = torch.cat([enc.dp_keep, dec.dp_keep], 0)
    want = ref_drop_path_keep(torch.rand((keep.shape[0], B), dtype=torch.float32, device=DEV), keep)
    state = torch.cuda.get_rng_state()
    o = 0
    for s in (enc, dec):
        got = nn_ops.stack_keeps(s, B)
        for i, blk in enumerate(s.blocks):
            if blk.drop_prob == 0.0:
                assert got[i] == (None, None)
            else:
                assert torch.equal(got[i][0].cpu(), want[o + 2 * i]) and torch.equal(got[i][1].cpu(), want[o + 2 * i + 1])
                inv = (1.0 / s.dp_keep[2 * i]).item()
                assert all(((f == 0) | (f == inv)).all() for f in got[i])
        o += s.dp_keep.shape[0]
    assert torch.equal(torch.cuda.get_rng_state(), state)        # the stacks drew nothing of their own
    assert '_keeps_next' not in enc.__dict__ and '_keeps_next' not in dec.__dict__


# ===================================================================================================================
# 3. pdae_pos_embed_fc1 and nn_ops.pos_embed
# ===================================================================================================================
def ref_gelu(z):
    """GELU(z) = z Phi(z) and GELU'(z) = Phi(z) + z phi(z) in the dtype of z"""
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return z * cdf, cdf + z * pdf


def ref_pos_fc1(x, w1, b1):
    """fp64 first layer on the gathered rows x (M, 3): z, h = GELU(z), gp = GELU'(z), and A_z = |x| |W1|^T + |b1|"""
    x, w1, b1 = x.double(), w1.double(), b1.double()
    z = x @ w1.T + b1
    h, gp = ref_gelu(z)
    return z, h, gp, x.abs() @ w1.abs().T + b1.abs()


def ref_pos_embed_module(w1, b1, w2, b2):
    """Linear(3, H) -> GELU -> Linear(H, C) in fp64 on the host with the given parameters (copies, requiring grad)"""
    H, C = w1.shape[0], w2.shape[0]
    seq = nn.Sequential(nn.Linear(3, H), nn.GELU(), nn.Linear(H, C)).double()
    with torch.no_grad():
        for p, v in zip(seq.parameters(), (w1, b1, w2, b2)):
            p.copy_(v.detach().double().cpu())
    return seq


def _gather_rows(M, R, rng):
    """int64 row ids into an xyz of R > M rows: they repeat, are out of order and skip most of xyz; the last row of
    xyz is among them"""
    rows = rng.integers(0, R, M)
    rows[0] = R - 1
    if M > 2:
        rows[-1] = rows[1]                      # a repeat ...
        rows[2] = 0                             # ... and a descent, whatever was drawn
    return torch.from_numpy(rows.astype(np.int64))


def run_pos_fc1(xyz, rows, w1, b1):
    """-> h, gp (M, H), xp (M, 4)"""
    L = _L()
    M = rows.numel() if rows is not None else xyz.shape[0]
    H = w1.shape[0]
    xd, rd, wd, bd = _up(xyz), (_up(rows) if rows is not None else None), _up(w1), _up(b1)
    h, gp, xp = _nan((M, H)), _nan((M, H)), _nan((M, 4))
    L.call('pdae_pos_embed_fc1', xd, M, H, xd.data_ptr(), L.ptr(rd), wd.data_ptr(), bd.data_ptr(), h.data_ptr(),
           gp.data_ptr(), xp.data_ptr())
    _written(h, gp, xp)
    return h.cpu(), gp.cpu(), xp.cpu()


def _fc1_inputs(M, H, gathered, wscale):
    rng = np.random.default_rng([M, H, int(gathered), wscale])
    R = 4 * M + 7 if gathered else M
    xyz = torch.from_numpy(rng.uniform(-1, 1, (R, 3)).astype(np.float32))       # FPS centres live in [-1, 1]^3
    rows = _gather_rows(M, R, rng) if gathered else None
    torch.manual_seed(M * 1000 + H)
    lin = nn.Linear(3, H)                                                        # nn.Linear's default initialisation
    return xyz, rows, (lin.weight.detach() * wscale).contiguous(), (lin.bias.detach() * wscale).contiguous()


@pytest.mark.parametrize('M,H,gathered,wscale', [(1, 4, False, 1), (1, 4, True, 1), (5, 8, False, 1), (5, 8, True, 1),
                                                 (300, 128, False, 1), (300, 128, True, 1), (64, 128, False, 1),
                                                 (64, 128, True, 1),
                                                 (300, 128, True, 4)], ids=str)     # weights x 4: z reaches about +-6
def test_pos_embed_fc1_gather_z_gelu_and_its_derivative(M, H, gathered, wscale):
    xyz, rows, w1, b1 = _fc1_inputs(M, H, gathered, wscale)
    x = xyz[rows] if gathered else xyz
    h, gp, xp = run_pos_fc1(xyz, rows, w1, b1)
    assert torch.equal(xp, torch.cat([x, torch.zeros(M, 1)], 1))          # the gathered row and a zero fourth column
    z, want_h, want_gp, Az = ref_pos_fc1(x, w1, b1)
    if wscale > 1:
        assert z.abs().max().item() > 5.0
    # z itself is not an output.  It is read off a second launch with the bias raised by 12 wscale: |x . w| <= sqrt(3)
    # and |b| <= 1 / sqrt(3) at the default initialisation, |z| <= 2.31 wscale, so every z' lies above 9.69 wscale, and
    # for z' > 8: erf(z' / sqrt 2) > 1 - 1e-15, erff returns 1.0f, cdf = 0.5 (1 + 1) = 1 and h' = z' 1 = z' exactly.
    # z' = fma(x2, w2, fma(x1, w1, fl(x0 w0))) + b': the first product passes 4 roundings (its own, two fma, the bias
    # addition), the second 3, the third 2, the bias 1: gamma(4) A_z covers them
    lift = 12.0 * wscale
    b_hi = b1 + lift
    z_hi, _, _, Az_hi = ref_pos_fc1(x, w1, b_hi)
    assert z_hi.min().item() > 8.0
    h_hi, _, _ = run_pos_fc1(xyz, rows, w1, b_hi)
    _within(h_hi, z_hi, gamma(4) * Az_hi, "z (read as h at z > 8, where GELU is the identity in fp32)")
    # h and gp: the yardstick rule of the module docstring
    zy = F.linear(_up(x), _up(w1), _up(b1)).requires_grad_(True)
    hy = F.gelu(zy)
    gpy, = torch.autograd.grad(hy.sum(), zy)
    for kind, got, yard, want in (('h', h, hy, want_h), ('gp', gp, gpy, want_gp)):
        print(f'FC1 ({M}, {H}, {gathered}, {wscale}) {kind}: kernel {_err(got, want):.3e}  fp32-pytorch {_err(yard, want):.3e}')
    for kind, got, want in (('h', h, want_h), ('gp', gp, want_gp)):
        assert _err(got, want) <= FC1_TOL[kind], (kind, _err(got, want), FC1_TOL[kind])


def test_pos_embed_fc1_refusals():
    xyz, rows, w1, b1 = _fc1_inputs(5, 8, True, 1)
    for H in (6, 0):
        with pytest.raises(RuntimeError, match='pos_embed_fc1: M >= 0, H a positive multiple of 4 required'):
            run_pos_fc1(xyz, rows, torch.zeros(H, 3), torch.zeros(max(H, 1)))
    L = _L()
    xd = _up(xyz)
    with pytest.raises(RuntimeError, match='pos_embed_fc1: null pointer'):
        L.call('pdae_pos_embed_fc1', xd, 5, 8, xd.data_ptr(), None, None, None, None, None, None)


POS_CASES = [(300, 128, 384, True), (23, 128, 384, False), (7, 8, 16, True)]


@pytest.mark.parametrize('arith', ['f32mfma', 'bf16x3'])
@pytest.mark.parametrize('case', POS_CASES, ids=str)
def test_pos_embed_against_the_fp64_module_in_both_gemm_arithmetics(case, arith):
    from point_dae_amd import _lib, nn_ops
    M, H, C, gathered = case
    rng = np.random.default_rng([M, H, C, 3])
    R = 4 * M + 7 if gathered else M
    xyz = torch.from_numpy(rng.uniform(-1, 1, (R, 3)).astype(np.float32))
    rows = _gather_rows(M, R, rng) if gathered else None
    t = torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32))
    torch.manual_seed(M + H + C)
    seq = nn.Sequential(nn.Linear(3, H), nn.GELU(), nn.Linear(H, C)).to(DEV)
    params = [p.detach().clone() for p in seq.parameters()]
    x = xyz[rows] if gathered else xyz

    def grads(module, y, t_):
        (y * t_).sum().backward()
        w1, b1, w2, b2 = module.parameters()
        return dict(y=y.detach(), dW1=w1.grad, db1=b1.grad, dW2=w2.grad, db2=b2.grad)
    ref_seq = ref_pos_embed_module(*params)
    ref = grads(ref_seq, ref_seq(x.double()), t.double())
    yard_seq = ref_pos_embed_module(*params).float().to(DEV)
    yard = grads(yard_seq, yard_seq(_up(x)), _up(t))
    xyz_d = _up(xyz).requires_grad_(True)
    before = _lib.gemm_arith()
    _lib.set_gemm_arith(_lib.GEMM_F32MFMA if arith == 'f32mfma' else _lib.GEMM_BF16X3)
    try:
        got = grads(seq, nn_ops.pos_embed(xyz_d, seq, _up(rows) if gathered else None), _up(t))
        torch.cuda.synchronize()
    finally:
        _lib.set_gemm_arith(before)
    assert got['dW1'].shape == (H, 3) and got['dW1'].is_contiguous()
    assert xyz_d.grad is None                                                   # centres carry no gradient
    for kind in POS_TOL:
        assert torch.isfinite(got[kind]).all()
        print(f'POS {case} {arith} {kind}: kernels {_err(got[kind], ref[kind]):.3e}  fp32-pytorch {_err(yard[kind], ref[kind]):.3e}')
    for kind, tol in POS_TOL.items():
        assert _err(got[kind], ref[kind]) <= tol, (kind, _err(got[kind], ref[kind]), tol)


def test_pos_embed_refusals():
    from point_dae_amd import nn_ops
    xyz = torch.zeros(4, 3)
    seq6 = nn.Sequential(nn.Linear(3, 6), nn.GELU(), nn.Linear(6, 16)).to(DEV)
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        nn_ops.pos_embed(xyz.to(DEV), seq6)
    seq8 = nn.Sequential(nn.Linear(3, 8), nn.GELU(), nn.Linear(8, 16))
    with pytest.raises(RuntimeError, match='no CPU path'):
        nn_ops.pos_embed(xyz, seq8)


# ===================================================================================================================
# 4. pdae_mean_sum2, pdae_chamfer_backward_mean and ChamferDistanceL2
# ===================================================================================================================
def ref_mean_sum2(a, b):
    """fp64 mean(a) + mean(b) of positive fp32 inputs, and the kernels' forward error bound.  Per input of n elements a
    term passes: the thread-strided serial chain (128 x 256 threads: ceil(n / 32768) additions), 6 shuffle levels,
    3 additions of the four waves' LDS slots; in the final kernel 1 + 6 more, the division and the last addition:
    ceil(n / 32768) + 18 roundings.  The inputs are positive, so A is the mean itself."""
    ma, mb = a.double().mean().item(), b.double().mean().item()
    ra, rb = (math.ceil(t.numel() / 32768) + 18 for t in (a, b))
    return ma + mb, gamma(ra) * ma + gamma(rb) * mb


def _final_kernel_on_host(part, na, nb):
    """mean_sum2_final_kernel in fp32 torch: lane l adds partials l and l + 64, six xor-butterfly levels (every lane of a
    pair forms the same commutative sum), sa / na + sb / nb -- each operation rounded once on either side"""
    lane = torch.arange(64)

    def total(p):
        v = p[:64] + p[64:128]
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ o]
        return v[0]
    return total(part[:128]) / torch.tensor(float(na), dtype=torch.float32) + \
        total(part[128:256]) / torch.tensor(float(nb), dtype=torch.float32)


def run_mean_sum2(a, b, guard=64):
    """a, b on the device -> the workspace as _ChamferL2Loss lays it out (256 partials, the result in float 256), with
    a NaN guard band behind it"""
    ws = _nan((257 + guard,))
    _L().call('pdae_mean_sum2', a, a.numel(), a.data_ptr(), b.numel(), b.data_ptr(), ws.data_ptr(), ws.data_ptr() + 4 * 256)
    return ws.cpu()


@pytest.mark.parametrize('na,nb', [(1, 1), (7, 32769), (65536 + 3, 5), (2_000_003, 131_072)], ids=str)
def test_mean_sum2_bound_layout_and_repeatability(na, nb):
    rng = np.random.default_rng([na % 1000, nb % 1000, 4])
    a = _up(rng.uniform(0.0, 1.0, na).astype(np.float32) ** 2 * 3.0)           # positive, as squared distances are
    b = _up(rng.uniform(0.0, 1.0, nb).astype(np.float32) ** 2 * 3.0)
    ws = run_mean_sum2(a, b)
    _written(ws[:257])
    assert torch.isnan(ws[257:]).all()                                           # the guard band survives
    want, bound = ref_mean_sum2(a.cpu(), b.cpu())
    assert abs(ws[256].double().item() - want) <= bound, (ws[256].item(), want, bound)
    # floats 0..127 are the partial sums of a, 128..255 those of b (each within the first 9 + chain roundings of its
    # share), and float 256 is exactly what the final kernel makes of them
    for part, t in ((ws[:128], a), (ws[128:256], b)):
        s = t.double().sum().item()
        assert abs(part.double().sum().item() - s) <= gamma(math.ceil(t.numel() / 32768) + 9) * s
    assert torch.equal(ws[256], _final_kernel_on_host(ws[:256], na, nb))
    assert torch.equal(run_mean_sum2(a, b)[:257], ws[:257])                      # a fixed summation order: bit for bit


def test_mean_sum2_refusals():
    L = _L()
    a = _up(np.ones(8, np.float32))
    ws = _nan((257,))
    p, w, o = a.data_ptr(), ws.data_ptr(), ws.data_ptr() + 1024
    for args in ((0, p, 8, p, w, o), (8, p, 0, p, w, o), (8, None, 8, p, w, o), (8, p, 8, None, w, o), (8, p, 8, p, None, o),
                 (8, p, 8, p, w, None)):
        with pytest.raises(RuntimeError, match='mean_sum2: empty input or null pointer'):
            L.call('pdae_mean_sum2', a, *args)
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()


def ref_chamfer_mean_grad(a, b, idx1, idx2, g):
    """fp64 gradient of g (mean(dist1) + mean(dist2)) for GIVEN winners: the own terms 2 g / (B n) (a - b[idx1]) and
    2 g / (B m) (b - a[idx2]), and their negatives scattered onto the winners with index_add_ -> per cloud (grad, S, c):
    S the sum of the absolute values of the terms an element receives, c the number of scatter terms it receives"""
    B, n, _ = a.shape
    m = b.shape[1]
    a, b = a.double(), b.double()
    f1 = (idx1.long() + torch.arange(B).view(B, 1) * m).reshape(-1)             # flat rows of b that a's points won
    f2 = (idx2.long() + torch.arange(B).view(B, 1) * n).reshape(-1)
    a2, b2 = a.reshape(B * n, 3), b.reshape(B * m, 3)
    t1 = 2.0 * g / (B * n) * (a2 - b2[f1])
    t2 = 2.0 * g / (B * m) * (b2 - a2[f2])
    g1 = t1.clone().index_add_(0, f2, -t2)
    g2 = t2.clone().index_add_(0, f1, -t1)
    S1 = t1.abs().index_add_(0, f2, t2.abs())
    S2 = t2.abs().index_add_(0, f1, t1.abs())
    c1 = torch.zeros(B * n, dtype=torch.float64).index_add_(0, f2, torch.ones(B * m, dtype=torch.float64))
    c2 = torch.zeros(B * m, dtype=torch.float64).index_add_(0, f1, torch.ones(B * n, dtype=torch.float64))
    return (g1.view(B, n, 3), S1.view(B, n, 3), c1.view(B, n, 1)), (g2.view(B, m, 3), S2.view(B, m, 3), c2.view(B, m, 1))


def run_chamfer_forward(a, b):
    L = _L()
    B, n, _ = a.shape
    m = b.shape[1]
    ad, bd = _up(a), _up(b)
    d1, d2 = _nan((B, n)), _nan((B, m))
    i1 = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
    i2 = torch.full((B, m), -1, dtype=torch.int32, device=DEV)
    L.call('pdae_chamfer_forward', ad, B, n, ad.data_ptr(), m, bd.data_ptr(), d1.data_ptr(), d2.data_ptr(), i1.data_ptr(),
           i2.data_ptr())
    _written(d1, d2)
    assert i1.min().item() >= 0 and i1.max().item() < m and i2.min().item() >= 0 and i2.max().item() < n
    return d1.cpu(), d2.cpu(), i1.cpu(), i2.cpu()


def run_chamfer_backward(a, b, i1, i2, gd1=None, gd2=None, g=None):
    """pdae_chamfer_backward with the two distance gradients, or pdae_chamfer_backward_mean with the scalar g"""
    L = _L()
    B, n, _ = a.shape
    m = b.shape[1]
    ad, bd, i1d, i2d = _up(a), _up(b), _up(i1), _up(i2)
    g1, g2 = _nan((B, n, 3)), _nan((B, m, 3))
    if g is None:
        x, y = _up(gd1), _up(gd2)
        L.call('pdae_chamfer_backward', ad, B, n, ad.data_ptr(), m, bd.data_ptr(), i1d.data_ptr(), i2d.data_ptr(),
               x.data_ptr(), y.data_ptr(), g1.data_ptr(), g2.data_ptr())
    else:
        gl = torch.tensor(g, dtype=torch.float32, device=DEV)
        L.call('pdae_chamfer_backward_mean', ad, B, n, ad.data_ptr(), m, bd.data_ptr(), i1d.data_ptr(), i2d.data_ptr(),
               gl.data_ptr(), g1.data_ptr(), g2.data_ptr())
    _written(g1, g2)
    return g1.cpu(), g2.cpu()


# (B, n, m) and the path chamfer_backward_impl takes: packed needs n, m <= 256; the counting sort nq >= 4 mt
LOSS_CASES = [(37, 36, 32),        # packed gather, both directions: a fixed order
              (2, 600, 1100),      # own + atomic scatter, both directions
              (3, 4096, 300),      # 4096 onto 300: counting sort; 300 onto 4096: atomics
              (2, 257, 2050),      # the same with the roles swapped
              (5, 1024, 1),        # every query on one target (sorted); the one point onto its winner (atomics)
              (1, 300, 7)]         # 300 onto 7: counting sort; n > 256 keeps it off the packed path
_loss_cache = {}


def _loss_case(case):
    if case not in _loss_cache:
        B, n, m = case
        a, b = torch.from_numpy(make_clouds(81, B, n)), torch.from_numpy(make_clouds(82, B, m))
        _loss_cache[case] = (a, b) + run_chamfer_forward(a, b)
    return _loss_cache[case]


def _order_free(got, other, S, c, what):
    """two sums of the SAME fp32 terms in unspecified orders: each is within gamma(c) S of the exact sum of its c + 1
    terms (c additions), so the worst case of the difference is 2 c u S; the issue's (c + constant) u S with the
    constant 3 is asserted where it is the smaller (c >= 3) -- rounding errors of a sum grow as sqrt(c), far inside.
    c = 0 (the own term alone) asks for equal bits.  S is the reference's, a relative gamma(3) from the fp32 terms'
    (see below)."""
    _within(got, other.double(), torch.minimum(2 * c, c + 3) * U * S * (1 + gamma(3)), what)


@pytest.mark.parametrize('g', [1.0, -0.37])
@pytest.mark.parametrize('case', LOSS_CASES, ids=str)
def test_chamfer_backward_mean_on_every_backward_path(case, g):
    B, n, m = case
    a, b, d1, d2, i1, i2 = _loss_case(case)
    g32 = np.float32(g)
    m1, m2 = run_chamfer_backward(a, b, i1, i2, g=float(g32))
    # the constant gradients of the two means, each rounded once in fp32 as the kernel's g / (float)(B n) is
    gd1 = torch.full((B, n), float(g32 / np.float32(B * n)), dtype=torch.float32)
    gd2 = torch.full((B, m), float(g32 / np.float32(B * m)), dtype=torch.float32)
    assert gd1[0, 0].item() == float(g32 / np.float32(B * n))
    p1, p2 = run_chamfer_backward(a, b, i1, i2, gd1, gd2)
    (r1, S1, c1), (r2, S2, c2) = ref_chamfer_mean_grad(a, b, i1, i2, float(g32))
    if case == LOSS_CASES[0]:                    # the gather form adds in a fixed order: the same bits
        assert torch.equal(m1, p1) and torch.equal(m2, p2)
    else:
        _order_free(m1, p1, S1, c1, 'grad_xyz1: mean form against the plain backward')
        _order_free(m2, p2, S2, c2, 'grad_xyz2: mean form against the plain backward')
    # against fp64: a term 2 fl(g / div) fl(a - b) passes 3 roundings (the division, the subtraction, the product; x 2
    # is exact), and an element's c + 1 terms are added in c additions, in whatever order: gamma(c + 3) S
    _within(m1, r1, (c1 + 3) * U / (1 - (c1 + 3) * U) * S1, 'grad_xyz1 against fp64')
    _within(m2, r2, (c2 + 3) * U / (1 - (c2 + 3) * U) * S2, 'grad_xyz2 against fp64')
    if case == (5, 1024, 1):
        assert c2.max().item() == 1024
    if case == (2, 600, 1100):
        assert c1.max().item() >= 3 and c2.min().item() == 0


@pytest.mark.parametrize('case', LOSS_CASES, ids=str)
def test_chamfer_l2_module_loss_and_backward(case):
    from point_dae_amd.chamfer_dist import ChamferDistanceL2
    B, n, m = case
    a, b, d1, d2, i1, i2 = _loss_case(case)
    ad, bd = _up(a).requires_grad_(True), _up(b).requires_grad_(True)
    loss = ChamferDistanceL2()(ad, bd)
    assert loss.shape == () and loss.dtype == torch.float32
    want, bound = ref_mean_sum2(d1.reshape(-1), d2.reshape(-1))                 # the distances are bit-exact (test_gpu_ops.py)
    assert abs(loss.double().item() - want) <= bound, (loss.item(), want, bound)
    loss.backward()
    m1, m2 = run_chamfer_backward(a, b, i1, i2, g=1.0)
    if case == LOSS_CASES[0]:
        assert torch.equal(ad.grad.cpu(), m1) and torch.equal(bd.grad.cpu(), m2)
    else:
        (_, S1, c1), (_, S2, c2) = ref_chamfer_mean_grad(a, b, i1, i2, 1.0)
        _order_free(ad.grad.cpu(), m1, S1, c1, 'xyz1.grad against the direct call')
        _order_free(bd.grad.cpu(), m2, S2, c2, 'xyz2.grad against the direct call')


# ===================================================================================================================
# 5. Chamfer forward: ties and ragged tails on chamfer_fwd_tiled<4> and chamfer_fwd_many
# ===================================================================================================================
# Per case: the shape, and plants (I, Q): the points I of cloud 2 and Q of cloud 1 all moved onto one far lattice point of
# their own, so that direction 1's queries Q tie (distance 0) over the candidates I and must answer min(I), and direction
# 2's queries I tie over Q and must answer min(Q).  Paths by chamfer_fwd_dir: a direction with n queries and m candidates
# takes tiled<4> when n >= 4096 (or B ceil(n / 1024) >= 1024), else `many` when m >= 2048, else tiled<1> (n > 256).
FORWARD_CASES = {
    # direction 1: 4100 queries -> tiled<4>: its fifth block holds 4 live queries (4096..4099); 4102 candidates are four
    # 1024-tiles and a 6-candidate tail.  Direction 2: 4102 queries -> tiled<4> as well (n >= 4096 wins over m >= 2048):
    # 6 live queries in the last block, 4100 candidates with a 4-candidate tail
    'tiled4-both (1, 4100, 4102)': ((1, 4100, 4102), [([1023, 1024, 4101], [1023, 1024, 4099]),    # across a tile edge + the tail
                                                      ([4097, 4100], [4097, 4098]),               # inside the tail
                                                      ([7, 8], [7, 8]), ([3071, 3072], [2047, 2048])]),
    # the shape that puts direction 2 on `many` next to a tiled<4> direction 1: 3078 queries (< 4096) against m = 4100
    # candidates = two full 2048-tiles and a 4-candidate tail (one whole quad); direction 1: 4100 queries -> tiled<4>, three
    # 1024-tiles and a 6-candidate tail
    'tiled4-many (1, 4100, 3078)': ((1, 4100, 3078), [([1023, 1024, 3077], [2047, 2048, 4099]),    # across a tile edge + the tail
                                                      ([3073, 3076], [4097, 4098]),               # inside the tail
                                                      ([7, 8], [7, 8]),                           # `many`: minimum 3 holds 7, minimum 0 holds 8
                                                      ([2047, 2048], [4094, 4096]),               # last full quad / tail quad
                                                      ([100], [13, 14, 15, 16])]),                # minima 1, 2, 3 of one quad, 0 of the next
    # direction 1: 257 queries, 2051 candidates -> many: one full tile, then a tail of 3 padded to 4 with +inf.
    # Direction 2: 2051 queries, 257 candidates -> tiled<1>
    'many-pad1 (2, 257, 2051)': ((2, 257, 2051), [([2047, 2048, 2050], [0, 256]), ([2049], [5, 6]), ([7, 8], [100, 101])]),
    # the same with a tail of 2 padded with two +inf
    'many-pad2 (2, 257, 2050)': ((2, 257, 2050), [([2047, 2048], [0, 256]), ([2049], [5, 6]), ([7, 8], [100, 101])]),
}


def _forward_clouds(shape, plants, lattice):
    B, n, m = shape
    a, b = make_clouds(91, B, n), make_clouds(92, B, m)
    if lattice:                                  # 343 lattice points: hundreds of exact ties per query
        a, b = np.round(a * 3) / 3, np.round(b * 3) / 3
    for j, (I, Q) in enumerate(plants):
        far = np.array([3 + j, -3 - j, 3 + j], np.float32)
        b[:, I], a[:, Q] = far, far
    return a.astype(np.float32), b.astype(np.float32)


@pytest.mark.parametrize('lattice', [True, False], ids=['lattice', 'random'])
@pytest.mark.parametrize('name', list(FORWARD_CASES))
def test_chamfer_forward_ties_and_ragged_tails_on_tiled4_and_many(oracle_ops, name, lattice):
    shape, plants = FORWARD_CASES[name]
    a, b = _forward_clouds(shape, plants, lattice)
    wd1, wd2, wi1, wi2 = oracle_ops.chamfer_forward(a, b)
    for I, Q in plants:                          # the plants decide what they were planted for
        assert (wi1[:, Q] == min(I)).all() and (wd1[:, Q] == 0).all()
        assert (wi2[:, I] == min(Q)).all() and (wd2[:, I] == 0).all()
    if lattice:                                  # and every query ties on its own: each lattice point is there several times
        assert len(np.unique(b[0], axis=0)) < shape[2] // 4 and len(np.unique(a[0], axis=0)) <= 343 + len(plants)
    d1, d2, i1, i2 = run_chamfer_forward(torch.from_numpy(a), torch.from_numpy(b))
    for got, want in ((i1, wi1), (i2, wi2), (d1, wd1), (d2, wd2)):
        np.testing.assert_array_equal(got.numpy(), want)
    from point_dae_amd import chamfer_dist
    for got, want in zip(chamfer_dist.forward(_up(a), _up(b)), (wd1, wd2, wi1, wi2)):        # the wrapper
        np.testing.assert_array_equal(got.cpu().numpy(), want)
