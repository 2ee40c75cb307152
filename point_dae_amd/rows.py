"""The row-GEMM wrappers every model file builds on: products of flat (rows, channels) activations.

A leaf of the package (it imports only _lib, arena and probe), so a model file, nn_ops.py, patch_embed.py and
sa_mlp.py all take these from here and from nowhere else:
  * empty / colsum, the allocation and the bias-gradient column sum;
  * the operand padding helpers (pad2d, insert_zero_col, split_weight_cols: csrc/glue.hip) -- the row GEMMs reduce in
    multiples of 4 and write multiples of 4;
  * rows_gemm, its few-rows split-K variant and the grouped weight gradients rows_wgrad (csrc/rows_gemm.hip: fused
    bias / ReLU / GELU / GELU' epilogues, split-K slabs, no BLAS library), each launch timed as a family for bench.py;
  * the BatchNorm-aware forms the patch embedder, the set-abstraction MLP and DGCNN share (wgrad_listed, gemm_bnstats,
    bn_finalize, bn_eval_affine);
  * linear_any: x W^T + b (+ ReLU) for any K, N as one autograd node.
"""
import os

import torch
import torch.nn.functional as F

from . import _lib
from .arena import arena
from .probe import probed_family


def empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


def colsum(x):
    """Column sums (bias gradients) into a pre-zeroed arena slice."""
    out, _ = arena.take(x.shape[1], x)
    _lib.call('pdae_colsum', x, x.shape[0], x.shape[1], _lib.ptr(x), _lib.ptr(out), 1)
    return out


class _Pad2d(torch.autograd.Function):
    """x (R, C) [or (C,)] -> (R + pr, C + pc) with zeros, one launch (csrc/glue.hip pad2d; F.pad is a fill + a copy)."""

    @staticmethod
    def forward(ctx, x, pr, pc):
        one_d = x.dim() == 1
        x2 = x.reshape(1, -1) if one_d else x
        if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
            x2 = x2.contiguous()                        # (a column slice of a row-major matrix is read through its row stride)
        R, C = x2.shape
        ld = x2.stride(0) if R > 1 else C
        out = empty((R + pr, C + pc), x2)
        _lib.call('pdae_pad2d', x2, R, C, ld, R + pr, C + pc, _lib.ptr(x2), _lib.ptr(out))
        ctx.dims = (R, C, one_d)
        return out.reshape(-1) if one_d else out

    @staticmethod
    def backward(ctx, g):
        R, C, one_d = ctx.dims
        return (g[:C] if one_d else g[:R, :C]), None, None


PAD2D = os.environ.get('PDAE_PAD2D', os.environ.get('PDAE_GLUE', '1')) != '0'

# A backward whose parameter inputs all have requires_grad == False (a frozen model differentiated with respect to its
# input: saliency_ops) skips its weight-gradient launches.  (A/B: 0 = they are issued anyway, as before; with any
# parameter requiring a gradient the switch changes nothing)
SKIP_FROZEN_WGRAD = os.environ.get('PDAE_SKIP_FROZEN_WGRAD', '1') != '0'


def pad2d(x, pr, pc):
    """zero rows below / zero columns right of a 1-D or 2-D fp32 device tensor (1-D: pc elements appended)."""
    if not PAD2D or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (1, 2):
        return F.pad(x, (0, pc, 0, pr)) if x.dim() == 2 else F.pad(x, (0, pc))
    return _Pad2d.apply(x, pr, pc)


def _hcat(pieces, R, like):
    """pieces: [(2-D tensor or None, cols)] -> (R, sum cols) with the pieces' leading columns side by side (None: zeros)."""
    out = empty((R, sum(c for _, c in pieces)), like)
    _lib.call('pdae_hcat', like, len(pieces), R, _lib.ptr_array([t for t, _ in pieces]), _lib.int_array([c for _, c in pieces]),
              _lib.int_array([(t.stride(0) if t is not None else c) for t, c in pieces]), _lib.ptr(out))
    return out


class _InsertZeroCol(torch.autograd.Function):
    """w (R, C) -> (R, C + 1) with a zero column at `at` (the pad column of a set-abstraction level's first weight: the grouped
    rows are [xyz - centre | 0 | features]); one launch each way (was new_zeros + cat, and two slice gradients + their add)."""

    @staticmethod
    def forward(ctx, w, at):
        w = w.contiguous()
        R, C = w.shape
        ctx.at, ctx.shape = at, (R, C)
        pieces = [(w, at), (None, 1)] + ([(w[:, at:], C - at)] if C > at else [])
        return _hcat(pieces, R, w)

    @staticmethod
    def backward(ctx, g):
        R, C = ctx.shape
        g = g.contiguous()
        pieces = [(g, ctx.at)] + ([(g[:, ctx.at + 1:], C - ctx.at)] if C > ctx.at else [])
        return _hcat(pieces, R, g), None


def insert_zero_col(w, at):
    if not PAD2D or not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or not 0 < at <= w.shape[1]:
        return torch.cat([w[:, :at], w.new_zeros(w.shape[0], 1), w[:, at:]], dim=1)
    return _InsertZeroCol.apply(w, at)


class _SplitWeightCols(torch.autograd.Function):
    """w (R, C) -> its column blocks [b0, b1), ... as separate contiguous operands, each zero-padded to a multiple of 4 columns
    (one launch per block: pad2d reads the block through w's row stride); backward: the blocks' gradients side by side as dW
    in ONE launch (csrc/glue.hip hcat) -- autograd's own path is a zero fill + a copy per block and the adds between them."""

    @staticmethod
    def forward(ctx, w, *bounds):
        w = w.contiguous()
        R, C = w.shape
        outs = []
        for b0, b1 in zip(bounds[0::2], bounds[1::2]):
            n = b1 - b0
            o = empty((R, n + (-n) % 4), w)
            _lib.call('pdae_pad2d', w, R, n, C, R, o.shape[1], w.data_ptr() + 4 * b0, _lib.ptr(o))
            outs.append(o)
        ctx.bounds, ctx.shape = bounds, (R, C)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        R, C = ctx.shape
        widths = [b1 - b0 for b0, b1 in zip(ctx.bounds[0::2], ctx.bounds[1::2])]
        gs = [g.contiguous() if g is not None else None for g in gs]
        like = next(g for g in gs if g is not None)
        srcs = [g if g is not None else torch.zeros((R, n + (-n) % 4), device=like.device) for g, n in zip(gs, widths)]
        dw = empty((R, C), like)
        _lib.call('pdae_hcat', like, len(srcs), R, _lib.ptr_array(srcs), _lib.int_array(widths),
                  _lib.int_array([t.shape[1] for t in srcs]), _lib.ptr(dw))
        return (dw,) + (None,) * len(ctx.bounds)


def split_weight_cols(w, bounds):
    """w (R, C), bounds = [(b0, b1), ...] covering 0..C in order, at most four -> the column blocks as contiguous (R, width padded
    to a multiple of 4) operands."""
    flat = [v for b in bounds for v in b]
    ok = (PAD2D and w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and 1 <= len(bounds) <= 4 and flat[0] == 0
          and flat[-1] == w.shape[1] and all(flat[2 * i + 1] == flat[2 * i + 2] for i in range(len(bounds) - 1))
          and all(b1 > b0 for b0, b1 in bounds))
    if not ok:
        return tuple(pad2d(w[:, b0:b1], 0, (-(b1 - b0)) % 4) for b0, b1 in bounds)
    return _SplitWeightCols.apply(w, *flat)


# Tile shapes for the FoldingNet stage's multi-millisecond products (tools/lab/rows_big.py, 524288 x 512 x 512: bias+ReLU
# forward 96x128 tiles 126.7 vs 121.9 TFLOP/s on 64x64; ReLU-masked data gradient 128x128 123.0 vs 115.7)
BIG_ROWS = 1 << 19                 # (the published variant's 190 k-row stages are faster on the planned 64x64 tiles: 17.55 vs 17.63 ms)


def _row_ptr(t, row):
    """Address of row `row` of a contiguous fp32 (rows, cols) operand (None stays None); split-K slabs (S, rows, cols)
    only ever start at row 0."""
    return t.data_ptr() + 4 * row * t.shape[-1] if t is not None else None


def rows_gemm(x, w, w_kn=False, bias=None, epi=0, z=None, may_split=False, big_cfg=None):
    """y = epi(x . op(w)) on the row-GEMM family (csrc/rows_gemm.hip, include/pdae.h).
    w_kn False: w is (N, K), torch's (out, in): a Linear's forward; True: w is (K, N): the same
    weight as the data-gradient operand.  epi 0 store (+bias) | 1 bias+ReLU | 2 GELU(z) -> y and
    GELU'(z) -> z | 3 y = acc * z.  may_split: the result may be (S, M, N) split-K slabs whose
    consumer adds them up (the LayerNorm kernels do)."""
    M, K = x.shape
    N = w.shape[1] if w_kn else w.shape[0]
    # the kernels address an operand with 32-bit byte offsets: one of 4 GB or more goes in row chunks, each a launch of its
    # own without split-K; every other product is the one chunk of all M rows
    chunk = ((1 << 30) // max(K, N) - 1) // 128 * 128 if M * max(K, N) >= 1 << 30 else M
    for m0 in (range(0, M, chunk) if chunk < M else (0,)):
        rows = min(chunk, M - m0)
        cfg, splits, sb = _lib.rows_gemm_plan(rows, N, K, w_kn, may_split and chunk == M)
        if big_cfg is not None and cfg < 16 and rows >= BIG_ROWS and splits == 1:
            cfg = big_cfg     # a caller's measured fp32-input tile shape for a multi-millisecond product (that plan is calibrated
                              # on M <= 8192; the exact-split family's plan, cfg >= 16, prices rounds and stands)
        if m0 == 0:
            y = empty((splits, M, N) if splits > 1 else (M, N), x)
        probed_family('rows_gemm', 2.0 * rows * N * K,
                      lambda m0=m0, rows=rows, cfg=cfg, splits=splits, sb=sb: _lib.call(
                          'pdae_rows_gemm', x, rows, N, K, _row_ptr(x, m0), _lib.ptr(w), int(w_kn), _lib.ptr(bias), epi,
                          _row_ptr(z, m0), _row_ptr(y, m0), cfg, splits, sb),
                      nbytes=4.0 * (rows * K + N * K + splits * rows * N + (rows * N if z is not None else 0)))
    return y


def rows_gemm_few_rows(x, w, w_kn, bias, epi, z=None):
    """rows_gemm for a handful of rows against a long reduction: planned with up to 8 split-K slabs, which
    pdae_slab_sum_epi adds with the bias and the epilogue (one GEMM launch when the plan keeps one slab)."""
    M, K = x.shape
    N = w.shape[1] if w_kn else w.shape[0]
    cfg, splits, sb = _lib.rows_gemm_plan(M, N, K, w_kn, 8)
    if splits == 1:
        return rows_gemm(x, w, w_kn, bias, epi, z)
    slabs = empty((splits, M, N), x)
    y = empty((M, N), x)

    def both():                                     # the product is complete only behind the slab sum: one probed unit
        _lib.call('pdae_rows_gemm', x, M, N, K, _lib.ptr(x), _lib.ptr(w), int(w_kn), None, 0, None,
                  _lib.ptr(slabs), cfg, splits, sb)
        _lib.call('pdae_slab_sum_epi', x, splits, M, N, _lib.ptr(slabs), _lib.ptr(bias), epi, _lib.ptr(z), _lib.ptr(y))
    # bytes: operands + the slabs written by the GEMM, then the slabs read and the result written by the sum
    probed_family('rows_gemm', 2.0 * M * N * K, both, nbytes=4.0 * (M * K + N * K + 2 * slabs.numel() + M * N))
    return y


def rows_wgrad(dys, xs, with_bias, outs=None, db_outs=None):
    """Weight (and bias) gradients of a group of Linear layers that share their rows, one grouped
    launch (+ the ordered slab reduction, complete when the call returns to the stream).  -> ([dW], [db or None]);
    outs / db_outs: preallocated outputs (db_outs: one per True in with_bias), e.g. the flat gradient views of an armed
    FlatDataParallel (nn_ops.py, the gradient sink)."""
    M = dys[0].shape[0]
    Ns, Ks = [t.shape[1] for t in dys], [t.shape[1] for t in xs]
    ws = empty((max(_lib.rows_wgrad_workspace(M, Ns, Ks), 1),), dys[0])
    dws = outs if outs is not None else [empty((n, k), dys[0]) for n, k in zip(Ns, Ks)]
    it = iter(db_outs) if db_outs is not None else None
    dbs = [(next(it) if it is not None else empty((n,), dys[0])) if f else None for n, f in zip(Ns, with_bias)]
    probed_family('rows_wgrad', 2.0 * M * sum(n * k for n, k in zip(Ns, Ks)),
                  lambda: _lib.rows_wgrad(dys[0], M, dys, xs, dws, dbs, ws),
                  nbytes=4.0 * sum(M * (n + k) + n * k for n, k in zip(Ns, Ks)))
    return dws, dbs


# the weight gradients with group-listed operands and BatchNorm + ReLU recomputed (the patch embedder's, the set-abstraction
# MLP's) on the grouped kernel of csrc/rows_gemm.hip (ordered reduction, no atomics, no memset)
def wgrad_listed(M, dy, a_groups, x, b_groups, scale=None, shift=None, bias=False):
    """dW (N, K) = sum over the M listed rows of dy^T . relu(x * scale + shift) [-> (dW, column sums of dy or None)]."""
    N, K = dy.shape[1], x.shape[1]
    dw = empty((N, K), x)
    db = empty((N,), x) if bias else None
    ws = empty((max(_lib.rows_wgrad_workspace(M, [N], [K]), 1),), x)
    probed_family('rows_wgrad', 2.0 * M * N * K,
                  lambda: _lib.call('pdae_rows_wgrad_listed', x, M, N, K, _lib.ptr(dy), _lib.ptr(a_groups), _lib.ptr(x),
                                    _lib.ptr(b_groups), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(dw), _lib.ptr(db),
                                    _lib.ptr(ws)), nbytes=4.0 * (M * (N + K) + N * K))
    return dw, db


def gemm_bnstats(dy, w, X, groups, sc, sh, mean, invstd):
    """The data gradient dy . w (w (K, N) as stored: a conv / Linear weight (out, in)) that flows into relu(bn(X)), with the
    ReLU mask applied and BatchNorm-backward's two column sums S (2, N) out of the same launch (csrc/rows_gemm.hip
    pdae_rows_gemm_bnrelu_stats) -> (t, S).  X rows through `groups` (int32 list of 32-row groups) when given."""
    M, K = dy.shape
    N = w.shape[1]
    t = empty((M, N), dy)
    S = empty((2, N), dy)
    ws = empty((max(_lib.lib().pdae_rows_gemm_bnrelu_stats_workspace(M, N), 1),), dy)
    probed_family('rows_gemm', 2.0 * M * N * K,
                  lambda: _lib.call('pdae_rows_gemm_bnrelu_stats', dy, M, N, K, _lib.ptr(dy), _lib.ptr(w), _lib.ptr(X),
                                    _lib.ptr(groups), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(mean), _lib.ptr(invstd),
                                    _lib.ptr(t), _lib.ptr(S), _lib.ptr(ws)),
                  nbytes=4.0 * (M * K + N * K + 2 * M * N))
    return t, S


def bn_finalize(bn, rows, like, stats64=None, partials=None):
    """Training-mode BatchNorm bookkeeping in one launch (csrc/embed.hip bn_finalize):
    -> scale, shift, mean, invstd; updates the running estimates and the counter."""
    C = bn.weight.numel()
    scale, shift, mean, invstd = (empty((C,), like) for _ in range(4))
    m = bn.momentum if bn.momentum is not None else 0.1
    track = bn.track_running_stats and bn.running_mean is not None
    _lib.call('pdae_bn_finalize', like, C, rows, _lib.ptr(stats64), _lib.ptr(partials),
              partials.shape[0] if partials is not None else 0, _lib.ptr(bn.weight), _lib.ptr(bn.bias),
              float(bn.eps), float(m), _lib.ptr(bn.running_mean) if track else None,
              _lib.ptr(bn.running_var) if track else None,
              _lib.ptr(bn.num_batches_tracked) if track else None,
              _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(mean), _lib.ptr(invstd))
    return scale, shift, mean, invstd


def bn_eval_affine(bn):
    """Eval-mode BatchNorm (running estimates) as y = x * scale + shift -> scale, shift, mean, invstd, contiguous."""
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    scale = bn.weight * invstd
    shift = bn.bias - bn.running_mean * scale
    return scale.contiguous(), shift.contiguous(), bn.running_mean.contiguous(), invstd.contiguous()


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b) on rows; act None or 'relu' (the ReLU mask is recomputed from y)."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        x = x.contiguous()
        y = rows_gemm(x, w, False, b, 1 if relu else 0)
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.has_bias, ctx.relu = b is not None, relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.relu:
            dy = dy * (y > 0)
        dx = rows_gemm(dy, w, True) if ctx.needs_input_grad[0] else None
        if SKIP_FROZEN_WGRAD and not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return dx, None, None, None
        dws, dbs = rows_wgrad([dy], [x], [ctx.has_bias])
        return dx, dws[0], dbs[0], None


def linear_any(x, w, b=None, relu=False):
    """x W^T (+ b) (+ ReLU) for any K, N on the row GEMMs: they reduce in multiples of 4 and write
    multiples of 4, so a ragged weight (K = 3 xyz columns, N = 3 output coordinates) is zero-padded
    (the weight is small; an activation is padded only when it is narrow -- wide ones should be built
    padded by the caller, as the set-abstraction grouping does)."""
    if not (x.dim() == 2 and x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError('linear_any: rows must be a 2-D fp32 tensor on the GPU (there is no CPU / library path)')
    N, K = w.shape
    pk, pn = (-K) % 4, (-N) % 4
    if pk:
        if x.shape[1] == K:
            x = pad2d(x, 0, pk)
    if pk or pn:
        w = pad2d(w, pn, pk)                            # (both paddings of the weight in one launch)
    if pn:
        b = pad2d(b, 0, pn) if b is not None else None
    y = _Linear.apply(x, w, b, relu)
    return y[:, :N] if pn else y
