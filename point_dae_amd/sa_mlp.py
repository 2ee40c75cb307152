"""Shared MLP + max-pool of a PointNet++ set-abstraction level as one autograd Function, and the level's grouping.

Reference: extensions/pointnet2/pointnet2_modules.py (PointnetSAModule.forward: SharedMLP of
Conv2d(1x1, bias=False) -> BatchNorm2d -> ReLU layers on (B, C, npoint, nsample), then
F.max_pool2d over nsample), used by models/pointnetv2_util.py:319-346 for Point_CAE_PointNetv2.

On rows = (cloud, centre, sample) a 1x1 conv is a GEMM and the activations of a level are
1-2 M rows x 64-256 channels (0.5-1 GB each), so every pass over one costs as much as the GEMM that
made it.  Layout of the fused version (csrc/gemm.hip conv_stats, csrc/set_abstraction.hip,
csrc/embed.hip), the patch embedder's recipe:
  forward   per layer ONE kernel: the previous layer's BatchNorm + ReLU is applied while the
            operand is staged, this layer's batch statistics come out of the epilogue, only the
            raw conv output y_l is stored; bn_finalize turns the sums into scale / shift and
            updates the running estimates; the last layer's BatchNorm + ReLU + max over nsample
            is one read of y_3.
  backward  max-pool scatter (dense), then per layer: ReLU + BatchNorm backward in two sweeps
            (bnrelu_backward: the sums that are dgamma / dbeta, then the in-place apply), the
            weight gradient with the normalised input recomputed in the GEMM's producer, the
            data gradient on the row GEMMs.
ATen ran ~7 passes per layer forward (stats, transform, clamp) and ~6 backward.

The chain is written once: mlp_max_forward / mlp_max_backward.  SharedMLPMaxFunction runs it from layer 0 on grouped
rows (group_rows), SplitFirstMLPMaxFunction from layer 1 behind csrc/sa_train.hip, sa_eval_ops.group_all runs the forward
with running-estimate affines.  Each layout a kernel form takes is one predicate beside the wrapper it guards.
"""
import torch
import torch.nn as nn

from . import _lib
from .rows import _hcat, bn_finalize, empty, gemm_bnstats, insert_zero_col, rows_gemm, rows_wgrad, wgrad_listed


# Parity-test hook (None in production): called as ARG_HOOK(arg) with the (groups, C) uint8 winners of a level's
# max-pool right after the forward computed them; what it returns is what the backward routes the gradient through.
# The reference's own winners can be injected this way, so that a gradient comparison is not at the mercy of near-ties
# that 1 ulp of GEMM rounding resolves the other way (tests/test_gpu_model.py).
ARG_HOOK = None


def mlp_max_forward(inp, sc, sh, ws, affine, ns, hook=True):
    """The chain from a staged input on: inp (R, K) rows, R = groups * ns, with the pending BatchNorm scale / shift of the
    layer that made them (None: inp is taken as it is); ws the weights (C_l, C_{l-1}) of the layers to run;
    affine(i, stats) -> the BatchNorm of ws[i] as (scale, shift, ...) given its batch-statistic partials: bn_finalize in
    training mode, the running-estimate affine in evaluation mode.  hook: hand the winners to ARG_HOOK.
    -> out (groups, C_last), its winners arg, the raw outputs ys and the affines, one per layer of ws."""
    R = inp.shape[0]
    ys, affs = [], []
    for i, w in enumerate(ws):
        N, K = w.shape
        y = empty((R, N), inp)
        stats = empty((8, 2, N), inp)
        _lib.call('pdae_conv_stats', inp, R, N, K, _lib.ptr(inp), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(w),
                  _lib.ptr(y), _lib.ptr(stats))
        aff = affine(i, stats)
        sc, sh = aff[0], aff[1]
        ys.append(y)
        affs.append(aff)
        inp = y
    G, C = R // ns, inp.shape[1]
    out = empty((G, C), inp)
    arg = empty((G, C), inp, torch.uint8)
    _lib.call('pdae_bnrelu_group_max', inp, G, ns, C, _lib.ptr(inp), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(out),
              _lib.ptr(arg))
    if hook and ARG_HOOK is not None:
        arg = ARG_HOOK(arg).contiguous()
    return out, arg, ys, affs


def _batch_affine(bns, R):
    """mlp_max_forward's affine in training mode: scale, shift, mean, invstd of the batch (rows.bn_finalize)."""
    return lambda i, stats: bn_finalize(bns[i], R, stats, partials=stats)


def fused_pool_supported(C):
    """Whether the max-pool gradient goes straight through the pool (pool_bn_backward) at the pooled width C: mirrors that
    entry's check in csrc/set_abstraction.hip ("C/4 must divide 256", C at most 1024)."""
    return 256 % (C // 4) == 0 and C <= 1024


def mlp_max_backward(dout, arg, out, ns, ys, affs, ws, gammas):
    """The chain's backward from the pooled gradient dout (groups, C_last) down to and including layer 0's BatchNorm
    backward; ws[l] is read for l >= 1 only.  -> d, the gradient of the raw first-layer output ys[0], and the gradient
    slots (dw, dgamma, dbeta) per layer, every one filled but layer 0's dw.

    BatchNorm l's backward takes one of three forms: straight through the max-pool (the last layer, where the kernel
    takes the width); the apply sweep alone, when the GEMM that produced d left that BatchNorm's sums
    (rows.gemm_bnstats); else both sweeps on the dense d."""
    nl = len(ys)
    R, C = ys[-1].shape
    G = R // ns
    x = ys[-1]
    grads = [None] * (3 * nl)
    d = empty((R, C), x)
    dout = dout.contiguous()
    fused_pool = fused_pool_supported(C)
    if not fused_pool:
        _lib.call('pdae_group_max_scatter_n', x, G, ns, C, _lib.ptr(dout), _lib.ptr(arg), _lib.ptr(d))
    S_pre = None                     # BatchNorm l's sums when the GEMM that produced d left them (rows_gemm_bnrelu_stats)
    for l in range(nl - 1, -1, -1):
        sc, sh, mean, invstd = affs[l]
        N = ys[l].shape[1]
        S = empty((2, N), x) if S_pre is None else S_pre
        if l == nl - 1 and fused_pool:
            # straight through the max-pool: the gradient is non-zero only at the arg-max rows
            wsp = empty((max(_lib.lib().pdae_pool_bn_backward_workspace(G, C), 1),), x)
            _lib.call('pdae_pool_bn_backward', x, G, ns, C, _lib.ptr(dout), _lib.ptr(arg), _lib.ptr(out),
                      _lib.ptr(ys[l]), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(gammas[l]), _lib.ptr(S),
                      _lib.ptr(wsp), _lib.ptr(d))
        else:
            # d <- gradient of the raw conv output y_l (ReLU mask, BatchNorm backward), in place
            _lib.call('pdae_bnrelu_backward' if S_pre is None else 'pdae_bnrelu_backward_apply', x, R // 32, N,
                      _lib.ptr(d), _lib.ptr(ys[l]), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(mean), _lib.ptr(invstd),
                      _lib.ptr(gammas[l]), _lib.ptr(S), None, R // 32, None, None, None)
        grads[3 * l + 1], grads[3 * l + 2] = S[1], S[0]                   # dgamma, dbeta
        if l > 0:
            psc, psh = affs[l - 1][0], affs[l - 1][1]
            # BatchNorm + ReLU of the previous layer recomputed while its raw output is staged (rows.wgrad_listed)
            grads[3 * l] = wgrad_listed(R, d, None, ys[l - 1], None, psc, psh)[0]
            # gradient of relu(bn(y_{l-1})), ReLU-masked, + that BatchNorm's sums out of the same launch
            d, S_pre = gemm_bnstats(d, ws[l], ys[l - 1], None, psc, psh, affs[l - 1][2], affs[l - 1][3])
    return d, grads


def _save_level(ctx, own, arg, out, ws, gammas, ys, affs):
    """What mlp_max_backward reads, behind the Function's own tensors (entries of own and ws may be None)."""
    ctx.save_for_backward(*own, arg, out, *ws, *gammas, *ys, *[t for a in affs for t in a])
    ctx.n_own, ctx.nl = len(own), len(ys)


def _saved_level(ctx):
    """-> own, arg, out, ws, gammas, ys, affs as _save_level took them."""
    t, nl = iter(ctx.saved_tensors), ctx.nl
    take = lambda n: [next(t) for _ in range(n)]
    own, (arg, out) = take(ctx.n_own), take(2)
    ws, gammas, ys = take(nl), take(nl), take(nl)
    return own, arg, out, ws, gammas, ys, [take(4) for _ in range(nl)]


def _level_params(layers, pad_at=None):
    """The level's _ConvBN modules -> the Functions' params (w (C_l, C_{l-1}), gamma, beta per layer) and the BatchNorm
    modules; pad_at: the first weight gets a zero column there."""
    params, bns = [], []
    for i, layer in enumerate(layers):
        w = layer.conv.weight.reshape(layer.conv.weight.shape[0], -1)
        if i == 0 and pad_at is not None:
            w = insert_zero_col(w, pad_at)
        bn = layer.bn.bn
        params += [w, bn.weight, bn.bias]
        bns.append(bn)
    return params, bns


def batch_stats_are_local(layers):
    """No SyncBatchNorm in the level: the fused forms compute BatchNorm's statistics over this replica's rows."""
    return not any(isinstance(layer.bn.bn, nn.SyncBatchNorm) for layer in layers)


def fused_chain_supported(per, rows, layers):
    """Whether SharedMLPMaxFunction takes a level's grouped rows: mirrors csrc/set_abstraction.hip check_sa
    ("bnrelu_group_max: 1 <= nsample <= 256") and the 32-row groups of the BatchNorm-backward sweeps, which
    SharedMLPMaxFunction.forward asks for."""
    return per <= 256 and rows % 32 == 0 and batch_stats_are_local(layers)


class SharedMLPMaxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ns, bns, *params):
        """x (R, K0) rows, R = groups * ns; params = (w, gamma, beta) per layer, w (C_l, C_{l-1})."""
        x = x.contiguous()
        R = x.shape[0]
        if R % ns != 0 or R % 32 != 0:
            raise RuntimeError('shared MLP: rows must be groups * nsample and a multiple of 32')
        ws = [params[i].contiguous() for i in range(0, len(params), 3)]
        gammas = [params[i] for i in range(1, len(params), 3)]
        out, arg, ys, affs = mlp_max_forward(x, None, None, ws, _batch_affine(bns, R), ns)
        _save_level(ctx, [x], arg, out, ws, gammas, ys, affs)
        ctx.ns = ns
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,), arg, out, ws, gammas, ys, affs = _saved_level(ctx)
        d, grads = mlp_max_backward(dout, arg, out, ctx.ns, ys, affs, ws, gammas)
        (grads[0],), _ = rows_wgrad([d], [x], [False])
        dx = rows_gemm(d, ws[0], True) if ctx.needs_input_grad[0] else None
        return (dx, None, None) + tuple(grads)


def shared_mlp_max(x, layers, ns, pad_at=None):
    """x (groups*ns, K0) -> (groups, C_last).  layers: the level's _ConvBN modules (conv without bias,
    BatchNorm2d, ReLU); pad_at: x carries a zero column there, the first weight gets the matching one."""
    params, bns = _level_params(layers, pad_at)
    return SharedMLPMaxFunction.apply(x, ns, bns, *params)


def split_first_supported(B, N, npoint, ns, C0, C1):
    """Whether csrc/sa_train.hip takes a level's layout (host-side query, nothing is read)."""
    return bool(_lib.lib().pdae_sa_first_supported(B, N, npoint, ns, C0, C1))


class SplitFirstMLPMaxFunction(torch.autograd.Function):
    """SharedMLPMaxFunction without the grouped rows: the level's first layer split by source point (csrc/sa_train.hip).

        y0[row] = P[b N + idx[row]] + W0x (xyz[idx[row]] - new_xyz[centre]),    P = features W0f^T on B N rows

    The feature half of the first product runs once per SOURCE point (sa2: B 512 rows instead of B 128 64) and only three
    FMAs on the centred difference stay per (centre, sample) row; no (R, 4 + C0) tensor is built.  From y0 on the chain is
    the shared one (mlp_max_forward from layer 1; mlp_max_backward down to dy0).  Then one entry turns dy0 into dP (per
    source point, ascending row order) and dW0x, and dW0f = dP^T features, dfeatures = dP W0f are products on B N rows."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, idx, features, bns, *params):
        """xyz (B,N,3), new_xyz (B,np,3), idx (B,np,ns) i32, features (B*N, C0) or None; params = (w, gamma, beta) per layer,
        the first w (C1, 3 + C0) as the module holds it."""
        B, N, _ = xyz.shape
        _, npoint, ns = idx.shape
        xyz, new_xyz, idx = xyz.contiguous(), new_xyz.contiguous(), idx.contiguous()
        C0 = 0 if features is None else features.shape[1]
        w0 = params[0]
        C1 = w0.shape[0]
        if w0.shape[1] != 3 + C0:
            raise RuntimeError('split first layer: the first weight must be (C1, 3 + feature width)')
        R = B * npoint * ns
        w0x = w0[:, :3].contiguous()
        w0f = feats = P = None
        if C0:
            w0f, feats = w0[:, 3:].contiguous(), features.contiguous()
            P = rows_gemm(feats, w0f)                                       # (B*N, C1), once per source point
        ws = [None] + [params[i].contiguous() for i in range(3, len(params), 3)]
        gammas = [params[i] for i in range(1, len(params), 3)]
        y0 = empty((R, C1), xyz)
        stats = empty((8, 2, C1), xyz)
        wsp = empty((max(_lib.lib().pdae_sa_first_forward_workspace(R, C1), 4),), xyz)
        _lib.call('pdae_sa_first_forward', xyz, B, N, npoint, ns, C0, C1, _lib.ptr(xyz), _lib.ptr(new_xyz), _lib.ptr(idx),
                  _lib.ptr(P), _lib.ptr(w0x), _lib.ptr(y0), _lib.ptr(stats), _lib.ptr(wsp))
        del P, wsp
        aff0 = bn_finalize(bns[0], R, xyz, partials=stats)
        out, arg, ys, affs = mlp_max_forward(y0, aff0[0], aff0[1], ws[1:], _batch_affine(bns[1:], R), ns)
        _save_level(ctx, [xyz, new_xyz, idx, feats, w0f], arg, out, ws, gammas, [y0] + ys, [aff0] + affs)
        ctx.dims = (B, N, npoint, ns, C0, C1)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, N, npoint, ns, C0, C1 = ctx.dims
        (xyz, new_xyz, idx, feats, w0f), arg, out, ws, gammas, ys, affs = _saved_level(ctx)
        d, grads = mlp_max_backward(dout, arg, out, ns, ys, affs, ws, gammas)
        # d is dy0: per source point and against the centred differences, then products on B*N rows
        R = B * npoint * ns
        dfeat = None
        dP = empty((B * N, C1), d) if C0 else None
        dw0x = empty((C1, 3), d)
        wsp = empty((max(_lib.lib().pdae_sa_first_backward_workspace(R, C1), 4),), d)
        _lib.call('pdae_sa_first_backward', d, B, N, npoint, ns, C0, C1, _lib.ptr(xyz), _lib.ptr(new_xyz),
                  _lib.ptr(idx), _lib.ptr(d), _lib.ptr(dP), _lib.ptr(dw0x), _lib.ptr(wsp))
        if C0:
            (dw0f,), _ = rows_wgrad([dP], [feats], [False])
            grads[0] = _hcat([(dw0x, 3), (dw0f, C0)], C1, d)
            if ctx.needs_input_grad[3]:
                dfeat = rows_gemm(dP, w0f, True)
        else:
            grads[0] = dw0x
        return (None, None, None, dfeat, None) + tuple(grads)


def split_first_mlp_max(xyz, new_xyz, idx, features, layers):
    """A level's shared MLP + max-pool with the first layer split by source point -> (B*np, C_last).  layers: the level's
    _ConvBN modules; the caller has asked split_first_supported."""
    params, bns = _level_params(layers)
    return SplitFirstMLPMaxFunction.apply(xyz, new_xyz, idx, features, bns, *params)


def group_rows_supported(N, npoint, ns, C):
    """Whether the grouping kernel and its gradient (_GroupRows) take a level's layout: mirrors the checks of
    sa_group_rows_grad in csrc/ball_group.hip (the feature width a multiple of 4, at most 1024; a cloud's sort lives in LDS)."""
    return C % 4 == 0 and C <= 1024 and N <= 4096 and 4 * (2 * N + 1 + npoint * ns) <= 150 * 1024


class _GroupRows(torch.autograd.Function):
    """QueryAndGroup in row layout (pointnet2_utils.py:345-361) as one kernel each way (csrc/ball_group.hip
    sa_group_rows*): rows [xyz - centre | 0 | features]; gradient to the features only (coordinates are inputs)."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, idx, features):
        B, N, _ = xyz.shape
        _, npoint, ns = idx.shape
        C = 0 if features is None else features.shape[1]
        out = torch.empty((B * npoint * ns, 4 + C), device=xyz.device, dtype=torch.float32)
        xyz, new_xyz, idx = xyz.contiguous(), new_xyz.contiguous(), idx.contiguous()
        feats = features.contiguous() if features is not None else None
        _lib.call('pdae_sa_group_rows', xyz, B, N, npoint, ns, C, _lib.ptr(xyz), _lib.ptr(new_xyz), _lib.ptr(idx),
                  _lib.ptr(feats), _lib.ptr(out))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, npoint, ns, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, N, npoint, ns, C = ctx.dims
        if C == 0 or not ctx.needs_input_grad[3]:
            return None, None, None, None
        dout = dout.contiguous()
        dfeat = torch.empty((B * N, C), device=dout.device, dtype=torch.float32)
        _lib.call('pdae_sa_group_rows_grad', dout, B, N, npoint, ns, C, _lib.ptr(idx), _lib.ptr(dout), _lib.ptr(dfeat))
        return None, None, None, dfeat


def group_rows(xyz, new_xyz, idx, features):
    """A grouped level's rows [xyz - centre | 0 | features] (K a multiple of 4): xyz (B,N,3), new_xyz (B,np,3), idx
    (B,np,ns) i32, features (B*N, C) rows or None -> (B*np*ns, 4 + C), by the kernel where it takes the layout, else by
    index_select / cat."""
    B, N, _ = xyz.shape
    _, npoint, ns = idx.shape
    if group_rows_supported(N, npoint, ns, 0 if features is None else features.shape[1]):
        return _GroupRows.apply(xyz, new_xyz, idx, features)
    flat = (idx.long() + torch.arange(B, device=xyz.device).view(B, 1, 1) * N).reshape(-1)
    g = xyz.reshape(B * N, 3).index_select(0, flat).reshape(B, npoint, ns, 3)
    g = (g - new_xyz.unsqueeze(2)).reshape(-1, 3)
    return all_rows(g, features.index_select(0, flat) if features is not None else None)


def all_rows(xyz_rows, features):
    """Coordinate rows (R, 3) and feature rows (R, C) or None -> [xyz | 0 | features] (R, 4 + C): the rows of a group-all
    level, which has every point once."""
    return torch.cat([xyz_rows, xyz_rows.new_zeros(xyz_rows.shape[0], 1)] + ([features] if features is not None else []),
                     dim=1)
