"""Fused patch embedder (mini-PointNet) of the Transformer DAE.

Computes Encoder.forward of the reference (models/PointCAE_transformer.py:37-51)

    f  = conv2(relu(bn1(conv1(x))))                     (R, 256)   R = B*G*32 points
    g  = max over each group's 32 points of f           (BG, 256)
    h3 = conv3(concat([g expanded, f]))                 (R, 512)
    t  = max over the group of conv4(relu(bn2(h3)))     (BG, C)

with the gfx950 kernels of csrc/gemm.hip and csrc/embed.hip instead of a chain of
cuDNN convs and separate BatchNorm / ReLU / max / concat / add passes:

  forward   conv2: BN1+ReLU applied while A is staged, epilogue stores f AND the
                   group max / argmax;
            conv3: the concat is never built -- the weight is split, the global
                   half is one small GEMM per group and enters as a per-group
                   bias; the epilogue accumulates BatchNorm's batch statistics;
            conv4: BN2+ReLU applied while A is staged, epilogue keeps only the
                   group max / argmax: the (R, C) product is never written.
  backward  max-pool / ReLU / BatchNorm backward are fused sweeps
            (group_max_scatter, bnrelu_backward, group_scatter_add), the last two
            folded into neighbouring kernels on the masked step (FOLD); weight
            gradients recompute the BN+ReLU activations in the GEMM producer;
            data-gradient GEMMs read the (out, in) weights as [K][N] operands on the row
            GEMM family (csrc/rows_gemm.hip): no transposed copies, no BLAS library.

Training-mode BatchNorm semantics are PyTorch's: biased batch variance for the
normalisation, unbiased for the running estimate, momentum 0.1.
"""
import os

import torch

from . import _lib
from .arena import arena
from .probe import probed, probed_family
from .rows import bn_eval_affine, bn_finalize, colsum, empty, gemm_bnstats, linear_any, rows_gemm, rows_wgrad, wgrad_listed


# (A/B: 0 = the small element-wise steps of the embedder as framework launches: 2 + 4 + 3 + 2 of them instead of 1 + 1 + 1 + 1)
GLUE = os.environ.get('PDAE_EMBED_GLUE', os.environ.get('PDAE_GLUE', '1')) != '0'

# (A/B: 0 = the embedder backward's three stand-alone sweeps as their own launches: BatchNorm-1's apply before the first conv's
#  weight gradient (a), group_sum_listed (b), group_scatter_add (c); 1 = folded into the neighbouring kernels; letters = those alone)
_fold = os.environ.get('PDAE_EMBED_FOLD', '1').lower()
FOLD = _fold != '0'
FOLD_PARTS = ''.join(c for c in 'abc' if c in _fold) or 'abc'


DEBUG_KEEP = None       # (lab) a dict: the backward keeps clones of its intermediates in it (tools/lab/model_nondet.py)


# Parity-test hook (None in production): called with what decides the embedder's backward -- the BatchNorm-ReLU inputs
# (rows y1 and h3 with the affine scale / shift: an entry passes where y * sc + sh > 0, as the kernels evaluate it) and
# the (groups, C) uint8 max-pool winners arg2, arg4 -- so a test can replay those decisions in the CPU oracle.
DECISION_HOOK = None


class PatchEmbedFunction(torch.autograd.Function):
    """points (R,3) + the 12 parameter tensors of Encoder -> tokens (R/32, C)."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, w3, b3, g2, be2, w4, b4, first_conv, second_conv, training,
                groups, masked=None):
        R = x.shape[0]
        BG = R // 32
        x = x.contiguous()
        w1m, w2m = w1.squeeze(-1), w2.squeeze(-1).contiguous()
        w3m, w4m = w3.squeeze(-1), w4.squeeze(-1).contiguous()
        c1, c2, c3, c4 = w1m.shape[0], w2m.shape[0], w3m.shape[0], w4m.shape[0]
        # conv1 (K = 3) + BN1 statistics
        if training:
            y1 = empty((R, c1), x)
            st1 = arena.take(4 * c1, x)[0].view(torch.float64)      # [2][c1] fp64 sums, pre-zeroed
            _lib.call('pdae_embed_conv1_stats', x, R, c1, _lib.ptr(x), _lib.ptr(w1m.contiguous()), _lib.ptr(b1),
                      _lib.ptr(y1), _lib.ptr(st1))
            sc1, sh1, mean1, is1 = bn_finalize(first_conv[1], R, x, stats64=st1)
        else:
            y1 = empty((R, c1), x)                                  # same kernel; its sums go unused in eval mode
            st1 = torch.zeros(2 * c1, dtype=torch.float64, device=x.device)
            _lib.call('pdae_embed_conv1_stats', x, R, c1, _lib.ptr(x), _lib.ptr(w1m.contiguous()), _lib.ptr(b1),
                      _lib.ptr(y1), _lib.ptr(st1))
            sc1, sh1, mean1, is1 = bn_eval_affine(first_conv[1])
        # conv2: BN1+ReLU producer, store f, group max
        f = empty((R, c2), x)
        g = empty((BG, c2), x)
        arg2 = empty((BG, c2), x, torch.uint8)
        # (the backward's masked-groups algebra wants the groups' row sums of f: the same epilogue leaves them)
        algebra = groups is not None and masked is not None and masked.numel() > 0 and training
        gsum = empty((BG, c2), x) if algebra and FOLD and 'b' in FOLD_PARTS and c2 % 4 == 0 else None
        if gsum is not None:
            probed_family('embed_gemm', 2.0 * R * c2 * c1, lambda: _lib.call(
                'pdae_embed_bnrelu_conv_store_groupmax_sum', x, R, c2, c1, _lib.ptr(y1), _lib.ptr(sc1),
                _lib.ptr(sh1), _lib.ptr(w2m), _lib.ptr(b2), _lib.ptr(f), _lib.ptr(g), _lib.ptr(arg2), _lib.ptr(gsum)))
        else:
            probed_family('embed_gemm', 2.0 * R * c2 * c1, lambda: _lib.call(
                'pdae_embed_bnrelu_conv_store_groupmax', x, R, c2, c1, _lib.ptr(y1), _lib.ptr(sc1),
                _lib.ptr(sh1), _lib.ptr(w2m), _lib.ptr(b2), _lib.ptr(f), _lib.ptr(g), _lib.ptr(arg2)))
        # conv3 on concat([g, f]): global half once per group, local half as the GEMM
        wlt = None
        if GLUE and w3m.shape[1] == 2 * c2 and w3m.is_contiguous():
            wg, wl = empty((c3, c2), x), empty((c3, c2), x)
            wlt = empty((c2, c3), x) if training else None         # (the backward's visible-rows data gradient reads wl^T)
            _lib.call('pdae_embed_split_conv3_weight', x, c3, c2, _lib.ptr(w3m), _lib.ptr(wg), _lib.ptr(wl), _lib.ptr(wlt))
        else:
            wg = w3m[:, :c2].contiguous()
            wl = w3m[:, c2:].contiguous()
        gb = rows_gemm(g, wg, False, b3)
        h3 = empty((R, c3), x)
        stats = empty((8, 2, c3), x)
        # the largest hand-written kernel of the step: bench.py's roofline kernel
        probed_family('embed_gemm', 2.0 * R * c3 * c2, lambda: probed(
            'patch_embed.second_conv[0] forward (group bias + BatchNorm statistics epilogue) %dx%dx%d' % (R, c3, c2),
            2.0 * R * c3 * c2,
            lambda: _lib.call('pdae_embed_conv_groupbias_stats', x, R, c3, c2, _lib.ptr(f), _lib.ptr(wl),
                              _lib.ptr(gb), _lib.ptr(h3), _lib.ptr(stats))))
        if training:
            sc2, sh2, mean2, is2 = bn_finalize(second_conv[1], R, x, partials=stats)
        else:
            sc2, sh2, mean2, is2 = bn_eval_affine(second_conv[1])
        # conv4: BN2+ReLU producer, only the group max leaves the kernel.  It comes after the
        # last BatchNorm, so it is evaluated only for the groups whose tokens are used
        # (`groups`: the visible patches; masked tokens are discarded by the caller).
        if groups is not None:
            Gv = groups.numel()
            inv = None
            if not algebra:          # the dense BatchNorm backward wants group -> position in the list
                inv = torch.full((BG,), -1, dtype=torch.int32, device=x.device)
                inv[groups.long()] = torch.arange(Gv, dtype=torch.int32, device=x.device)
        else:
            Gv, inv = BG, None
        Rv = Gv * 32
        tok = empty((Gv, c4), x)
        arg4 = empty((Gv, c4), x, torch.uint8)
        # the largest GEMM of the step: bench.py's roofline kernel
        probed_family('embed_gemm', 2.0 * Rv * c4 * c3, lambda: _lib.call(
            'pdae_embed_bnrelu_conv_groupmax', x, Rv, c4, c3, _lib.ptr(h3), _lib.ptr(sc2), _lib.ptr(sh2),
            _lib.ptr(w4m), _lib.ptr(b4), _lib.ptr(tok), _lib.ptr(arg4), _lib.ptr(groups)))
        if DECISION_HOOK is not None:
            DECISION_HOOK(dict(y1=y1, sc1=sc1, sh1=sh1, arg2=arg2, h3=h3, sc2=sc2, sh2=sh2, arg4=arg4))
        ctx.save_for_backward(x, y1, sc1, sh1, mean1, is1, f, g, arg2, h3, sc2, sh2, mean2, is2, arg4,
                              w1m, w2m, wg, wl, w4m, g1, g2, groups, inv)
        ctx.training, ctx.wlt = training, wlt
        # masked groups by algebra (backward): needs the complementary list and the per-group bias term
        ctx.algebra = algebra
        if ctx.algebra:
            ctx.masked, ctx.gb, ctx.gsum = masked.contiguous(), gb, gsum
        return tok

    @staticmethod
    def _masked_by_algebra(ctx, d3c, S2, f, h3, sc2, sh2, mean2, is2, g2, wl, groups, BG, wg=None, arg2=None):
        """conv3 + BatchNorm-2 backward with the masked groups handled by algebra.  A group whose token is
        dropped sends no activation gradient into BatchNorm-2, so on its rows the conv-output gradient is the
        correction alone, dh_r = u + v * h_r, with h_r = f_r W^T + gb_g (W = the local half of conv3's weight):
            df_r  = f_r (W^T diag(v) W) + (gb_g * v + u) W                       a 256x256 product, not 512x256
            dW    = dW_visible + diag(v) W Gram + xe^T fsum,   Gram = sum f_r^T f_r,  xe_g = u + v * gb_g
            dgb_g = v * (fsum_g W^T) + 32 xe_g,                                     fsum_g = sum_{r in g} f_r
        and the dense sweep + the two R x 512 x 256 GEMMs run on the visible rows only.  Same arithmetic error
        as the direct form (both 7e-7 of fp64 on a 32 k-row case).  -> dwl, dgb, df, dbeta2, dgamma2.
        fsum comes from the conv2 forward's epilogue when it left the group sums (ctx.gsum); with wg and arg2 the
        max-pool gradient dg = dgb wg is added to df where the two products store it (the lists partition the groups)."""
        x = f
        c3, c2 = wl.shape
        masked, gb = ctx.masked, ctx.gb
        Gv, Gm = groups.numel(), masked.numel()
        Rv, Rm, R = Gv * 32, Gm * 32, BG * 32
        uv, dgb = empty((2, c3), x), empty((BG, c3), x)
        # (S2: BatchNorm-2's sums, left by the GEMM that produced d3c)
        _lib.call('pdae_bnrelu_backward_listed_apply', x, BG, c3, _lib.ptr(d3c), _lib.ptr(h3), _lib.ptr(sc2), _lib.ptr(sh2),
                  _lib.ptr(mean2), _lib.ptr(is2), _lib.ptr(g2), _lib.ptr(S2), _lib.ptr(dgb), 1, _lib.ptr(uv), Gv,
                  _lib.ptr(groups))              # d3c <- dh of the visible rows; dgb[visible groups] <- their row sums
        u, v = uv[0], uv[1]
        fsum_m = empty((Gm, c2), x)
        gsum = ctx.gsum
        if gsum is None:
            _lib.call('pdae_group_sum_listed', x, Gm, c2, _lib.ptr(f), _lib.ptr(masked), _lib.ptr(fsum_m))
        elif not GLUE:
            fsum_m = gsum.index_select(0, masked.long())
        if GLUE:                                                      # xe and diag(v) W (and fsum_m = gsum[masked]), one launch
            xe, wv = empty((Gm, c3), x), empty((c3, c2), x)
            if gsum is None:
                _lib.call('pdae_embed_masked_prep', x, Gm, c3, c2, _lib.ptr(uv), _lib.ptr(gb), _lib.ptr(masked), _lib.ptr(wl),
                          _lib.ptr(xe), _lib.ptr(wv))
            else:
                _lib.call('pdae_embed_masked_prep_fsum', x, Gm, c3, c2, _lib.ptr(uv), _lib.ptr(gb), _lib.ptr(masked),
                          _lib.ptr(wl), _lib.ptr(xe), _lib.ptr(wv), _lib.ptr(gsum), _lib.ptr(fsum_m))
        else:
            xe = torch.addcmul(u, gb.index_select(0, masked.long()), v)   # u + v * gb_g  (Gm, 512)
            wv = wl * v.unsqueeze(1)
        # ---- weight gradient: dW_visible + diag(v) W Gram + xe^T fsum   (u (x) sum f rides in xe)
        dwl, _ = wgrad_listed(Rv, d3c, None, f, groups)
        gram, _ = wgrad_listed(Rm, f, masked, f, masked)
        wgram = rows_gemm(wl, gram)                                   # (Gram is symmetric)
        (xterm,), _ = rows_wgrad([xe], [fsum_m], [False])
        if GLUE:
            dwl = (dwl, v, wgram, xterm)                              # summed where conv3's gradient is assembled (backward)
        else:
            dwl.addcmul_(v.unsqueeze(1), wgram).add_(xterm)
        # ---- per-group sums of the masked groups (the global half of the split concat weight)
        hs = rows_gemm(fsum_m, wl)                                    # the group's summed conv output, bias term apart
        _lib.call('pdae_masked_group_sums', x, Gm, c3, _lib.ptr(hs), _lib.ptr(xe), _lib.ptr(v), _lib.ptr(masked),
                  _lib.ptr(dgb))
        # ---- data gradient
        (q,), _ = rows_wgrad([wv], [wl], [False])                     # W^T diag(v) W  (symmetric)
        e = rows_gemm(xe, wl, True)                                   # (gb_g * v + u) W   (Gm, 256)
        df = empty((R, c2), x)
        wlt = ctx.wlt if ctx.wlt is not None else wl.t().contiguous()
        scatter, pool = 'pdae_group_gemm_scatter', ()
        if wg is not None:
            dg = rows_gemm(dgb, wg, True)                             # (BG, 256) -> arg-max rows of f, added as df is stored
            scatter, pool = 'pdae_group_gemm_scatter_add', (_lib.ptr(dg), _lib.ptr(arg2))
        probed_family('embed_gemm', 2.0 * Rm * c2 * c2, lambda: _lib.call(
            scatter, x, Rm, c2, c2, _lib.ptr(f), _lib.ptr(masked), _lib.ptr(q), _lib.ptr(e),
            _lib.ptr(df), c2, _lib.ptr(masked), *pool))
        probed_family('embed_gemm', 2.0 * Rv * c2 * c3, lambda: _lib.call(
            scatter, x, Rv, c2, c3, _lib.ptr(d3c), None, _lib.ptr(wlt), None,
            _lib.ptr(df), c2, _lib.ptr(groups), *pool))
        return dwl, dgb, df, S2[0], S2[1]

    @staticmethod
    def _eval_input_grad(ctx, dtok):
        """The eval-mode, data-only backward: d tokens -> dx (R, 3), no parameter gradient.  On its running estimates a
        BatchNorm is a per-channel affine map, so its backward is the scale alone, folded into the rows of the weight the
        gradient meets next (tiny products on weights: sc2 into the two halves of conv3's, sc1 into conv1's); the ReLU
        masks come out of the same transposed-weight row GEMMs the training backward uses (their BatchNorm sums go
        unread), and the last step is the 128 -> 3 contraction of csrc/input_grad.hip."""
        (x, y1, sc1, sh1, mean1, is1, f, g, arg2, h3, sc2, sh2, mean2, is2, arg4,
         w1m, w2m, wg, wl, w4m, g1, g2, groups, inv) = ctx.saved_tensors
        R, BG = x.shape[0], x.shape[0] // 32
        c2, c4 = w2m.shape[0], w4m.shape[0]
        if groups is not None:
            raise NotImplementedError('patch embedder: the eval-mode input gradient covers every group (no group list)')
        dtok = dtok.contiguous()
        dy4 = empty((R, c4), x)
        _lib.call('pdae_group_max_scatter', x, BG, c4, _lib.ptr(dtok), _lib.ptr(arg4), _lib.ptr(dy4))
        d3, _ = gemm_bnstats(dy4, w4m, h3, None, sc2, sh2, mean2, is2)        # (R, 512): d relu(bn2(h3)), ReLU-masked
        del dy4
        wls, wgs = wl * sc2.unsqueeze(1), wg * sc2.unsqueeze(1)               # diag(sc2) W: BatchNorm-2's backward
        df = rows_gemm(d3, wls, True)                                         # (R, 256), the local half
        dgb = empty((BG, d3.shape[1]), x)
        _lib.call('pdae_group_sum_listed', x, BG, d3.shape[1], _lib.ptr(d3), None, _lib.ptr(dgb))
        del d3
        dg = rows_gemm(dgb, wgs, True)                                        # (BG, 256) -> the arg-max rows of f
        _lib.call('pdae_group_scatter_add', x, BG, c2, _lib.ptr(dg), _lib.ptr(arg2), _lib.ptr(df))
        d1, _ = gemm_bnstats(df, w2m, y1, None, sc1, sh1, mean1, is1)         # (R, 128): d relu(bn1(y1)), ReLU-masked
        del df
        w1s = (w1m * sc1.unsqueeze(1)).contiguous()                           # (128, 3): BatchNorm-1's backward
        dx = empty((R, 3), x)
        _lib.call('pdae_rows_contract3', x, R, d1.shape[1], _lib.ptr(d1), _lib.ptr(w1s), None, R, _lib.ptr(dx))
        return (dx,) + (None,) * 17

    @staticmethod
    def backward(ctx, dtok):
        if not ctx.training:
            if ctx.needs_input_grad[0] and not any(ctx.needs_input_grad[1:13]):
                return PatchEmbedFunction._eval_input_grad(ctx, dtok)
            raise NotImplementedError('patch embedder backward is implemented for training-mode BatchNorm')
        (x, y1, sc1, sh1, mean1, is1, f, g, arg2, h3, sc2, sh2, mean2, is2, arg4,
         w1m, w2m, wg, wl, w4m, g1, g2, groups, inv) = ctx.saved_tensors
        R, BG = x.shape[0], x.shape[0] // 32
        c1, c2, c3, c4 = w1m.shape[0], w2m.shape[0], wl.shape[0], w4m.shape[0]
        dtok = dtok.contiguous()
        Gv = dtok.shape[0]                                        # groups that went through conv4
        Rv = Gv * 32
        # ---- conv4 + max-pool (compact: only the listed groups carry gradient)
        dy4 = empty((Rv, c4), x)
        _lib.call('pdae_group_max_scatter', x, Gv, c4, _lib.ptr(dtok), _lib.ptr(arg4), _lib.ptr(dy4))
        db4 = colsum(dtok)
        dw4, _ = wgrad_listed(Rv, dy4, None, h3, groups, sc2, sh2)
        # (Rv, 512) grad of relu(bn2(h3)) rows, ReLU-masked, + BatchNorm-2's sums out of the same launch
        d3c, S2 = gemm_bnstats(dy4, w4m, h3, groups, sc2, sh2, mean2, is2)
        del dy4
        pooled = ctx.algebra and FOLD and 'c' in FOLD_PARTS                           # the max-pool gradient rides in df's two products
        if ctx.algebra:
            dwl, dgb, df, dbe2, dg2 = PatchEmbedFunction._masked_by_algebra(
                ctx, d3c, S2, f, h3, sc2, sh2, mean2, is2, g2, wl, groups, BG, *((wg, arg2) if pooled else ()))
            del d3c
        else:
            # ---- ReLU + BN2 backward + per-group sums for the global half
            dgb = empty((BG, c3), x)
            d3 = empty((R, c3), x) if groups is not None else d3c
            _lib.call('pdae_bnrelu_backward_apply', x, BG, c3, _lib.ptr(d3c), _lib.ptr(h3), _lib.ptr(sc2), _lib.ptr(sh2),
                      _lib.ptr(mean2), _lib.ptr(is2), _lib.ptr(g2), _lib.ptr(S2), _lib.ptr(dgb), Gv,
                      _lib.ptr(groups), _lib.ptr(inv), _lib.ptr(d3) if groups is not None else None)
            del d3c
            dbe2, dg2 = S2[0], S2[1]
            # ---- conv3 (split weight)
            (dwl,), _ = rows_wgrad([d3], [f], [False])                # stream-K grouped kernel, ordered reduction (no atomics)
            df = rows_gemm(d3, wl, True)                              # (R, 256)
            del d3
        (dwg,), _ = rows_wgrad([dgb], [g], [False])
        # conv3's bias feeds a training-mode BatchNorm: its gradient, sum_r dy3_r, is EXACTLY zero (BatchNorm's
        # backward removes the batch mean of the gradient); the column-sum pass over dgb would only measure
        # its own rounding (the reference's value is ~1e-6 of the other gradients, noise of either sign)
        db3 = arena.take(c3, x)[0]
        if GLUE and c2 % 4 == 0:
            parts = dwl if isinstance(dwl, tuple) else (dwl, None, None, None)
            dw3 = empty((c3, 2 * c2, 1), x)
            _lib.call('pdae_embed_dw3_assemble', x, c3, c2, _lib.ptr(dwg), *[_lib.ptr(t) for t in parts], _lib.ptr(dw3))
        else:
            if isinstance(dwl, tuple):
                dwl = dwl[0].addcmul_(dwl[1].unsqueeze(1), dwl[2]).add_(dwl[3])
            dw3 = torch.cat([dwg, dwl], dim=1).unsqueeze(-1)
        if not pooled:
            dg = rows_gemm(dgb, wg, True)                         # (BG, 256) -> arg-max rows of f
            _lib.call('pdae_group_scatter_add', x, BG, c2, _lib.ptr(dg), _lib.ptr(arg2), _lib.ptr(df))
        # ---- conv2
        dw2, db2 = wgrad_listed(R, df, None, y1, None, sc1, sh1, bias=True)    # db2: column sums of df, same kernel
        d1, S1 = gemm_bnstats(df, w2m, y1, None, sc1, sh1, mean1, is1)      # (R, 128), ReLU-masked, + BatchNorm-1's sums
        if DEBUG_KEEP is not None:
            DEBUG_KEEP.update(df=df.clone(), d1_pre=d1.clone(), dw2=dw2.clone(), y1=y1.clone())
        del df
        # ---- ReLU + BN1 backward, conv1 (K = 3)
        dbe1, dg1 = S1[0], S1[1]
        part1 = empty((_lib.lib().pdae_embed_conv1_backward_weight_parts(R), 3, c1), x)
        if FOLD and 'a' in FOLD_PARTS and DEBUG_KEEP is None:         # one pass: d1's BatchNorm-1 backward feeds the weight gradient unstored
            _lib.call('pdae_embed_bnrelu_backward_conv1_weight', x, R, c1, _lib.ptr(d1), _lib.ptr(y1), _lib.ptr(sc1),
                      _lib.ptr(sh1), _lib.ptr(mean1), _lib.ptr(is1), _lib.ptr(g1), _lib.ptr(S1), _lib.ptr(x), _lib.ptr(part1))
        else:
            _lib.call('pdae_bnrelu_backward_apply', x, BG, c1, _lib.ptr(d1), _lib.ptr(y1), _lib.ptr(sc1), _lib.ptr(sh1),
                      _lib.ptr(mean1), _lib.ptr(is1), _lib.ptr(g1), _lib.ptr(S1), None, BG, None, None, None)
            _lib.call('pdae_embed_conv1_backward_weight', x, R, c1, _lib.ptr(d1), _lib.ptr(x), _lib.ptr(part1))
        if GLUE:                                                      # (c1, 3, 1): one pass over d1, ordered partials
            dw1 = empty((c1, 3, 1), x)
            _lib.call('pdae_partials_sum_t', x, part1.shape[0], 3, c1, _lib.ptr(part1), _lib.ptr(dw1))
        else:
            dw1 = part1.sum(0).t().unsqueeze(-1)
        if DEBUG_KEEP is not None:
            DEBUG_KEEP.update(d1_post=d1.clone(), part1=part1.clone(), dw1=dw1.clone(), x=x.clone(), S1=S1.clone())
        db1 = arena.take(c1, x)[0]                                   # exactly zero, as db3 (saves a 134 MB pass)
        return (None, dw1, db1, dg1, dbe1, dw2.unsqueeze(-1), db2, dw3, db3, dg2, dbe2,
                dw4.unsqueeze(-1), db4, None, None, None, None, None)


def patch_embed(points, first_conv, second_conv, training, groups=None, masked=None):
    """points (BG, n=32, 3) -> tokens (BG, C), or -- with `groups`, an int32 device
    tensor of group ids -- the tokens of just those groups (len(groups), C) in list
    order; BatchNorm statistics always cover all BG groups.  masked: the complementary
    list (the groups whose tokens the caller drops): their share of the backward is then
    done by algebra (PatchEmbedFunction._masked_by_algebra)."""
    BG, n, _ = points.shape
    if points.requires_grad and torch.is_grad_enabled():
        # input-point gradients: the fused path's eval-mode data-only backward (PatchEmbedFunction._eval_input_grad)
        if n != 32:
            raise NotImplementedError('patch embedder: a gradient with respect to the points needs group_size == 32 '
                                      '(the fused path), got %d' % n)
        if isinstance(first_conv[1], torch.nn.SyncBatchNorm) or isinstance(second_conv[1], torch.nn.SyncBatchNorm):
            raise NotImplementedError('patch embedder: a gradient with respect to the points is not implemented under '
                                      'SyncBatchNorm (the fused path keeps plain BatchNorm1d)')
    if n != 32:
        # the fused kernels tile a patch as one 32-row MFMA tile; other group sizes of the reference's YAML grid
        # (16, 64) take the layer-by-layer path on the same row GEMMs
        return patch_embed_layerwise(points, first_conv, second_conv, groups)
    if isinstance(first_conv[1], torch.nn.SyncBatchNorm) or isinstance(second_conv[1], torch.nn.SyncBatchNorm):
        # --sync_bn (runner_pretrain.py:81-83, off in every shipped config): batch statistics over ALL replicas.
        # The fused kernels keep BatchNorm's sums on the device of one replica, so this flag takes the layer-by-layer
        # path: the same row GEMMs, torch's SyncBatchNorm modules (which own the collectives) in between.
        return patch_embed_layerwise(points, first_conv, second_conv, groups)
    return PatchEmbedFunction.apply(
        points.reshape(BG * n, 3), first_conv[0].weight, first_conv[0].bias, first_conv[1].weight,
        first_conv[1].bias, first_conv[3].weight, first_conv[3].bias, second_conv[0].weight,
        second_conv[0].bias, second_conv[1].weight, second_conv[1].bias, second_conv[3].weight,
        second_conv[3].bias, first_conv, second_conv, training, groups, masked)


def patch_embed_layerwise(points, first_conv, second_conv, groups=None):
    """Encoder.forward (models/PointCAE_transformer.py:37-51) layer by layer on the row GEMMs, calling the
    BatchNorm MODULES as they are -- which is what lets nn.SyncBatchNorm (collective C4 of SURVEY 2.2) compute its
    statistics across the replicas.  Slower than the fused path (every intermediate is materialised); used only under
    --sync_bn and, from Encoder.forward, when a gradient is required through BatchNorms in eval mode (the frozen encoder
    of optimizer.part only_new).  The last conv + max-pool run on the listed groups only, like the fused path."""
    BG, n, _ = points.shape
    R = BG * n
    y = linear_any(points.reshape(R, 3), first_conv[0].weight.squeeze(-1), first_conv[0].bias)
    z1 = first_conv[1](y)
    y = torch.relu(z1)
    f = linear_any(y, first_conv[3].weight.squeeze(-1), first_conv[3].bias)
    C2 = f.shape[1]
    g, arg2 = f.view(BG, n, C2).max(dim=1, keepdim=True)
    cat = torch.cat([g.expand(-1, n, -1), f.view(BG, n, C2)], dim=2).reshape(R, 2 * C2)
    h = linear_any(cat, second_conv[0].weight.squeeze(-1), second_conv[0].bias)
    z3 = second_conv[1](h)
    h = torch.relu(z3)
    if groups is not None:
        h = h.view(BG, n, -1).index_select(0, groups.long()).reshape(-1, h.shape[1])
    t = linear_any(h, second_conv[3].weight.squeeze(-1), second_conv[3].bias)
    t, arg4 = t.view(-1, n, t.shape[1]).max(dim=1)
    if DECISION_HOOK is not None:             # the BatchNorm outputs stand in for (rows, scale, shift): scale 1, shift 0
        one, zero = (lambda c: torch.ones(c, device=t.device)), (lambda c: torch.zeros(c, device=t.device))
        DECISION_HOOK(dict(y1=z1, sc1=one(z1.shape[1]), sh1=zero(z1.shape[1]), arg2=arg2.squeeze(1).to(torch.uint8),
                           h3=z3, sc2=one(z3.shape[1]), sh2=zero(z3.shape[1]), arg4=arg4.to(torch.uint8)))
    return t
