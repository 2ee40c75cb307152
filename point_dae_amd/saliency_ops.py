"""Input-point gradients of a fine-tuned classifier: the saliency maps of tools/runner_finetune.py:751-833
(vis_saliency_map) of the reference, which differentiates `logits[0, label]` with framework autograd one cloud at a time.

In eval mode the clouds of a batch are independent (every BatchNorm runs on its running estimates), so a batch is one
eval forward of B clouds and ONE data-only backward down to (B, N, 3):

    logits, grad = input_gradients(model, points, labels, score='logit')

score 'logit' seeds the backward with one_hot(labels) (the reference's live line); 'loss' with each cloud's own
cross-entropy (the batch-mean loss times B: the reference's commented alternative).

PDAE_SALIENCY=hip (default) is the model's own chain: grouping (csrc/input_grad.hip group_points_backward), the position
embedding (rows_contract3), the eval-mode patch embedder (patch_embed.PatchEmbedFunction._eval_input_grad), the blocks
and the head with their weight gradients skipped (rows.SKIP_FROZEN_WGRAD).  PDAE_SALIENCY=torch restates the three links
that end at coordinates as framework ops under framework autograd -- the neighbourhoods and centres by indexing with the
FPS / kNN kernels' indices, the embedder's four convs, BatchNorms and max-pools (at the product's own ReLU and max-pool
decisions, patch_embed.DECISION_HOOK), torch Linear / GELU for the position embedding -- around the same forward: the
tokens and the position embedding keep the kernels' VALUES, so both backends return the same logits bit for bit, and
only the gradient's path differs.  It is the timing baseline (tools/bench_saliency.py).
"""
import os

import torch

from . import nn_ops
from .arena import begin_step

SCORES = ('logit', 'loss')


def backend():
    """'hip' or 'torch', from PDAE_SALIENCY."""
    name = os.environ.get('PDAE_SALIENCY', 'hip').lower()
    if name not in ('hip', 'torch'):
        raise ValueError('PDAE_SALIENCY=%r: hip or torch' % name)
    return name


class _ValuesOf(torch.autograd.Function):
    """The values of `value` with the gradient path of `carrier` (same shape): the forward hands on the kernels' bits,
    the backward flows into the framework restatement."""

    @staticmethod
    def forward(ctx, value, carrier):
        return value.view_as(value)

    @staticmethod
    def backward(ctx, g):
        return None, g


def _embed_torch(enc, nb, d):
    """Encoder.forward (models/PointCAE_transformer.py:37-51) on (BG, n, 3) patches as framework ops, eval-mode BatchNorm
    modules included, with the ReLUs and max-pools taken where the product's kernels took them (d: DECISION_HOOK's dict).
    The R = BG n points go through the 1x1 convs as ONE sample of length R: one GEMM per conv."""
    BG, n, _ = nb.shape
    fc, sc = enc.first_conv, enc.second_conv

    def mask(y, scale, shift):                                               # (R, C) rows -> (1, C, R)
        return ((y * scale + shift) > 0).t().unsqueeze(0)

    def pool(f, arg):                                                        # (1, C, R) -> (C, BG, 1) at the winners
        return f.view(f.shape[1], BG, n).gather(2, arg.long().t().unsqueeze(-1))

    # (the framework's own GEMM-backed convolution: the vendor library's first-use kernel search would dominate a short run)
    with torch.backends.cudnn.flags(enabled=False):
        x = nb.reshape(BG * n, 3).t().unsqueeze(0)                           # (1, 3, R)
        h = fc[1](fc[0](x)) * mask(d['y1'], d['sc1'], d['sh1'])
        f = fc[3](h)                                                         # (1, 256, R)
        fg = pool(f, d['arg2']).expand(-1, -1, n).reshape(1, f.shape[1], BG * n)
        h = sc[1](sc[0](torch.cat([fg, f], dim=1))) * mask(d['h3'], d['sc2'], d['sh2'])
        return pool(sc[3](h), d['arg4']).squeeze(-1).t()                     # (BG, C)


def _forward_hip(model, pts):
    return model(pts)


def _forward_torch(model, pts):
    from . import patch_embed
    if not hasattr(model, 'trunk_from_tokens'):
        raise NotImplementedError('PDAE_SALIENCY=torch restates the PointTransformer family only')
    B = pts.shape[0]
    G, k, C = model.num_group, model.group_size, model.trans_dim
    begin_step(pts.device)
    seen, idx = [], {}
    outer, patch_embed.DECISION_HOOK = patch_embed.DECISION_HOOK, seen.append
    try:
        with torch.no_grad():                                               # the forward both backends share
            nb_h, ctr_h = model.group_divider(pts.detach(), idx)
            tok_h = model.encoder(nb_h)
            pos_h = nn_ops.pos_embed(ctr_h.reshape(B * G, 3), model.pos_embed).reshape(B, G, C)
    finally:
        patch_embed.DECISION_HOOK = outer
    if outer is not None:
        outer(seen[0])
    fps_idx, knn_idx = idx['fps_idx'].long(), idx['knn_idx']
    ctr = torch.gather(pts, 1, fps_idx.unsqueeze(-1).expand(-1, -1, 3))                                   # xyz[fps]
    nb = torch.gather(pts, 1, knn_idx.reshape(B, G * k, 1).expand(-1, -1, 3)).view(B, G, k, 3) - ctr.unsqueeze(2)
    tok_t = _embed_torch(model.encoder, nb.reshape(B * G, k, 3), seen[0]).view(B, G, C)
    pos_t = model.pos_embed(ctr)                                            # torch Linear -> GELU -> Linear
    tokens, pos = _ValuesOf.apply(tok_h, tok_t), _ValuesOf.apply(pos_h, pos_t)
    return model.head(model.trunk_from_tokens(tokens, pos))


def input_gradients(model, points, labels, score='logit'):
    """points (B, N, 3+) on the GPU, labels (B,) -> (logits (B, K), grad (B, N, 3)): the eval-mode logits and the
    gradient of every cloud's score with respect to its own points.  One forward, one backward.  The model is put in
    eval mode and, for the call, every parameter is frozen (no parameter gradient is computed or left behind); both are
    put back afterwards."""
    if score not in SCORES:
        raise ValueError('score %r: one of %s' % (score, ', '.join(SCORES)))
    if not getattr(model, 'input_grad_supported', False):
        raise NotImplementedError('%s.input_grad_supported is False: its backward carries no gradient down to the '
                                  'input points' % type(model).__name__)
    if not points.is_cuda:
        raise RuntimeError('input_gradients: points must be on the GPU (there is no CPU path)')
    forward = _forward_torch if backend() == 'torch' else _forward_hip
    modes = [(m, m.training) for m in model.modules()]     # (a runner may have frozen single BatchNorms)
    live = [p for p in model.parameters() if p.requires_grad]
    model.eval()
    for p in live:
        p.requires_grad_(False)
    try:
        pts = points.detach()[:, :, :3].contiguous().requires_grad_()
        labels = labels.view(-1).long()
        with torch.enable_grad():
            logits = forward(model, pts)
            if score == 'logit':
                seed = torch.zeros_like(logits).scatter_(1, labels.unsqueeze(1), 1.0)
                logits.backward(seed)
            else:
                loss, _ = model.get_loss_acc(logits, labels)
                (loss * float(pts.shape[0])).backward()
        return logits.detach(), pts.grad
    finally:
        for p in live:
            p.requires_grad_(True)
        for m, mode in modes:
            m.training = mode
