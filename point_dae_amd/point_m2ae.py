"""Point-M2AE's hierarchical encoder as a frozen feature extractor, MI355X host side (models/Point_M2AE.py:1079-1169
Point_M2AE_SVMFeature, :17-180 H_Encoder with eval=True; models/Point_M2AE_modules.py:169-216 Token_Embed, :269-343
Attention / Block / Encoder_Block of the reference).

Same parameter and buffer names as the reference, so a Point-M2AE pretraining checkpoint loads through
builder.remap_pretrain_keys with strict=False (its decoder keys unexpected, nothing missing):

    model = MODELS.build(cfg.model)              # cfg.model.NAME == 'Point_M2AE_SVMFeature'
    model.load_model_from_ckpt(path_or_None)
    feature = model.eval()(points)               # (B, encoder_dims[-1]): what --svm_classification fits its SVMs on

Forward only, evaluation mode only, no CPU path.  Per level: the token embedder (level 0: Token_Embed(3 -> C) on
patches of 4..32 points with the second_conv products kept on chip, csrc/m2ae.hip embed_tail; level i > 0: token
merging, whose pointwise layers run once per SOURCE token before the gather -- exact algebra in evaluation mode, G_{i-1}
rows instead of G_i k_i), the compaction of each sample's visible tokens to the front of a zero-padded buffer, the
position embedding, and depth_i pre-LN blocks on the row GEMMs and LayerNorm kernels of the flat Transformer around
the masked attention core pdae_attention_local_forward, which evaluates the padding-and-radius mask from the centres.
BatchNorm runs on its running statistics, folded into the weights next to it.  One host read per level and batch sizes
the padded buffer (T_pad = the batch's longest visible sequence).

A sample's feature depends on its batch through T_pad, as in the reference: a query whose centre lies within the
level's radius of the origin attends to the batch's padded rows.  Unlike the reference the
radius mask of a level always comes from that level's own centres.
"""
import torch
import torch.nn as nn

from . import _lib, nn_ops
from .classifier import Classifier
from .point_cae_transformer import Block
from .point_m2ae_group import Group, multi_scale_mask
from .registry import MODELS
from .rows import bn_eval_affine, empty, linear_any, rows_gemm

MAX_TOKENS = 512           # pdae_attention_local_forward takes T <= 512 tokens per cloud
HEAD_DIMS = (16, 32, 64)


class Token_Embed(nn.Module):
    """Point_M2AE_modules.py:169-216 in the reference's Sequential layout; the forward is token_embed_points (in_c == 3)
    or token_embed_merge."""

    def __init__(self, in_c, out_c):
        super().__init__()
        self.in_c, self.out_c = in_c, out_c
        if in_c == 3:
            self.first_conv = nn.Sequential(nn.Conv1d(in_c, 128, 1), nn.BatchNorm1d(128), nn.ReLU(inplace=True),
                                            nn.Conv1d(128, 256, 1))
            self.second_conv = nn.Sequential(nn.Conv1d(512, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                             nn.Conv1d(512, out_c, 1))
        else:
            self.first_conv = nn.Sequential(nn.Conv1d(in_c, in_c, 1), nn.BatchNorm1d(in_c), nn.ReLU(inplace=True),
                                            nn.Conv1d(in_c, in_c, 1))
            self.second_conv = nn.Sequential(nn.Conv1d(in_c * 2, out_c, 1), nn.BatchNorm1d(out_c), nn.ReLU(inplace=True),
                                             nn.Conv1d(out_c, out_c, 1))


class Encoder_Block(nn.Module):
    """Point_M2AE_modules.py:328-343: `depth` pre-LN blocks, each fed x + pos."""

    def __init__(self, embed_dim, depth, num_heads, drop_path_rate):
        super().__init__()
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, drop_path_rate[i]) for i in range(depth)])


def _folded(conv, bn):
    """conv (kernel 1) followed by an eval-mode BatchNorm as one affine layer -> (weight (out, in), bias (out,))."""
    scale, shift, _, _ = bn_eval_affine(bn)
    w = conv.weight.squeeze(-1) * scale.unsqueeze(1)
    b = conv.bias * scale + shift if conv.bias is not None else shift
    return w.contiguous(), b.contiguous()


def group_max(x, P, n):
    """x (P*n, C) -> the max over each patch's n consecutive rows (P, C)."""
    out = empty((P, x.shape[1]), x)
    _lib.call('pdae_m2ae_group_max', x, P, n, x.shape[1], _lib.ptr(x), _lib.ptr(out))
    return out


def embed_tail(f, n, wl, gb, w4, b4):
    """max over each patch's n rows of relu(f wl^T + gb[patch]) w4^T, + b4 -> (R / n, N4); nothing else is stored."""
    R, K = f.shape
    tok = empty((R // n, w4.shape[0]), f)
    _lib.call('pdae_m2ae_embed_tail', f, R, n, K, wl.shape[0], w4.shape[0], _lib.ptr(f), _lib.ptr(wl), _lib.ptr(gb),
              _lib.ptr(w4), _lib.ptr(b4), _lib.ptr(tok))
    return tok


def token_embed_points(te, patches):
    """Token_Embed(3 -> C) in evaluation mode on patches (P, n, 3) -> tokens (P, C).  The concat of :213 is never
    built (the weight is split, the global half enters as a per-patch term) and second_conv's (R, 512) and (R, C)
    products are never stored: only the patch maxima leave pdae_m2ae_embed_tail."""
    P, n, _ = patches.shape
    w1, b1 = _folded(te.first_conv[0], te.first_conv[1])
    y = linear_any(patches.reshape(P * n, 3), w1, b1, relu=True)                          # (R, 128)
    f = rows_gemm(y, te.first_conv[3].weight.squeeze(-1), False, te.first_conv[3].bias)   # (R, 256)
    del y
    c2 = f.shape[1]
    g = group_max(f, P, n)
    w3, b3 = _folded(te.second_conv[0], te.second_conv[1])
    gb = rows_gemm(g, w3[:, :c2].contiguous(), False, b3)                                 # (P, 512)
    return embed_tail(f, n, w3[:, c2:].contiguous(), gb, te.second_conv[3].weight.squeeze(-1).contiguous(),
                      te.second_conv[3].bias)


def token_embed_merge(te, table, idx, P, k):
    """Token merging (Point_M2AE.py:132) + Token_Embed(C_in -> C_out) in evaluation mode: table (S, C_in) source
    tokens, idx (P*k,) int64 flat source rows of every patch member -> tokens (P, C_out).  Everything before the
    first max is pointwise per source row, so first_conv and the local half of second_conv[0] run once per source
    token; the gather-max, the per-patch global half, the add + ReLU and the last conv with its max run per member."""
    w1, b1 = _folded(te.first_conv[0], te.first_conv[1])
    y = rows_gemm(table, w1, False, b1, 1)
    f = rows_gemm(y, te.first_conv[3].weight.squeeze(-1), False, te.first_conv[3].bias)   # (S, C_in)
    c_in = f.shape[1]
    w3, b3 = _folded(te.second_conv[0], te.second_conv[1])
    u = rows_gemm(f, w3[:, c_in:].contiguous())                                           # (S, C_out), the local half
    g = empty((P, c_in), f)
    _lib.call('pdae_m2ae_gather_max', f, P, k, c_in, _lib.ptr(f), _lib.ptr(idx), _lib.ptr(g))
    gb = rows_gemm(g, w3[:, :c_in].contiguous(), False, b3)                               # (P, C_out)
    h = empty((P * k, u.shape[1]), f)
    _lib.call('pdae_m2ae_gather_add_relu', f, P, k, u.shape[1], _lib.ptr(u), _lib.ptr(idx), _lib.ptr(gb), _lib.ptr(h))
    t = rows_gemm(h, te.second_conv[3].weight.squeeze(-1), False, te.second_conv[3].bias)
    return group_max(t, P, k)


def attention_local(qkv, centres, lens, B, T, H, scale, radius):
    """softmax(q k^T * scale + mask * -100000) v per (sample, head) on qkv rows (B*T, 3*H*D), the padding-and-radius
    mask of H_Encoder.forward (:144-163) evaluated from centres (B*T, 3; padded rows zero) and lens (B,) int32."""
    D = qkv.shape[1] // (3 * H)
    o = empty((B * T, H * D), qkv)
    _lib.call('pdae_attention_local_forward', qkv, B, T, H, D, float(scale), float(radius), _lib.ptr(qkv),
              _lib.ptr(centres), _lib.ptr(lens), _lib.ptr(o))
    return o


def compact_visible(masked):
    """masked (B, G) bool / uint8 -> (lens (B,) int32, ids (B, G) int32: the visible tokens ascending, -1 behind)."""
    B, G = masked.shape
    m8 = masked.to(torch.uint8).contiguous()
    lens = torch.empty(B, dtype=torch.int32, device=m8.device)
    ids = torch.empty((B, G), dtype=torch.int32, device=m8.device)
    _lib.call('pdae_m2ae_compact', m8, B, G, _lib.ptr(m8), _lib.ptr(lens), _lib.ptr(ids))
    return lens, ids


def block_forward(blk, x, pos, B, T, centres, lens, radius):
    """One pre-LN block on x + pos without autograd state.  x: rows (B*T, C) or an nn_ops.Pending -> nn_ops.Pending."""
    attn, mlp = blk.attn, blk.mlp
    if isinstance(x, nn_ops.Pending):
        x1, n1, _, _ = nn_ops._res_ln_forward(x.a, x.bias, None, x.res, pos, blk.norm1.weight, blk.norm1.bias,
                                              blk.norm1.eps, T)
    else:
        x1, n1, _, _ = nn_ops._add_ln_forward(x, pos, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
    qkv = rows_gemm(n1, attn.qkv.weight)
    o = attention_local(qkv, centres, lens, B, T, attn.num_heads, attn.scale, radius)
    a1 = rows_gemm(o, attn.proj.weight, may_split=True)
    x2, n2, _, _ = nn_ops._res_ln_forward(a1, attn.proj.bias, None, x1, None, blk.norm2.weight, blk.norm2.bias,
                                          blk.norm2.eps, T)
    gp = empty((n2.shape[0], mlp.fc1.weight.shape[0]), n2)
    h = rows_gemm(n2, mlp.fc1.weight, False, mlp.fc1.bias, 2, gp)
    a2 = rows_gemm(h, mlp.fc2.weight, may_split=True)
    return nn_ops.Pending(a2, mlp.fc2.bias, None, x2, T)


class H_Encoder(nn.Module):
    """Point_M2AE.py:17-180, the eval=True branch of its forward."""

    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.mask_ratio = config.mask_ratio
        self.encoder_depths = list(config.encoder_depths)
        self.encoder_dims = list(config.encoder_dims)
        self.local_radius = list(config.local_radius)
        self.num_heads = config.num_heads
        self.token_embed = nn.ModuleList()
        self.encoder_pos_embeds = nn.ModuleList()
        for i, dim in enumerate(self.encoder_dims):
            if dim % self.num_heads or dim // self.num_heads not in HEAD_DIMS:
                raise NotImplementedError('H_Encoder: head dim %s / %d; the masked attention core takes %s'
                                          % (dim, self.num_heads, (HEAD_DIMS,)))
            self.token_embed.append(Token_Embed(3 if i == 0 else self.encoder_dims[i - 1], dim))
            self.encoder_pos_embeds.append(nn.Sequential(nn.Linear(3, dim), nn.GELU(), nn.Linear(dim, dim)))
        dpr = [x.item() for x in torch.linspace(0, config.drop_path_rate, sum(self.encoder_depths))]
        self.encoder_blocks = nn.ModuleList()
        count = 0
        for dim, depth in zip(self.encoder_dims, self.encoder_depths):
            self.encoder_blocks.append(Encoder_Block(dim, depth, self.num_heads, dpr[count:count + depth]))
            count += depth
        self.encoder_norms = nn.ModuleList(nn.LayerNorm(dim) for dim in self.encoder_dims)
        self.apply(Classifier._init_weights)

    @torch.no_grad()
    def forward(self, neighborhoods, centers, idxs, eval=True, capture=None):
        """The grouping of point_m2ae_group.HierarchicalGroup -> the last level's normed tokens (B, T_pad, C).
        capture: a dict that receives, per level, lens (B,), T_pad and the valid output rows before the norm."""
        if not eval or self.training:
            raise NotImplementedError('H_Encoder: evaluation mode only (masked pretraining of Point-M2AE is not built)')
        levels = len(centers)
        B = centers[0].shape[0]
        top = torch.zeros((B, centers[-1].shape[1]), dtype=torch.bool, device=centers[0].device)     # :102-105: no mask
        masks = multi_scale_mask(top, idxs, centers)
        for i in range(levels):
            G, C = centers[i].shape[1], self.encoder_dims[i]
            if i == 0:
                n = neighborhoods[0].shape[2]
                table = token_embed_points(self.token_embed[0], neighborhoods[0].reshape(B * G, n, 3))
            else:
                k = idxs[i].numel() // (B * G)
                table = token_embed_merge(self.token_embed[i], table, idxs[i], B * G, k)
            lens, ids = compact_visible(masks[i])
            Tp = int(lens.max())                             # the one host read of the level
            if not 0 < Tp <= MAX_TOKENS:
                raise NotImplementedError('H_Encoder: %d visible tokens per cloud at level %d; the attention core '
                                          'takes 1 to %d' % (Tp, i, MAX_TOKENS))
            ctr = centers[i].reshape(B * G, 3).contiguous()
            x, cen = empty((B * Tp, C), table), empty((B * Tp, 3), table)
            _lib.call('pdae_m2ae_pack', table, B, G, Tp, C, _lib.ptr(ids), _lib.ptr(lens), _lib.ptr(table), _lib.ptr(ctr),
                      _lib.ptr(x), _lib.ptr(cen))
            pos = nn_ops.pos_embed(cen, self.encoder_pos_embeds[i])
            for blk in self.encoder_blocks[i].blocks:                                   # :340-343: x + pos every block
                x = block_forward(blk, x, pos, B, Tp, cen, lens, float(self.local_radius[i]))
            last = i == levels - 1
            if capture is not None or not last:
                x = x.resolve()                              # the level's output rows, before any norm
                if capture is not None:
                    valid = torch.arange(Tp, device=x.device).unsqueeze(0) < lens.unsqueeze(1)
                    capture['level%d' % i] = dict(lens=lens.clone(), T_pad=Tp, rows=x.reshape(B, Tp, C)[valid])
            if not last:                                     # :174: the valid rows replace the visible tokens
                _lib.call('pdae_m2ae_unpack', table, B, G, Tp, C, _lib.ptr(ids), _lib.ptr(lens), _lib.ptr(x),
                          _lib.ptr(table))
        # :177-178: only the last level's norm reaches the feature (it also adds the last block's pending branch)
        return nn_ops.layer_norm(x, self.encoder_norms[-1]).reshape(B, Tp, C)


@MODELS.register_module()
class Point_M2AE_SVMFeature(Classifier):
    """Point_M2AE.py:1079-1169: the hierarchical encoder as the frozen feature extractor of --svm_classification.
    get_loss_acc, load_model_from_ckpt and _init_weights are the classifier's (the reference's class carries copies)."""
    eval_only = ('the forward-only encoder of the linear-SVM protocol; training of Point-M2AE and Point_M2AE_Finetune are '
                 'not built')

    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.group_sizes = list(config.group_sizes)
        self.num_groups = list(config.num_groups)
        if len(self.group_sizes) != len(self.num_groups) or len(self.num_groups) != len(config.encoder_dims):
            raise ValueError('Point_M2AE_SVMFeature: num_groups, group_sizes and encoder_dims must have one length')
        if self.num_groups[0] > MAX_TOKENS:
            raise NotImplementedError('Point_M2AE_SVMFeature: num_groups[0] = %d; the attention core takes at most %d '
                                      'tokens per cloud' % (self.num_groups[0], MAX_TOKENS))
        if self.group_sizes[0] not in (4, 8, 16, 32):
            raise NotImplementedError('Point_M2AE_SVMFeature: group_sizes[0] = %d; the level-0 embedder tiles patches '
                                      'of 4, 8, 16 or 32 points' % self.group_sizes[0])
        self.group_dividers = nn.ModuleList(Group(num_group=g, group_size=k)
                                            for g, k in zip(self.num_groups, self.group_sizes))
        self.h_encoder = H_Encoder(config)

    def group(self, pts):
        """Point_M2AE.py:1155-1163 -> (neighborhoods, centers, idxs), finest level first."""
        neighborhoods, centers, idxs = [], [], []
        src = pts
        for divider in self.group_dividers:
            neighborhood, center, idx = divider(src)
            neighborhoods.append(neighborhood), centers.append(center), idxs.append(idx)
            src = center
        return neighborhoods, centers, idxs

    forward = torch.no_grad()(Classifier.forward_features)

    def trunk(self, pts, capture):
        """pts (B, N, 3) -> the feature (B, encoder_dims[-1]) = mean + max over the last level's normed tokens."""
        neighborhoods, centers, idxs = self.group(pts)
        x = self.h_encoder(neighborhoods, centers, idxs, eval=True, capture=capture)
        f = nn_ops.max_plus_mean(x)
        if capture is not None:
            capture.update(feature=f)
        return f
