"""Point-M2AE's hierarchical encoder in evaluation mode, restated as plain framework ops (a test helper, not a test).

Written from the description of what the reference computes (models/Point_M2AE.py H_Encoder.forward with eval=True,
Point_M2AE_SVMFeature.forward; models/Point_M2AE_modules.py Token_Embed / Attention / Block), on any device, in the
dtype of the state dict (fp32 or fp64).  It is the yardstick of the GPU tests: tests/test_m2ae_cpu.py checks that in
fp64 it reproduces the live reference's fp64 features stored in tests/golden/m2ae_svmfeat_*.npz.

One deliberate difference: the radius mask of a level always comes from that level's own
centres; the reference reuses the previous level's distances when two consecutive levels pad to the same length.
"""
import torch
import torch.nn.functional as F

EPS = 1e-5                                      # nn.BatchNorm1d / nn.LayerNorm defaults


def _conv(sd, name, x):
    return x @ sd[name + '.weight'].squeeze(-1).t() + sd[name + '.bias']


def _bn_eval(sd, name, x):
    inv = torch.rsqrt(sd[name + '.running_var'] + EPS)
    return (x - sd[name + '.running_mean']) * inv * sd[name + '.weight'] + sd[name + '.bias']


def _ln(sd, name, x):
    return F.layer_norm(x, (x.shape[-1],), sd[name + '.weight'], sd[name + '.bias'], EPS)


def _linear(sd, name, x):
    y = x @ sd[name + '.weight'].t()
    return y + sd[name + '.bias'] if name + '.bias' in sd else y


def token_embed(sd, prefix, groups):
    """Token_Embed on groups (P, n, C_in) -> (P, C_out): conv, BN (running statistics), ReLU, conv, max over the
    group, concat [global, local], conv, BN, ReLU, conv, max."""
    P, n, _ = groups.shape
    x = groups.reshape(P * n, -1)
    f = _conv(sd, prefix + '.first_conv.3', torch.relu(_bn_eval(sd, prefix + '.first_conv.1', _conv(sd, prefix + '.first_conv.0', x))))
    f = f.reshape(P, n, -1)
    g = f.max(dim=1, keepdim=True)[0]
    cat = torch.cat([g.expand(-1, n, -1), f], dim=2).reshape(P * n, -1)
    t = _conv(sd, prefix + '.second_conv.3', torch.relu(_bn_eval(sd, prefix + '.second_conv.1', _conv(sd, prefix + '.second_conv.0', cat))))
    return t.reshape(P, n, -1).max(dim=1)[0]


def attention_mask(centres, lens, radius):
    """(B, T, T) with 1 = masked: mask_vis[b, q, k] = 0 iff q < L_b and k < L_b; with radius > 0 the product with
    (distance >= radius).  centres (B, T, 3) with the padded rows zero."""
    B, T, _ = centres.shape
    valid = torch.arange(T, device=centres.device).unsqueeze(0) < lens.unsqueeze(1)
    mask_vis = (~(valid.unsqueeze(2) & valid.unsqueeze(1))).to(centres.dtype)
    if radius > 0:
        d = (centres.unsqueeze(2) - centres.unsqueeze(1)).pow(2).sum(-1).sqrt()
        return (d >= radius).to(centres.dtype) * mask_vis
    return mask_vis


def attention(q, k, v, scale, mask):
    """q, k, v (B, H, T, D), mask (B, T, T) -> (B, H, T, D): softmax(q k^T * scale + mask * -100000) v."""
    s = (q @ k.transpose(-2, -1)) * scale + (mask * -100000.0).unsqueeze(1)
    return s.softmax(dim=-1) @ v


def block(sd, prefix, x, mask, num_heads):
    B, T, C = x.shape
    D = C // num_heads
    qkv = _linear(sd, prefix + '.attn.qkv', _ln(sd, prefix + '.norm1', x)).reshape(B, T, 3, num_heads, D).permute(2, 0, 3, 1, 4)
    o = attention(qkv[0], qkv[1], qkv[2], D ** -0.5, mask).transpose(1, 2).reshape(B, T, C)
    x = x + _linear(sd, prefix + '.attn.proj', o)
    h = F.gelu(_linear(sd, prefix + '.mlp.fc1', _ln(sd, prefix + '.norm2', x)))
    return x + _linear(sd, prefix + '.mlp.fc2', h)


def visibility(centers, idxs):
    """Multi-scale masking from an all-visible top level -> [masked (B, G_i) bool], finest level first."""
    B = centers[0].shape[0]
    masks = [torch.zeros(B, centers[-1].shape[1], dtype=torch.bool, device=centers[0].device)]
    for i in range(len(centers) - 1, 0, -1):
        G, Gc = centers[i].shape[1], centers[i - 1].shape[1]
        idx = idxs[i].reshape(B * G, -1).long()
        idx_masked = (~masks[-1].reshape(-1)).unsqueeze(-1) * idx              # masked parents send index 0
        child = torch.ones(B * Gc, dtype=torch.bool, device=idx.device)
        child[idx_masked.reshape(-1)] = False
        masks.append(child.reshape(B, Gc))
    masks.reverse()
    return masks


def forward(neighborhoods, centers, idxs, sd, num_heads=6, local_radius=(0.32, 0.64, 1.28)):
    """-> dict(feature (B, C_last), levels = [dict(lens (B,), T_pad, rows = the valid output rows before the norm)])."""
    pre = 'h_encoder.'
    dtype = sd[pre + 'encoder_norms.0.weight'].dtype
    B = centers[0].shape[0]
    masks = visibility(centers, idxs)
    levels, x_vis = [], None
    for i in range(len(centers)):
        G = centers[i].shape[1]
        if i == 0:
            n = neighborhoods[0].shape[2]
            tokens = token_embed(sd, pre + 'token_embed.0', neighborhoods[0].to(dtype).reshape(B * G, n, 3)).reshape(B, G, -1)
        else:
            k = idxs[i].numel() // (B * G)
            merged = x_vis.reshape(-1, x_vis.shape[-1])[idxs[i].long()].reshape(B * G, k, -1)
            tokens = token_embed(sd, pre + 'token_embed.%d' % i, merged).reshape(B, G, -1)
        C = tokens.shape[-1]
        vis = ~masks[i]
        lens = vis.sum(1)
        Tp = int(lens.max())
        x = torch.zeros(B, Tp, C, dtype=dtype, device=tokens.device)
        cen = torch.zeros(B, Tp, 3, dtype=dtype, device=tokens.device)
        for b in range(B):
            x[b, :lens[b]] = tokens[b][vis[b]]
            cen[b, :lens[b]] = centers[i][b].to(dtype)[vis[b]]
        mask = attention_mask(cen, lens, local_radius[i])
        pos = _linear(sd, pre + 'encoder_pos_embeds.%d.2' % i, F.gelu(_linear(sd, pre + 'encoder_pos_embeds.%d.0' % i, cen)))
        j = 0
        while pre + 'encoder_blocks.%d.blocks.%d.norm1.weight' % (i, j) in sd:
            x = block(sd, pre + 'encoder_blocks.%d.blocks.%d' % (i, j), x + pos, mask, num_heads)
            j += 1
        valid = torch.arange(Tp, device=x.device).unsqueeze(0) < lens.unsqueeze(1)
        levels.append(dict(lens=lens, T_pad=Tp, rows=x[valid]))
        if i < len(centers) - 1:
            tokens = tokens.clone()
            tokens[vis] = x[valid]
            x_vis = tokens
    x = _ln(sd, pre + 'encoder_norms.%d' % (len(centers) - 1), x)
    return dict(feature=x.mean(1) + x.max(1)[0], levels=levels)
