"""Framework-op restatement of DGCNNPartSeg's evaluation forward (point_dae_amd/dgcnn_partseg.py), in whatever dtype its
inputs have: the yardstick of tests/test_dgcnn_partseg_cpu.py (against the live reference's fp64 logits) and of the GPU
tests (the fp64 definition of the csrc/edge2_eval.hip and csrc/partseg.hip kernels).

The three graphs are inputs.  Everything is written literally, layer by layer: the (B, N, k, 2C) edge tensor
[x_j - x_i | x_i], conv + BatchNorm + LeakyReLU once or twice per edge, the max over k, the (B, N, 1280) concatenation
[global | label | x1 | x2 | x3], four more layers.  None of the kernels' algebra (p[j] + q[i], the per-cloud bias, the
winner by the sign of gamma) appears here."""
import torch

from partseg_restatement import bn, conv, gather_rows

SLOPE = 0.2


def lrelu(x):
    return torch.where(x > 0, x, SLOPE * x)


def layer(x, sd, p):
    """conv (no bias) + eval-mode BatchNorm + LeakyReLU on the last dimension; p names the Sequential."""
    return lrelu(bn(conv(x, sd, p + '0.'), sd, p + '1.'))


def edge_features(x, idx):
    """x (B, N, C), idx (B, N, k) -> (B, N, k, 2C) = [x_j - x_i | x_i] (dgcnn_util.get_graph_feature)."""
    nbr = gather_rows(x, idx)
    ctr = x.unsqueeze(2).expand_as(nbr)
    return torch.cat([nbr - ctr, ctr], dim=-1)


def edgeconv2(x, idx, sd, p1, p2):
    """A two-layer EdgeConv on x (B, N, C): max over the neighbours of layer(layer(edge features))."""
    return layer(layer(edge_features(x, idx), sd, p1), sd, p2).max(dim=2)[0]


def encoder(pts, sd, graphs, pre='dgcnn_encoder.'):
    """pts (B, N, 3), graphs (3, B, N, k) -> (x1, x2, x3 (B, N, 64), global (B, 1024))."""
    x1 = edgeconv2(pts, graphs[0], sd, pre + 'conv1.', pre + 'conv2.')
    x2 = edgeconv2(x1, graphs[1], sd, pre + 'conv3.', pre + 'conv4.')
    x3 = layer(edge_features(x2, graphs[2]), sd, pre + 'conv5.').max(dim=2)[0]
    g = layer(torch.cat([x1, x2, x3], dim=-1), sd, pre + 'conv6.').max(dim=1)[0]
    return x1, x2, x3, g


def forward(pts, cls, sd, graphs):
    """pts (B, N, 3), cls (B,), the model's state dict in pts' dtype, graphs (3, B, N, k) integer
    -> dict(logits (B, N, P), x1, x2, x3, global)."""
    B, N, _ = pts.shape
    x1, x2, x3, g = encoder(pts, sd, graphs)
    onehot = torch.zeros(B, sd['conv7.0.weight'].shape[1], dtype=pts.dtype)
    onehot[torch.arange(B), cls.long()] = 1.0
    lab = layer(onehot, sd, 'conv7.')
    x = torch.cat([torch.cat([g, lab], dim=-1).unsqueeze(1).expand(-1, N, -1), x1, x2, x3], dim=-1)      # (B, N, 1280)
    for name in ('conv8.', 'conv9.', 'conv10.'):
        x = layer(x, sd, name)
    return {'logits': conv(x, sd, 'conv11.'), 'x1': x1, 'x2': x2, 'x3': x3, 'global': g}


def knn_distance(x):
    """dgcnn_util.knn's expression on rows: x (B, N, C) -> pd (B, N, N) = -xx_i - (-2 x_i . x_j) - xx_j (the larger the
    nearer)."""
    inner = -2 * (x @ x.transpose(1, 2))
    xx = (x ** 2).sum(-1, keepdim=True)
    return -xx.transpose(1, 2) - inner - xx


def edge2(pq, idx, scale1, shift1, w2, scale2, shift2):
    """The definition of pdae_edge2_eval_forward: pq (B, N, 2C) = [p | q], idx (B, N, k) -> (B, N, C2)."""
    C = pq.shape[-1] // 2
    h = lrelu((gather_rows(pq[..., :C], idx) + pq[..., C:].unsqueeze(2)) * scale1 + shift1)
    return lrelu((h @ w2.t()) * scale2 + shift2).max(dim=2)[0]


def logits_tail(y, scale, shift, w, bias=None):
    out = lrelu(y * scale + shift) @ w.t()
    return out + bias if bias is not None else out
