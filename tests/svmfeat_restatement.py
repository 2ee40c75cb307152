"""Framework-op restatement of the PointNet++ encoder in evaluation mode (models/pointnetv2_util.py:319-346 on
extensions/pointnet2/pointnet2_modules.py:31-72 of the reference), in whatever dtype its inputs have: the yardstick of
tests/test_svmfeat_cpu.py (against the live reference's fp64 features) and of the GPU tests (the fp64 definition of
pdae_sa_eval_forward).  Explicit grouped rows, three affine + ReLU layers, max; the geometric decisions are inputs."""
import torch

EPS = 1e-5          # nn.BatchNorm2d's default, which pytorch_utils.BatchNorm2d keeps


def gather_rows(x, idx):
    """x (B, N, C), idx (B, ...) -> x[b, idx[b, ...]] (B, ..., C)."""
    B, _, C = x.shape
    flat = idx.reshape(B, -1).long()
    return torch.gather(x, 1, flat.unsqueeze(-1).expand(-1, -1, C)).reshape(*idx.shape, C)


def mlp_max(rows, layers):
    """rows (..., ns, K) -> max over ns of the affine + ReLU layers [(W (C_l, C_{l-1}), scale, shift)]."""
    for w, scale, shift in layers:
        rows = torch.relu(rows @ w.t() * scale + shift)
    return rows.max(dim=-2)[0]


def sa_level(xyz, new_xyz, idx, features, layers):
    """One grouped level: xyz (B,N,3), new_xyz (B,np,3), idx (B,np,ns), features (B,N,C0) or None -> (B,np,C3)."""
    rows = gather_rows(xyz, idx) - new_xyz.unsqueeze(2)                       # (B, np, ns, 3)
    if features is not None:
        rows = torch.cat([rows, gather_rows(features, idx)], dim=-1)
    return mlp_max(rows, layers)


def group_all(xyz, features, layers):
    """xyz (B,N,3), features (B,N,C) -> (B, C_last)."""
    return mlp_max(torch.cat([xyz, features], dim=-1), layers)


def level_layers(sd, prefix):
    """The eval-mode layers of `prefix`.mlps.0 out of a state dict -> [(W, scale, shift)]."""
    out, i = [], 0
    while '%s.mlps.0.layer%d.conv.weight' % (prefix, i) in sd:
        p = '%s.mlps.0.layer%d.' % (prefix, i)
        w = sd[p + 'conv.weight']
        scale = sd[p + 'bn.bn.weight'] / torch.sqrt(sd[p + 'bn.bn.running_var'] + EPS)
        shift = sd[p + 'bn.bn.bias'] - sd[p + 'bn.bn.running_mean'] * scale
        out.append((w.reshape(w.shape[0], -1), scale, shift))
        i += 1
    return out


def pointnetv2_feature(pts, sd, fps_idx, ball_idx, prefix='pointnetv2_encoder'):
    """pts (B,N,3), the model's state dict in pts' dtype, the recorded FPS (B,np) and ball-query (B,np,ns) indices of the
    two grouped levels -> (feature (B,1024), [level-1 rows (B,512,128), level-2 rows (B,128,256)])."""
    xyz, feats, levels = pts, None, []
    for lvl in range(2):
        new_xyz = gather_rows(xyz, fps_idx[lvl])
        feats = sa_level(xyz, new_xyz, ball_idx[lvl], feats, level_layers(sd, '%s.sa%d' % (prefix, lvl + 1)))
        levels.append(feats)
        xyz = new_xyz
    return group_all(xyz, feats, level_layers(sd, prefix + '.sa3')), levels
