"""The PointNet++ classifier (models/PointCAE_pointnetv2.py PointNetv2 of the reference) restated literally as framework
ops -- gather, concatenate, matmul, batch-statistics BatchNorm, max -- for the tests of point_dae_amd's PointNetv2.

Nothing of the kernels' algebra is here: every (centre, sample) row is gathered, centred and concatenated to
[xyz - centre | features] and multiplied by the whole first weight; BatchNorm takes the mean and the biased variance over
all rows; the pool is a max.  The FPS and ball-query indices are INPUTS (recorded from the reference), so the restatement
takes no geometric decision.  It runs in the dtype of its inputs (the tests use fp64) and is differentiated by autograd.

    logits = forward(state, pts, fps_idx, ball_idx, training)          state: a state_dict in the reference's names
    loss = smoothed_loss(logits, labels, eps)                          (eps None: plain cross-entropy)
"""
import torch

BN_EPS = 1e-5
LEVELS = ('sa1', 'sa2', 'sa3')


def _conv_bn_relu(x, state, prefix, training):
    """x (..., Cin) -> relu(bn(x W^T)) (..., Cout); BatchNorm2d over every leading dimension."""
    w = state[prefix + '.conv.weight']
    x = torch.matmul(x, w.reshape(w.shape[0], -1).t())
    return _bn_relu(x, state, prefix + '.bn.bn', training)


def _bn_relu(x, state, prefix, training):
    dims = tuple(range(x.dim() - 1))
    if training:
        mean = x.mean(dim=dims)
        var = ((x - mean) ** 2).mean(dim=dims)
    else:
        mean, var = state[prefix + '.running_mean'], state[prefix + '.running_var']
    x = (x - mean) / torch.sqrt(var + BN_EPS) * state[prefix + '.weight'] + state[prefix + '.bias']
    return torch.relu(x)


def _layers(state, level):
    n = 0
    while 'pointnetv2_encoder.%s.mlps.0.layer%d.conv.weight' % (level, n) in state:
        n += 1
    return ['pointnetv2_encoder.%s.mlps.0.layer%d' % (level, i) for i in range(n)]


def sa_level(state, level, xyz, feats, fps_idx, ball_idx, training):
    """xyz (B,N,3), feats (B,N,C) or None, fps_idx (B,np), ball_idx (B,np,ns) -> new_xyz (B,np,3), (B,np,C')."""
    B = xyz.shape[0]
    batch = torch.arange(B).view(B, 1, 1)
    new_xyz = torch.gather(xyz, 1, fps_idx.long().unsqueeze(-1).expand(-1, -1, 3))
    ball = ball_idx.long()
    g = xyz[batch, ball] - new_xyz.unsqueeze(2)                               # (B, np, ns, 3)
    if feats is not None:
        g = torch.cat([g, feats[batch, ball]], dim=-1)
    for prefix in _layers(state, level):
        g = _conv_bn_relu(g, state, prefix, training)
    return new_xyz, g.max(dim=2)[0]


def group_all_level(state, level, xyz, feats, training):
    """One group holding every point, coordinates as they are: (B,N,3), (B,N,C) -> (B, C')."""
    g = torch.cat([xyz, feats], dim=-1)
    for prefix in _layers(state, level):
        g = _conv_bn_relu(g, state, prefix, training)
    return g.max(dim=1)[0]


def encoder(state, pts, fps_idx, ball_idx, training):
    l1_xyz, l1 = sa_level(state, 'sa1', pts, None, fps_idx[0], ball_idx[0], training)
    l2_xyz, l2 = sa_level(state, 'sa2', l1_xyz, l1, fps_idx[1], ball_idx[1], training)
    return group_all_level(state, 'sa3', l2_xyz, l2, training)


def head(state, f, training):
    """cls_head_finetune with its Dropout modules at p = 0: Linear - BatchNorm1d - ReLU, twice, then Linear."""
    h = 'cls_head_finetune.'
    x = torch.matmul(f, state[h + '0.weight'].t()) + state[h + '0.bias']
    x = _bn_relu(x, state, h + '1', training)
    x = torch.matmul(x, state[h + '4.weight'].t()) + state[h + '4.bias']
    x = _bn_relu(x, state, h + '5', training)
    return torch.matmul(x, state[h + '8.weight'].t()) + state[h + '8.bias']


def forward(state, pts, fps_idx, ball_idx, training):
    return head(state, encoder(state, pts, fps_idx, ball_idx, training), training)


def smoothed_loss(logits, labels, eps):
    logp = torch.log_softmax(logits, dim=1)
    if eps is None:
        return -logp.gather(1, labels.long().view(-1, 1)).mean()
    n = logits.shape[1]
    one_hot = torch.zeros_like(logits).scatter(1, labels.long().view(-1, 1), 1)
    target = one_hot * (1 - eps) + (1 - one_hot) * eps / (n - 1)
    return -(target * logp).sum(dim=1).mean()
