"""PointNet++ denoising auto-encoder (BASELINE configs 1-2), MI355X host side.

Reference: models/PointCAE_pointnetv2.py:61-173 (`Point_CAE_PointNetv2`) with the
encoder of models/pointnetv2_util.py:319-346; the set-abstraction module is the
third-party pointnet2_ops `PointnetSAModule`, whose vendored twin
(extensions/pointnet2/pointnet2_modules.py:31-72,124-158, pytorch_utils.py)
gives the parameter names kept here (`...mlps.0.layer{i}.conv.weight`,
`...layer{i}.bn.bn.weight`).

    model(corrupted_pts, pts) -> (loss_coarse, loss_fine)

Data path on MI355X: FPS+centre gather, ball query and the Chamfer losses are the
gfx950 kernels; activations are rows (points) x channels, so grouping is a row
gather and max-pool a reduction over consecutive rows.  folding2's first layer
is not run on the materialised (B,16384,1029) tensor (67 MB per cloud in the
reference, :157-163): its weight is split into the grid (2), coarse-point (3) and
global-feature (1024) column blocks, which are multiplied once per grid cell,
once per coarse point and once per cloud and added by broadcasting -- the same
sum, 25.9 -> 8.7 GFLOP per cloud.
"""
import itertools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import nn_ops, sa_eval_ops, sa_mlp
from .arena import begin_step
from .chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
from .classifier import Classifier
from .corrupt_util_tensor import corrupt_in_forward
from .pointnet2_utils import ball_query, furthest_point_sample_with_centres
from .registry import MODELS
from .rows import linear_any, pad2d, split_weight_cols
from .sa_mlp import _GroupRows  # noqa: F401  (its home is sa_mlp; tests import it from here)


class _ConvBN(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__()
        self.add_module('conv', nn.Conv2d(cin, cout, kernel_size=(1, 1), bias=False))
        bn = nn.Sequential()
        bn.add_module('bn', nn.BatchNorm2d(cout))
        self.add_module('bn', bn)
        self.add_module('activation', nn.ReLU(inplace=True))
        nn.init.kaiming_normal_(self.conv.weight)

    def rows(self, x, pad_at=None):
        """(rows, cin) -> relu(bn(conv)) (rows, cout); BatchNorm statistics over the rows.
        pad_at: x carries a zero column at that index (the 3 xyz columns padded to 4 so that the
        row GEMM reduces over a multiple of 4); the weight gets the matching zero column."""
        bn = self.bn.bn
        w = self.conv.weight.reshape(self.conv.weight.shape[0], -1)
        if pad_at is not None:
            w = torch.cat([w[:, :pad_at], w.new_zeros(w.shape[0], 1), w[:, pad_at:]], dim=1)
        y = linear_any(x, w)
        if isinstance(bn, nn.SyncBatchNorm):
            return F.relu(bn(y))                       # --sync_bn: the module owns the cross-replica statistics
        if self.training:
            bn.num_batches_tracked += 1
        y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training,
                         bn.momentum, bn.eps)
        return F.relu(y)


class SharedMLP(nn.Sequential):
    def __init__(self, spec):
        super().__init__()
        for i in range(len(spec) - 1):
            self.add_module('layer{}'.format(i), _ConvBN(spec[i], spec[i + 1]))


class PointnetSAModule(nn.Module):
    """FPS -> ball query -> group (centre-subtracted xyz || features) -> shared MLP -> max.
    fused_eval: in evaluation mode take the forward-only level of sa_eval_ops (PDAE_SA_EVAL=hip, the default) where it
    takes the layout; off (the default), and in training mode, forward is untouched by it.
    split_first: in training mode run the first layer split by source point (sa_mlp.SplitFirstMLPMaxFunction: no grouped
    rows) where csrc/sa_train.hip takes the layout, the grouped form elsewhere; off (the default): the grouped form, untouched.
    A group-all level has every point once, so the switch does nothing there."""

    def __init__(self, mlp, npoint=None, radius=None, nsample=None, use_xyz=True, fused_eval=False, split_first=False):
        super().__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.fused_eval = bool(fused_eval) and use_xyz
        self.split_first = bool(split_first) and use_xyz and npoint is not None
        spec = list(mlp)
        if use_xyz:
            spec[0] += 3
        self.mlps = nn.ModuleList([SharedMLP(spec)])

    def forward(self, xyz, features=None, capture=None):
        """xyz (B,N,3); features rows (B*N, C) or None -> new_xyz (B,np,3), rows (B*np, C').  capture: a dict that
        receives the level's FPS and ball-query indices and, from a split_first level in training mode, which form of
        the first layer ran ('first': 'split' or 'grouped') (tests)."""
        B, N, _ = xyz.shape
        layers = list(self.mlps[0])
        grouped = self.npoint is not None                  # (else the group-all level: one group per cloud, no centres)
        new_xyz = idx = None
        if grouped:
            with torch.no_grad():
                fps_idx, new_xyz = furthest_point_sample_with_centres(xyz, self.npoint)
                idx = ball_query(self.radius, self.nsample, xyz, new_xyz)          # (B,np,ns) i32
            if capture is not None:
                capture.update(fps_idx=fps_idx, ball_idx=idx)
        if self.fused_eval and not self.training and sa_eval_ops.mode() == 'hip':
            out = (sa_eval_ops.level(xyz, new_xyz, idx, features, layers) if grouped else
                   sa_eval_ops.group_all(xyz, features, layers))
            if out is not None:                  # (None: a layout the kernel refuses -- the layer-by-layer form below)
                return new_xyz, out
        if self.split_first and self.training:   # (never set on a group-all level)
            C = 0 if features is None else features.shape[1]
            split = (sa_mlp.split_first_supported(B, N, self.npoint, self.nsample, C, layers[0].conv.out_channels)
                     and sa_mlp.batch_stats_are_local(layers))
            if capture is not None:
                capture['first'] = 'split' if split else 'grouped'
            if split:                            # (else: a layout the kernels refuse -- the grouped form below)
                return new_xyz, sa_mlp.split_first_mlp_max(xyz, new_xyz, idx, features, layers)
        if grouped:
            g, groups, per = sa_mlp.group_rows(xyz, new_xyz, idx, features), B * self.npoint, self.nsample
        else:
            g, groups, per = sa_mlp.all_rows(xyz.reshape(B * N, 3), features), B, N
        if self.training and sa_mlp.fused_chain_supported(per, g.shape[0], layers):
            return new_xyz, sa_mlp.shared_mlp_max(g, layers, per, pad_at=3)
        for i, layer in enumerate(layers):
            g = layer.rows(g, pad_at=3 if i == 0 else None)
        return new_xyz, g.reshape(groups, per, -1).max(dim=1)[0]


class PointNetv2_encoder(nn.Module):
    def __init__(self, num_channel=3, fused_eval=False, split_first=False):
        super().__init__()
        self.sa1 = PointnetSAModule(npoint=512, radius=0.2, nsample=32, mlp=[0, 64, 64, 128], fused_eval=fused_eval,
                                    split_first=split_first)
        self.sa2 = PointnetSAModule(npoint=128, radius=0.4, nsample=64, mlp=[128, 128, 128, 256], fused_eval=fused_eval,
                                    split_first=split_first)
        self.sa3 = PointnetSAModule(mlp=[256, 256, 512, 1024], fused_eval=fused_eval)

    def forward(self, xyz, capture=None):
        caps = [None if capture is None else {} for _ in range(2)]
        l1_xyz, l1 = self.sa1(xyz, None, caps[0])
        l2_xyz, l2 = self.sa2(l1_xyz, l1, caps[1])
        _, l3 = self.sa3(l2_xyz, l2)
        if capture is not None:
            capture.update(fps_idx=[c['fps_idx'] for c in caps], ball_idx=[c['ball_idx'] for c in caps], levels=[l1, l2])
            if any('first' in c for c in caps):
                capture['first'] = [c.get('first') for c in caps]
        return l3                                                  # (B, 1024)


@MODELS.register_module()
class Point_CAE_PointNetv2(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.corrupt_type = config.corrupt_type
        self.grid_size, self.grid_scale, self.num_coarse = 4, 0.05, 1024
        self.num_fine = self.grid_size ** 2 * self.num_coarse
        self.pointnetv2_encoder = PointNetv2_encoder()
        self.folding1 = nn.Sequential(nn.Linear(1024, 1024), nn.ReLU(), nn.Linear(1024, 1024), nn.ReLU(),
                                      nn.Linear(1024, self.num_coarse * 3))
        self.folding2 = nn.Sequential(nn.Conv1d(1024 + 2 + 3, 512, 1), nn.ReLU(), nn.Conv1d(512, 512, 1),
                                      nn.ReLU(), nn.Conv1d(512, 3, 1))
        x = np.linspace(-self.grid_scale, self.grid_scale, self.grid_size)
        grid = torch.tensor(np.array(list(itertools.product(x, x)))).float()   # (16, 2), build_grid :94-99
        self.register_buffer('grid', grid, persistent=False)
        self.loss = config.loss
        self.build_loss_func(self.loss)

    @property
    def draws_in_forward(self):
        """True when forward() draws random numbers on the host (the in-forward corruptions): such a step
        must not be captured into a hipGraph -- the draw and its H2D copy would be replayed frozen."""
        return any(item in ('dropout_global', 'dropout_patch_pointmae') for item in self.corrupt_type)

    def build_loss_func(self, loss_type):
        if loss_type == 'cdl1':
            self.loss_func = ChamferDistanceL1()
        elif loss_type == 'cdl2':
            self.loss_func = ChamferDistanceL2()
        else:
            raise NotImplementedError(loss_type)

    def forward(self, corrupted_pts, pts, vis=False, capture=None, **kwargs):
        begin_step(pts.device)
        corrupted_pts = corrupted_pts[:, :, :3].contiguous()
        pts = pts[:, :, :3].contiguous()
        # the CUDA-side dropouts of the reference's forward (:143-149); everything else came from the loader
        corrupted_pts = corrupt_in_forward(corrupted_pts, self.corrupt_type, ('dropout_patch_pointmae', 'dropout_global'))
        B = pts.shape[0]
        feature = self.pointnetv2_encoder(corrupted_pts)                       # (B, 1024)
        f1 = self.folding1
        coarse = nn_ops.mlp_chain(feature, [f1[0], f1[2], f1[4]])
        coarse = coarse.view(B, self.num_coarse, 3)
        # folding2[0] on [grid(2) | coarse point(3) | global feature(1024)], split by column block
        w = self.folding2[0].weight.squeeze(-1)                                # (512, 1029)
        g2 = self.grid_size ** 2
        wg, wc, wf = split_weight_cols(w, [(0, 2), (2, 5), (5, w.shape[1])])                 # (narrow blocks padded to 4 columns)
        a = linear_any(feature, wf, self.folding2[0].bias)                                  # (B, 512)  once per cloud
        p = linear_any(pad2d(coarse.reshape(-1, 3), 0, 1), wc).reshape(B, self.num_coarse, 1, -1)                 # once per coarse point
        gd = linear_any(pad2d(self.grid, 0, 2), wg)                             # (16, 512)     once per grid cell
        off = nn_ops.fold_mlp(a, p.reshape(B * self.num_coarse, -1), gd, self.folding2[2], self.folding2[4],
                              B, self.num_coarse, g2)
        fine = off.reshape(B, self.num_coarse, g2, 3) + coarse.unsqueeze(2)
        fine = fine.reshape(B, self.num_fine, 3)
        if capture is not None:
            capture.update(feature=feature, coarse=coarse, fine=fine)
        return self.loss_func(coarse, pts), self.loss_func(fine, pts)


SMOOTH_EPS = 0.3           # get_loss_acc's label smoothing (PointCAE_pointnetv2.py:950-957)


class _PointNetv2Classifier(Classifier):
    """What PointNetv2_feat and PointNetv2 share: the config fields, the class count the loss kernels take, get_loss_acc's
    label smoothing (the reference's get_loss_acc: eps 0.3 with smoothloss, else F.cross_entropy) and the trunk.  A
    subclass builds pointnetv2_encoder."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.cls_dim = config.cls_dim
        self.smoothing = bool(config.get('smoothloss', False))
        if not 2 <= self.cls_dim <= 64:
            raise NotImplementedError('%s: cls_dim = %d; the loss kernels take 2 to 64 classes'
                                      % (type(self).__name__, self.cls_dim))

    @property
    def smooth_eps(self):
        return SMOOTH_EPS if self.smoothing else None

    def trunk(self, pts, capture):
        """pts (B, N, 3) -> the encoder's feature (B, 1024) (PointCAE_pointnetv2.py:833-840)."""
        f = self.pointnetv2_encoder(pts, capture)
        if capture is not None:
            capture.update(feature=f)
        return f


@MODELS.register_module()
class PointNetv2_feat(_PointNetv2Classifier):
    """models/PointCAE_pointnetv2.py:936-1017: the PointNet++ encoder as the frozen feature extractor of
    --svm_classification -- pointnetv2_encoder and nothing else that carries parameters, so a Point_CAE_PointNetv2
    checkpoint loads with folding1.* / folding2.* unexpected and nothing missing.  get_loss_acc, load_model_from_ckpt and
    _init_weights are the classifier's (the reference's class carries copies).  Forward only, evaluation mode only, no CPU
    path: the encoder runs its levels on sa_eval_ops (PDAE_SA_EVAL=hip, the default; =layers: layer by layer)."""
    eval_only = 'the forward-only encoder of the linear-SVM protocol; PointNet++ fine-tuning is not built'

    def __init__(self, config, **kwargs):
        super().__init__(config)
        self.pointnetv2_encoder = PointNetv2_encoder(fused_eval=True)

    forward = torch.no_grad()(Classifier.forward_features)       # pts (B, N, 3+) -> the encoder's feature (B, 1024)


# measured on the graphed fine-tuning step at B = 32 (tools/bench_pointnetv2_cls.py): split 3.84 ms against
# grouped 4.14 at N = 1024, 3.99 against 4.27 at N = 2048; the spread of grouped is 0.04 and 0.07
SA_FIRST_DEFAULT = 'split'


def sa_first_mode():
    """PDAE_SA_FIRST: how the classifier's sa1 and sa2 run their first layer in training mode -- 'split' (by source point,
    sa_mlp.SplitFirstMLPMaxFunction) or 'grouped' (sa_mlp.group_rows + SharedMLPMaxFunction, the pretraining step's form:
    the fallback for the layouts the split kernels refuse, and the A/B and timing baseline)."""
    mode = os.environ.get('PDAE_SA_FIRST', '') or SA_FIRST_DEFAULT
    if mode not in ('split', 'grouped'):
        raise ValueError("PDAE_SA_FIRST must be 'split' or 'grouped', got %r" % mode)
    return mode


@MODELS.register_module()
class PointNetv2(_PointNetv2Classifier):
    """models/PointCAE_pointnetv2.py:749-842: the PointNet++ encoder of a Point_CAE_PointNetv2 checkpoint fine-tuned as a
    classifier.  pointnetv2_encoder is the auto-encoder's module under the same name, so its checkpoint loads with
    folding1.* / folding2.* unexpected and cls_head_finetune.* missing; the head Linear(1024, 512) -> BatchNorm1d -> ReLU ->
    Dropout(0.5) -> Linear(512, 256) -> BatchNorm1d -> ReLU -> Dropout(0.5) -> Linear(256, cls_dim) runs on
    Classifier.head.  get_loss_acc, load_model_from_ckpt and _init_weights are the classifier's.

    Evaluation mode runs the fused levels of sa_eval_ops, as PointNetv2_feat does; training mode runs sa1 and sa2 as
    PDAE_SA_FIRST says (sa_first_mode, read here) and sa3, the group-all level, in the grouped form.  There is no CPU path."""

    # parameters whose gradients backward produces last (FlatDataParallel lays them at the end of the flat buffer)
    late_grad_prefixes = ('pointnetv2_encoder.sa1.',)
    input_grad_supported = False
    only_new_unsupported = ("set_bn_eval freezes every BatchNorm whose width is not 256, which leaves pointnetv2_encoder.sa2's "
                            "last and sa3's first BatchNorm (256 channels) in training mode beside frozen ones; the clip norm "
                            "is taken over the whole gradient, so the protocol needs an encoder backward through that mix of "
                            "batch-statistics and running-estimate BatchNorms, and the set-abstraction levels' autograd nodes "
                            "differentiate training-mode BatchNorm only")

    def __init__(self, config, **kwargs):
        super().__init__(config)
        self.sa_first = sa_first_mode()
        self.pointnetv2_encoder = PointNetv2_encoder(fused_eval=True, split_first=self.sa_first == 'split')
        self.cls_head_finetune = nn.Sequential(
            nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))
