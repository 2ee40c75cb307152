"""DGCNN classification fine-tuning model, MI355X host side (models/PointCAE_DGCNN.py:572-663 DGCNN of the reference).

The backbone is point_cae_dgcnn.dgcnn_encoder, the module Point_CAE_DGCNN_FCOnly holds under the same name, so a
checkpoint of that auto-encoder loads through builder.remap_pretrain_keys with strict=False: its recfc.* keys are
unexpected, cls_head_finetune.* missing, as in the reference:

    model = MODELS.build(cfg.model)              # cfg.model.NAME == 'DGCNN'
    model.load_model_from_ckpt(path_or_None)
    logits = model(points)                       # (B, cls_dim)
    loss, acc = model.get_loss_acc(logits, labels)

The encoder is the auto-encoder's explicit kernel sequence (csrc/dgcnn.hip).  The head Linear(1024, 512) -> BatchNorm1d
-> LeakyReLU(0.2) -> Linear(512, 256) -> BatchNorm1d -> LeakyReLU(0.2) -> Dropout(0.5) -> Linear(256, cls_dim) runs its
Linear layers on the row GEMMs (nn_ops.linear_any) and each BatchNorm + LeakyReLU [+ Dropout] as one launch
(finetune_ops.bn_lrelu_dropout); the loss is finetune_ops.softmax_xent_smooth (smoothloss) or softmax_xent.  There is
no CPU path.
"""
import logging

import torch
import torch.nn as nn

from . import finetune_ops, nn_ops
from .point_cae_dgcnn import dgcnn_encoder
from .point_cae_transformer import trunc_normal_
from .point_transformer import _missing_message, _unexpected_message
from .registry import MODELS

SMOOTH_EPS = 0.3           # get_loss_acc's label smoothing (PointCAE_DGCNN.py:594)
LRELU_SLOPE = 0.2


@MODELS.register_module()
class DGCNN(nn.Module):
    # parameters whose gradients backward produces last (FlatDataParallel lays them at the end of the flat buffer)
    late_grad_prefixes = ('dgcnn_encoder.',)

    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.cls_dim = config.cls_dim
        self.smoothing = bool(config.get('smoothloss', False))
        if not 2 <= self.cls_dim <= 64:
            raise NotImplementedError('DGCNN: cls_dim = %d; the loss kernels take 2 to 64 classes' % self.cls_dim)
        self.dgcnn_encoder = dgcnn_encoder(channel=3)
        self.cls_head_finetune = nn.Sequential(
            nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.LeakyReLU(negative_slope=LRELU_SLOPE, inplace=True),
            nn.Linear(512, 256), nn.BatchNorm1d(256), nn.LeakyReLU(negative_slope=LRELU_SLOPE, inplace=True),
            nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))

    # ---- the reference's helpers ------------------------------------------------------------------------------------
    def get_loss_acc(self, ret, gt):
        """PointCAE_DGCNN.py:592-605: with smoothloss the cross-entropy against the label-smoothed target (eps 0.3),
        else F.cross_entropy; the argmax accuracy in percent.  Both device scalars."""
        if self.smoothing:
            loss, correct = finetune_ops.softmax_xent_smooth(ret, gt, SMOOTH_EPS)
        else:
            loss, correct = finetune_ops.softmax_xent(ret, gt)
        return loss, correct * (100.0 / gt.shape[0])

    def load_model_from_ckpt(self, bert_ckpt_path, log=None):
        """PointCAE_DGCNN.py:607-638: a Point_CAE_DGCNN_FCOnly checkpoint with its keys remapped, strict=False, the
        missing and unexpected keys logged; None = training from scratch (_init_weights).  -> the incompatible-keys
        record (None from scratch)."""
        log = log or logging.getLogger('Transformer').info
        if bert_ckpt_path is None:
            log('Training from scratch!!!')
            self.apply(self._init_weights)
            return None
        from .builder import remap_pretrain_keys
        ckpt = torch.load(bert_ckpt_path, map_location='cpu')
        incompatible = self.load_state_dict(remap_pretrain_keys(ckpt['base_model']), strict=False)
        if incompatible.missing_keys:
            log('missing_keys')
            log(_missing_message(incompatible.missing_keys))
        if incompatible.unexpected_keys:
            log('unexpected_keys')
            log(_unexpected_message(incompatible.unexpected_keys))
        log(f'[Transformer] Successful Loading the ckpt from {bert_ckpt_path}')
        return incompatible

    @staticmethod
    def _init_weights(m):              # PointCAE_DGCNN.py:640-652: Linear and Conv1d (conv5); Conv2d and BatchNorm keep torch's
        if isinstance(m, (nn.Linear, nn.Conv1d)):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def draw_dropout(self, B, device):
        """The head's one dropout draw (B, 256) uniforms from torch's device generator (graph-safe: a replay draws again)."""
        return torch.rand(B, self.cls_head_finetune[3].out_features, device=device)

    def head(self, f, drop=None, drop_keep=None):
        """cls_head_finetune on the encoder feature f (B, 1024).  drop: the (B, 256) uniforms of its Dropout; drop_keep:
        a boolean keep mask (tests); neither in training mode: a fresh draw."""
        h = self.cls_head_finetune
        u = keep = None
        if self.training:
            if drop_keep is not None:
                keep = drop_keep
            else:
                u = drop if drop is not None else self.draw_dropout(f.shape[0], f.device)
        x = nn_ops.linear_any(f, h[0].weight, h[0].bias)
        x = finetune_ops.bn_lrelu_dropout(x, h[1], 0.0, h[2].negative_slope)
        x = nn_ops.linear_any(x, h[3].weight, h[3].bias)
        x = finetune_ops.bn_lrelu_dropout(x, h[4], h[6].p, h[5].negative_slope, u=u, keep=keep)
        return nn_ops.linear_any(x, h[7].weight, h[7].bias)

    def forward(self, pts, drop=None, drop_keep=None, capture=None):
        """pts (B, N, 3+) -> logits (B, cls_dim) (PointCAE_DGCNN.py:654-661)."""
        if not pts.is_cuda:
            raise RuntimeError('DGCNN: points must be on the GPU (there is no CPU path)')
        pts = pts[:, :, :3].contiguous()
        nn_ops.begin_step(pts.device)
        f = self.dgcnn_encoder.forward_rows(pts)                                     # (B, 1024)
        if capture is not None:
            capture.update(feature=f)
        return self.head(f, drop, drop_keep)
