"""Part segmentation on ShapeNetPart, MI355X host side: the reference's segmentation model (segmentation/models/pt.py:178-333
get_model) in evaluation mode, forward only.

Same parameter and buffer names and shapes as the reference, so its segmentation checkpoints load
(load_segmentation_checkpoint: the dict's model_state_dict under these names, or the older layout without the `_cls`
suffix, pt.py:264-285), and a pretraining checkpoint of this repository loads through the inherited load_model_from_ckpt
with the head missing and the decoder unexpected.

    model = MODELS.build(cfg.model)                         # cfg.model.NAME == 'PointTransformerPartSeg'
    model.load_segmentation_checkpoint(path)
    logp = model(points, cls_label)                         # (B, N, 50) log-probabilities, fp32

The trunk is the classifiers': FPS + kNN grouping, the fused patch embedder on every group, pos_embed, the pre-LN blocks
on flat (B*G, C) rows -- no class token, T = num_group tokens per cloud -- with the taps behind blocks 3, 7 and 11 each
through the final LayerNorm (a tap's LayerNorm kernel adds the pending MLP branch itself; the same pending branch goes
on into the next block).  The head is partseg_ops.head (csrc/partseg.hip).  There is no CPU path and no training.
"""
import logging

import torch
import torch.nn as nn

from . import nn_ops, partseg_ops
from .arena import begin_step
from .classifier import Classifier
from .point_cae_transformer import Encoder, Group, TransformerEncoder, pos_embed_layers
from .registry import MODELS

MAX_TOKENS = 128           # the attention kernels take T <= 128 tokens per cloud (csrc/attention.hip)
FETCH_IDX = (3, 7, 11)     # pt.py:170


class PointNetFeaturePropagation(nn.Module):
    """The parameters of segmentation/models/pointnet2_utils.py:262-271; the forward is partseg_ops.head."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out


@MODELS.register_module()
class PointTransformerPartSeg(Classifier):
    """pt.py:178-333.  Never trained here: forward only, evaluation mode only."""
    late_grad_prefixes = ()

    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.trans_dim = config.get('trans_dim', 384)
        self.depth = config.get('depth', 12)
        self.drop_path_rate = config.get('drop_path_rate', 0.1)
        self.cls_dim = config.get('cls_dim', 50)
        self.num_heads = config.get('num_heads', 6)
        self.group_size = config.get('group_size', 32)
        self.num_group = config.get('num_group', 128)
        self.encoder_dims = config.get('encoder_dims', 384)
        self.num_categories = config.get('num_categories', 16)
        name = type(self).__name__
        if self.num_group > MAX_TOKENS:
            raise NotImplementedError('%s: num_group = %d tokens per cloud; the attention kernels take at most %d'
                                      % (name, self.num_group, MAX_TOKENS))
        if self.num_group < 3:
            raise NotImplementedError('%s: num_group = %d; the propagation interpolates between the three nearest centres '
                                      '(the reference\'s single-centre branch is another formula)' % (name, self.num_group))
        if self.encoder_dims != self.trans_dim:
            raise NotImplementedError('%s: encoder_dims must equal trans_dim (the tokens feed the blocks)' % name)
        if self.depth <= max(FETCH_IDX):
            raise NotImplementedError('%s: depth %d; the taps sit behind blocks %s' % (name, self.depth, FETCH_IDX))
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.pos_embed = pos_embed_layers(self.trans_dim)
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(self.trans_dim, self.depth, self.num_heads, dpr)
        self.norm = nn.LayerNorm(self.trans_dim)
        self.label_conv_cls = nn.Sequential(nn.Conv1d(self.num_categories, 64, kernel_size=1, bias=False),
                                            nn.BatchNorm1d(64), nn.LeakyReLU(0.2))
        feat = len(FETCH_IDX) * self.trans_dim
        self.propagation_0_cls = PointNetFeaturePropagation(in_channel=feat + 3, mlp=[self.trans_dim * 4, 1024])
        self.convs1_cls = nn.Conv1d(1024 + 2 * feat + 64, 512, 1)
        self.dp1 = nn.Dropout(0.5)
        self.convs2_cls = nn.Conv1d(512, 256, 1)
        self.convs3_cls = nn.Conv1d(256, self.cls_dim, 1)
        self.bns1_cls = nn.BatchNorm1d(512)
        self.bns2_cls = nn.BatchNorm1d(256)

    # ---- checkpoints ------------------------------------------------------------------------------------------------
    def load_segmentation_checkpoint(self, path, log=None):
        """A segmentation checkpoint of the reference (segmentation/main.py:303-312: a dict with model_state_dict), under
        this model's names or under the older ones without the `_cls` suffix (pt.py:264-285: every key the checkpoint
        lacks is looked up with `_cls` removed).  strict: nothing may be missing.  -> the names that were renamed."""
        log = log or logging.getLogger('Transformer').info
        ckpt = torch.load(path, map_location='cpu')
        if 'model_state_dict' not in ckpt:
            raise RuntimeError('%s: no model_state_dict (a pretraining checkpoint loads through load_model_from_ckpt)' % path)
        src = {k[len('module.'):] if k.startswith('module.') else k: v for k, v in ckpt['model_state_dict'].items()}
        state, renamed = {}, []
        for k in self.state_dict():
            if k in src:
                state[k] = src[k]
                continue
            old = k.replace('_cls', '')
            if old not in src:
                raise RuntimeError('%s: neither %s nor %s in the checkpoint' % (path, k, old))
            state[k] = src[old]
            renamed.append(k)
        self.load_state_dict(state, strict=True)
        if renamed:
            log('renamed from the layout without _cls: %d entries' % len(renamed))
        log(f'[Transformer] Successful Loading the ckpt from {path}')
        return renamed

    # ---- forward ----------------------------------------------------------------------------------------------------
    def trunk(self, pts, capture=None):
        """pts (B, N, 3) -> (centres (B, G, 3), F (B*G, 3C) = [tap3 | tap7 | tap11], each through the final norm)."""
        B, G, C = pts.shape[0], self.num_group, self.trans_dim
        neighborhood, center = self.group_divider(pts, capture)      # (capture also receives fps_idx, knn_idx)
        tokens = self.encoder(neighborhood)                                           # (B, G, C)
        pos = nn_ops.pos_embed(center.reshape(B * G, 3), self.pos_embed)
        x = tokens.reshape(B * G, C)
        keeps = nn_ops.stack_keeps(self.blocks, B)
        taps = []
        for i, (blk, k) in enumerate(zip(self.blocks.blocks, keeps)):
            x = blk(x, pos, B, G, k, pending=True)                   # nn_ops.Pending: the next norm adds the MLP branch
            if i in FETCH_IDX:
                taps.append(nn_ops.layer_norm(x, self.norm))
            if i == max(FETCH_IDX):
                break
        F = torch.cat(taps, dim=1)
        if capture is not None:
            capture.update(center=center, tokens=tokens, F=F)
        return center, F

    @torch.no_grad()
    def forward(self, pts, cls_label, seg=None, counts=None, capture=None):
        """pts (B, N, 3+), cls_label (B,) the category id (not a one-hot) -> log-probabilities (B, N, cls_dim) fp32.
        With seg (B, N) and counts (partseg_ops.Counts): -> (log-probabilities, pred (B, N) over each shape's own part
        range), the metric's counts added on the device."""
        name = type(self).__name__
        if self.training:
            raise NotImplementedError('%s: evaluation mode only -- part-segmentation training is not built' % name)
        if not pts.is_cuda:
            raise RuntimeError('%s: points must be on the GPU (there is no CPU path)' % name)
        if pts.shape[1] < self.group_size:
            raise ValueError('%s: %d points per cloud, fewer than group_size = %d' % (name, pts.shape[1], self.group_size))
        if cls_label.dim() != 1 or cls_label.shape[0] != pts.shape[0]:
            raise ValueError('%s: cls_label is the (B,) category id, not a one-hot' % name)
        pts = pts[:, :, :3].contiguous()
        begin_step(pts.device)
        center, F = self.trunk(pts, capture)
        logp, pred = partseg_ops.head(self, pts, center, F, cls_label.to(pts.device), seg, counts, capture)
        return logp if seg is None else (logp, pred)
