"""Classification fine-tuning model, MI355X host side (models/Point_MAE.py:578-706 PointTransformer of the reference).

Same parameter names and shapes as the reference, so a pretraining checkpoint of this repository loads through
builder.remap_pretrain_keys (the 'MAE_encoder.' prefix dropped) with strict=False, reporting the same missing and
unexpected keys:

    model = MODELS.build(cfg.model)              # cfg.model.NAME == 'PointTransformer'
    model.load_model_from_ckpt(path_or_None)
    logits = model(points)                       # (B, cls_dim)
    loss, acc = model.get_loss_acc(logits, labels)

The trunk is the pretraining step's: FPS + kNN grouping, the fused patch embedder on every group, pos_embed, the pre-LN
blocks on flat (B*T, C) rows with T = num_group + 1 (the cls token), the final LayerNorm.  Around it the glue of
csrc/finetune.hip (finetune_ops.py): cls token / cls position assembly, cls + max pooling, the head's BatchNorm1d -> ReLU
-> Dropout, the softmax cross-entropy.  The head's Linear layers run on the row GEMMs (nn_ops.linear_any).  There is no
CPU path.
"""
import logging

import torch
import torch.nn as nn

from . import finetune_ops, nn_ops
from .point_cae_transformer import Encoder, Group, TransformerEncoder, _pos_embed, trunc_normal_
from .registry import MODELS

MAX_TOKENS = 128           # the attention kernels take T <= 128 tokens per cloud (csrc/attention.hip)


def _missing_message(keys):
    return 'Some model parameters or buffers are not found in the checkpoint:\n' + '\n'.join('  ' + k for k in keys)


def _unexpected_message(keys):
    return 'The checkpoint state_dict contains keys that are not used by the model:\n' + '\n'.join('  ' + k for k in keys)


@MODELS.register_module()
class PointTransformer(nn.Module):
    # parameters whose gradients backward produces last (FlatDataParallel lays them at the end of the flat buffer)
    late_grad_prefixes = ('encoder.',)

    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.trans_dim = config.trans_dim
        self.depth = config.depth
        self.drop_path_rate = config.drop_path_rate
        self.cls_dim = config.cls_dim
        self.num_heads = config.num_heads
        self.group_size = config.group_size
        self.num_group = config.num_group
        self.encoder_dims = config.encoder_dims
        if self.num_group + 1 > MAX_TOKENS:
            raise NotImplementedError(
                'PointTransformer: num_group + 1 = %d tokens per cloud; the attention kernels take at most %d'
                % (self.num_group + 1, MAX_TOKENS))
        if self.encoder_dims != self.trans_dim:
            raise NotImplementedError('PointTransformer: encoder_dims must equal trans_dim (the tokens feed the blocks)')
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, self.trans_dim))
        self.cls_pos = nn.Parameter(torch.randn(1, 1, self.trans_dim))
        self.pos_embed = _pos_embed(self.trans_dim)
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(self.trans_dim, self.depth, self.num_heads, dpr)
        self.norm = nn.LayerNorm(self.trans_dim)
        self.cls_head_finetune = nn.Sequential(
            nn.Linear(self.trans_dim * 2, 512), nn.BatchNorm1d(512), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))
        trunc_normal_(self.cls_token, std=.02)
        trunc_normal_(self.cls_pos, std=.02)

    # ---- the reference's helpers ------------------------------------------------------------------------------------
    def get_loss_acc(self, ret, gt):
        """nn.CrossEntropyLoss()(ret, gt) and the argmax accuracy in percent, both device scalars (Point_MAE.py:634-638)."""
        loss, correct = finetune_ops.softmax_xent(ret, gt)
        return loss, correct * (100.0 / gt.shape[0])

    def load_model_from_ckpt(self, bert_ckpt_path, log=None):
        """Point_MAE.py:640-676: a pretraining checkpoint with its encoder keys remapped, strict=False, the missing and
        unexpected keys logged; None = training from scratch (trunc-normal init).  -> the incompatible-keys record
        (None from scratch)."""
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
    def _init_weights(m):              # Point_MAE.py:678-690
        if isinstance(m, (nn.Linear, nn.Conv1d)):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def draw_dropout(self, B, device):
        """The head's two dropout draws from ONE torch.rand launch: (u1 (B, 512), u2 (B, 256)), each contiguous
        (graph-safe: a replay draws again from the device generator)."""
        h = self.cls_head_finetune
        n1, n2 = h[0].out_features, h[4].out_features
        u = torch.rand(B * (n1 + n2), device=device)
        return u[:B * n1].view(B, n1), u[B * n1:].view(B, n2)

    def head(self, f, drop=None, drop_keep=None):
        """cls_head_finetune on the pooled feature f (B, 2C).  drop: (u1, u2) uniforms; drop_keep: (keep1, keep2)
        boolean keep masks (tests); neither in training mode: a fresh draw."""
        h = self.cls_head_finetune
        B = f.shape[0]
        u1 = u2 = k1 = k2 = None
        if self.training:
            if drop_keep is not None:
                k1, k2 = drop_keep
            else:
                u1, u2 = drop if drop is not None else self.draw_dropout(B, f.device)
        x = nn_ops.linear_any(f, h[0].weight, h[0].bias)
        x = finetune_ops.bn_relu_dropout(x, h[1], h[3].p, u=u1, keep=k1)
        x = nn_ops.linear_any(x, h[4].weight, h[4].bias)
        x = finetune_ops.bn_relu_dropout(x, h[5], h[7].p, u=u2, keep=k2)
        return nn_ops.linear_any(x, h[8].weight, h[8].bias)

    def forward(self, pts, drop=None, drop_keep=None, capture=None):
        """pts (B, N, 3+) -> logits (B, cls_dim) (Point_MAE.py:692-706)."""
        if not pts.is_cuda:
            raise RuntimeError('PointTransformer: points must be on the GPU (there is no CPU path)')
        pts = pts[:, :, :3].contiguous()
        B = pts.shape[0]
        G, C = self.num_group, self.trans_dim
        T = G + 1
        nn_ops.begin_step(pts.device)
        neighborhood, center = self.group_divider(pts)
        tokens = self.encoder(neighborhood)                                           # (B, G, C), every group
        pos = nn_ops.pos_embed(center.reshape(B * G, 3), self.pos_embed).reshape(B, G, C)
        x = finetune_ops.prepend_token(tokens, self.cls_token).reshape(B * T, C)
        pos = finetune_ops.prepend_token(pos, self.cls_pos).reshape(B * T, C)
        x = self.blocks(x, pos, B, T)                    # nn_ops.Pending: the final norm's kernel adds the last branch
        x = nn_ops.layer_norm(x, self.norm).reshape(B, T, C)
        f = finetune_ops.cls_max_concat(x)                                            # (B, 2C)
        if capture is not None:
            capture.update(center=center, tokens=tokens, x=x, feature=f)
        return self.head(f, drop, drop_keep)
