"""The skeleton the fine-tuned classifiers share (point_transformer.PointTransformer, dgcnn_cls.DGCNN): checkpoint
loading, weight init, the loss, and cls_head_finetune run on the HIP kernels.

A subclass builds its trunk and a cls_head_finetune Sequential of Linear layers and, between them, blocks of
BatchNorm1d -> ReLU or LeakyReLU [-> Dropout], and defines trunk(pts, capture) -> the feature the head takes.  The head's
Linear layers run on the row GEMMs (rows.linear_any), each block as ONE launch (finetune_ops.bn_relu_dropout /
bn_lrelu_dropout).  There is no CPU path.  forward_features is the guard every forward shares (the refusals, the
three-column slice, begin_step) in front of the trunk; the frozen feature extractors are trunks whose forward is that.
"""
import logging

import torch
import torch.nn as nn

from . import finetune_ops
from .arena import begin_step
from .point_cae_transformer import trunc_normal_
from .rows import linear_any


def _missing_message(keys):
    return 'Some model parameters or buffers are not found in the checkpoint:\n' + '\n'.join('  ' + k for k in keys)


def _unexpected_message(keys):
    return 'The checkpoint state_dict contains keys that are not used by the model:\n' + '\n'.join('  ' + k for k in keys)


def _per_dropout(t):
    """A tensor (a head with one Dropout) or a sequence with one tensor per Dropout -> a tuple."""
    return (t,) if isinstance(t, torch.Tensor) else tuple(t)


class Classifier(nn.Module):
    # the label smoothing eps of get_loss_acc; None: plain cross-entropy
    smooth_eps = None
    # None, or why the model cannot train under optimizer.part only_new (runner_finetune.set_bn_eval freezes a part of
    # its BatchNorms): the text of the NotImplementedError runner_finetune raises
    only_new_unsupported = None
    # whether the eval-mode model can be differentiated with respect to its input points (saliency_ops.input_gradients,
    # runner_finetune.vis_saliency_map): every link of its backward must carry a data gradient down to (B, N, 3)
    input_grad_supported = False
    # None, or for a model that is never trained the tail of forward_features' refusal in training mode:
    # '<class>: evaluation mode only -- <eval_only>'
    eval_only = None

    # ---- the reference's helpers ------------------------------------------------------------------------------------
    def get_loss_acc(self, ret, gt):
        """The cross-entropy (mean; against the label-smoothed target when smooth_eps is set) and the argmax accuracy in
        percent, both device scalars (Point_MAE.py:634-638, PointCAE_DGCNN.py:592-605)."""
        if self.smooth_eps is None:
            loss, correct = finetune_ops.softmax_xent(ret, gt)
        else:
            loss, correct = finetune_ops.softmax_xent_smooth(ret, gt, self.smooth_eps)
        return loss, correct * (100.0 / gt.shape[0])

    def load_model_from_ckpt(self, bert_ckpt_path, log=None):
        """Point_MAE.py:640-676, PointCAE_DGCNN.py:607-638: a pretraining checkpoint with its keys remapped, strict=False,
        the missing and unexpected keys logged; None = training from scratch (_init_weights).  -> the incompatible-keys
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
    def _init_weights(m):              # Point_MAE.py:678-690, PointCAE_DGCNN.py:640-652: Conv2d and BatchNorm keep torch's
        if isinstance(m, (nn.Linear, nn.Conv1d)):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _head_layers(self):
        """cls_head_finetune as a list of Linear layers and (BatchNorm1d, LeakyReLU slope or None for ReLU, Dropout p or
        None) blocks."""
        mods, layers, i = list(self.cls_head_finetune), [], 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear):
                layers.append(m)
                i += 1
                continue
            act = mods[i + 1] if i + 1 < len(mods) else None
            if not (isinstance(m, nn.BatchNorm1d) and isinstance(act, (nn.ReLU, nn.LeakyReLU))):
                raise NotImplementedError(f'{type(self).__name__}: cls_head_finetune[{i}] is neither a Linear nor a '
                                          'BatchNorm1d followed by ReLU / LeakyReLU')
            i += 2
            p = None
            if i < len(mods) and isinstance(mods[i], nn.Dropout):
                p = mods[i].p
                i += 1
            layers.append((m, act.negative_slope if isinstance(act, nn.LeakyReLU) else None, p))
        return layers

    def draw_dropout(self, B, device):
        """The uniforms of the head's Dropout layers, a (B, N) view each, from ONE torch.rand launch (graph-safe: a
        replay draws again from the device generator)."""
        ns = [layer[0].num_features for layer in self._head_layers() if isinstance(layer, tuple) and layer[2] is not None]
        u = torch.rand(B * sum(ns), device=device)
        views, a = [], 0
        for n in ns:
            views.append(u[B * a:B * (a + n)].view(B, n))
            a += n
        return tuple(views)

    def head(self, f, drop=None, drop_keep=None):
        """cls_head_finetune on the trunk's feature f (B, F).  drop: the uniforms of its Dropout layers (draw_dropout);
        drop_keep: their boolean keep masks (tests); each a tuple with one tensor per Dropout or, with one Dropout, the
        tensor; neither in training mode: a fresh draw."""
        us = keeps = None
        if self.training:
            if drop_keep is not None:
                keeps = _per_dropout(drop_keep)
            else:
                us = _per_dropout(drop) if drop is not None else self.draw_dropout(f.shape[0], f.device)
        x, j = f, 0
        for layer in self._head_layers():
            if isinstance(layer, nn.Linear):
                x = linear_any(x, layer.weight, layer.bias)
                continue
            bn, slope, p = layer
            u = keep = None
            if p is None:                  # a block without Dropout
                p = 0.0
            else:
                u = us[j] if us is not None else None
                keep = keeps[j] if keeps is not None else None
                j += 1
            if slope is None:
                x = finetune_ops.bn_relu_dropout(x, bn, p, u=u, keep=keep, dropout=self.training)
            else:
                x = finetune_ops.bn_lrelu_dropout(x, bn, p, slope, u=u, keep=keep, dropout=self.training)
        return x

    def forward_features(self, pts, capture=None):
        """pts (B, N, 3+) -> the trunk's feature; capture: a dict the trunk fills with its intermediates (tests).  This is
        the whole forward of a frozen feature extractor (a trunk without a head)."""
        if self.training and self.eval_only is not None:
            raise NotImplementedError(f'{type(self).__name__}: evaluation mode only -- {self.eval_only}')
        if not pts.is_cuda:
            raise RuntimeError(f'{type(self).__name__}: points must be on the GPU (there is no CPU path)')
        pts = pts[:, :, :3].contiguous()
        begin_step(pts.device)
        return self.trunk(pts, capture)

    def forward(self, pts, drop=None, drop_keep=None, capture=None):
        """pts (B, N, 3+) -> logits (B, cls_dim)."""
        return self.head(self.forward_features(pts, capture), drop, drop_keep)
