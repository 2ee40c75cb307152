"""Classification fine-tuning models, MI355X host side (models/Point_MAE.py:578-706 PointTransformer and :846-966
PointTransformerLinearClassification of the reference; the two differ in cls_head_finetune only; :970-1092
PointTransformerNoClassTokenSVMFeature, the frozen feature extractor of --svm_classification).

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
-> Dropout, the softmax cross-entropy.  The head's Linear layers run on the row GEMMs (rows.linear_any).  There is no
CPU path.
"""
import torch
import torch.nn as nn

from . import finetune_ops, nn_ops
from .classifier import Classifier
from .point_cae_transformer import Encoder, Group, TransformerEncoder, pos_embed_layers, trunc_normal_
from .registry import MODELS

MAX_TOKENS = 128           # the attention kernels take T <= 128 tokens per cloud (csrc/attention.hip)


class _TransformerClassifier(Classifier):
    """The trunk both classifiers share; a subclass gives build_head() -> cls_head_finetune."""
    # parameters whose gradients backward produces last (FlatDataParallel lays them at the end of the flat buffer)
    late_grad_prefixes = ('encoder.',)
    # grouping, the position embedding and the eval-mode patch embedder carry a gradient down to the points
    input_grad_supported = True

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
                '%s: num_group + 1 = %d tokens per cloud; the attention kernels take at most %d'
                % (type(self).__name__, self.num_group + 1, MAX_TOKENS))
        if self.encoder_dims != self.trans_dim:
            raise NotImplementedError('%s: encoder_dims must equal trans_dim (the tokens feed the blocks)'
                                      % type(self).__name__)
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, self.trans_dim))
        self.cls_pos = nn.Parameter(torch.randn(1, 1, self.trans_dim))
        self.pos_embed = pos_embed_layers(self.trans_dim)
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(self.trans_dim, self.depth, self.num_heads, dpr)
        self.norm = nn.LayerNorm(self.trans_dim)
        self.cls_head_finetune = self.build_head()
        trunc_normal_(self.cls_token, std=.02)
        trunc_normal_(self.cls_pos, std=.02)

    def trunk(self, pts, capture):
        """pts (B, N, 3) -> the pooled feature (B, 2C) (Point_MAE.py:692-698)."""
        B = pts.shape[0]
        G, C = self.num_group, self.trans_dim
        T = G + 1
        neighborhood, center = self.group_divider(pts, capture)      # (capture also receives fps_idx, knn_idx)
        tokens = self.encoder(neighborhood)                                           # (B, G, C), every group
        pos = nn_ops.pos_embed(center.reshape(B * G, 3), self.pos_embed).reshape(B, G, C)
        return self.trunk_from_tokens(tokens, pos, center, capture)

    def trunk_from_tokens(self, tokens, pos, center=None, capture=None):
        """tokens (B, G, C), their position embedding (B, G, C) -> the pooled feature (B, 2C)."""
        B, G, C = tokens.shape
        T = G + 1
        x = finetune_ops.prepend_token(tokens, self.cls_token).reshape(B * T, C)
        pos = finetune_ops.prepend_token(pos, self.cls_pos).reshape(B * T, C)
        x = self.blocks(x, pos, B, T)                    # nn_ops.Pending: the final norm's kernel adds the last branch
        x = nn_ops.layer_norm(x, self.norm).reshape(B, T, C)
        f = finetune_ops.cls_max_concat(x)                                            # (B, 2C)
        if capture is not None:
            capture.update(center=center, tokens=tokens, x=x, feature=f)
        return f


@MODELS.register_module()
class PointTransformer(_TransformerClassifier):
    """Point_MAE.py:578-706: the MLP head (full fine-tuning, and the non-linear protocol on a frozen encoder)."""

    def build_head(self):
        return nn.Sequential(
            nn.Linear(self.trans_dim * 2, 512), nn.BatchNorm1d(512), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))


@MODELS.register_module()
class PointTransformerLinearClassification(_TransformerClassifier):
    """Point_MAE.py:846-966: one Linear(2C, cls_dim) on the pooled feature (the linear protocol on a frozen encoder)."""

    def build_head(self):
        return nn.Sequential(nn.Linear(self.trans_dim * 2, self.cls_dim))


@MODELS.register_module()
class PointTransformerNoClassTokenSVMFeature(Classifier):
    """Point_MAE.py:970-1092: the trunk without cls_token / cls_pos and without a head, T = num_group tokens per cloud;
    the feature is max + mean over the normed tokens (:1092), what --svm_classification fits its SVMs on.  A Transformer
    pretraining checkpoint loads with its decoder keys unexpected and nothing missing.  get_loss_acc, load_model_from_ckpt
    and _init_weights are the classifier's (the reference's class carries copies).  Never trained: forward only,
    evaluation mode only, no CPU path."""
    late_grad_prefixes = ()
    eval_only = ('the frozen feature extractor of the linear-SVM protocol; PointTransformerNoClassToken fine-tuning is '
                 'not built')

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
        if self.num_group > MAX_TOKENS:
            raise NotImplementedError('PointTransformerNoClassTokenSVMFeature: num_group = %d tokens per cloud; the '
                                      'attention kernels take at most %d' % (self.num_group, MAX_TOKENS))
        if self.encoder_dims != self.trans_dim:
            raise NotImplementedError('PointTransformerNoClassTokenSVMFeature: encoder_dims must equal trans_dim (the '
                                      'tokens feed the blocks)')
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.pos_embed = pos_embed_layers(self.trans_dim)
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(self.trans_dim, self.depth, self.num_heads, dpr)
        self.norm = nn.LayerNorm(self.trans_dim)

    forward = torch.no_grad()(Classifier.forward_features)

    def trunk(self, pts, capture):
        """pts (B, N, 3) -> the feature (B, trans_dim)."""
        B, G, C = pts.shape[0], self.num_group, self.trans_dim
        neighborhood, center = self.group_divider(pts, capture)      # (capture also receives fps_idx, knn_idx)
        tokens = self.encoder(neighborhood)                                           # (B, G, C)
        pos = nn_ops.pos_embed(center.reshape(B * G, 3), self.pos_embed)
        x = self.blocks(tokens.reshape(B * G, C), pos, B, G)         # nn_ops.Pending: the final norm adds the last branch
        x = nn_ops.layer_norm(x, self.norm).reshape(B, G, C)
        f = nn_ops.max_plus_mean(x)
        if capture is not None:
            capture.update(center=center, tokens=tokens, x=x, feature=f)
        return f
