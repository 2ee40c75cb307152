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
Linear layers on the row GEMMs (rows.linear_any) and each BatchNorm + LeakyReLU [+ Dropout] as one launch
(finetune_ops.bn_lrelu_dropout); the loss is finetune_ops.softmax_xent_smooth (smoothloss) or softmax_xent.  There is
no CPU path.

DGCNN_feat (models/PointCAE_DGCNN.py:755-846) is the same encoder without the head: forward returns the (B, 1024) feature
the linear-SVM evaluation protocol fits its classifiers on (runner_finetune.svm_classification).
"""
import torch.nn as nn

from .classifier import Classifier
from .point_cae_dgcnn import dgcnn_encoder
from .registry import MODELS

SMOOTH_EPS = 0.3           # get_loss_acc's label smoothing (PointCAE_DGCNN.py:594)
LRELU_SLOPE = 0.2


@MODELS.register_module()
class DGCNN(Classifier):
    # parameters whose gradients backward produces last (FlatDataParallel lays them at the end of the flat buffer)
    late_grad_prefixes = ('dgcnn_encoder.',)
    only_new_unsupported = ("set_bn_eval leaves dgcnn_encoder.bn4 (256 channels) in training mode beside frozen "
                            "BatchNorms, and dgcnn_encoder's single autograd node differentiates training-mode "
                            "BatchNorm only")

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

    @property
    def smooth_eps(self):
        """get_loss_acc's label smoothing (PointCAE_DGCNN.py:592-605): eps 0.3 with smoothloss, else F.cross_entropy."""
        return SMOOTH_EPS if self.smoothing else None

    def trunk(self, pts, capture):
        """pts (B, N, 3) -> the encoder's feature (B, 1024) (PointCAE_DGCNN.py:654-661)."""
        f = self.dgcnn_encoder.forward_rows(pts)
        if capture is not None:
            capture.update(feature=f)
        return f


@MODELS.register_module()
class DGCNN_feat(DGCNN):
    """The frozen feature extractor of --svm_classification: dgcnn_encoder and nothing else that carries parameters, so a
    Point_CAE_DGCNN_FCOnly checkpoint loads with recfc.* unexpected and nothing missing.  get_loss_acc,
    load_model_from_ckpt and _init_weights are the classifier's (the reference's class carries the same copies)."""

    def __init__(self, config, **kwargs):
        super().__init__(config, **kwargs)
        del self.cls_head_finetune

    forward = Classifier.forward_features      # pts (B, N, 3+) -> the encoder's feature (B, 1024); gradients are recorded
