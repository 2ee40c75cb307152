"""Autograd wrappers of the classification fine-tuning glue (csrc/finetune.hip, include/pdae.h).

The fine-tuned classifier (point_transformer.py, models/Point_MAE.py:578-706 of the reference) reuses the pretraining
step's patch embedder and Transformer blocks; what it adds around them is here: the cls token / cls position in front of
the group tokens, the cls + max pooling of the final norm's output, the head's BatchNorm1d -> ReLU -> Dropout, the
softmax cross-entropy with the argmax hit count, and the global gradient-norm clip coefficient.  The DGCNN classifier
(dgcnn_cls.py) adds the LeakyReLU variant of the head's glue and the label-smoothed cross-entropy.  Every function raises
off the GPU: there is no CPU path.
"""
import torch

from . import _lib
from .rows import empty


def _gpu(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f'{what}: tensors must be on the GPU (there is no CPU path)')


class _PrependToken(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, token):
        B, G, C = x.shape
        out = empty((B, G + 1, C), x)
        _lib.call('pdae_prepend_token', x, B, G, C, _lib.ptr(x), _lib.ptr(token), _lib.ptr(out))
        ctx.dims = (B, G, C)
        return out

    @staticmethod
    def backward(ctx, g):
        B, G, C = ctx.dims
        g = g.contiguous()
        dx, dtok = empty((B, G, C), g), empty((1, 1, C), g)
        _lib.call('pdae_prepend_token_grad', g, B, G, C, _lib.ptr(g), _lib.ptr(dx), _lib.ptr(dtok))
        return dx, dtok


def prepend_token(x, token):
    """x (B, G, C), token (1, 1, C) -> (B, 1 + G, C) = per cloud [token | x]
    (torch.cat((token.expand(B, -1, -1), x), dim=1), Point_MAE.py:690-694)."""
    _gpu(x, 'prepend_token')
    return _PrependToken.apply(_lib.require(x.contiguous(), 'x', dim=3), _lib.require(token.contiguous(), 'token'))


class _ClsMaxConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, T, C = x.shape
        out, arg = empty((B, 2 * C), x), empty((B, C), x, torch.uint8)
        _lib.call('pdae_cls_max_concat', x, B, T, C, _lib.ptr(x), _lib.ptr(out), _lib.ptr(arg))
        ctx.save_for_backward(arg)
        ctx.T = T
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        g = g.contiguous()
        B, C = arg.shape
        dx = empty((B, ctx.T, C), g)
        _lib.call('pdae_cls_max_concat_grad', g, B, ctx.T, C, _lib.ptr(g), _lib.ptr(arg), _lib.ptr(dx))
        return dx


def cls_max_concat(x):
    """x (B, T, C) -> (B, 2C) = [x[:, 0] | x[:, 1:].max(1)[0]] (Point_MAE.py:698); ties go to the first token."""
    _gpu(x, 'cls_max_concat')
    return _ClsMaxConcat.apply(_lib.require(x.contiguous(), 'x', dim=3))


class _BnReluDropout(torch.autograd.Function):
    """slope None: pdae_bn_relu_dropout (ReLU); a float: pdae_bn_lrelu_dropout (LeakyReLU with that negative slope).
    training: 1 batch statistics (BatchNorm in training mode), 0 the running estimates and no dropout, 2 the running
    estimates under a live Dropout (a frozen BatchNorm inside a model in training mode, runner_finetune.set_bn_eval)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, bn, training, p, u, slope=None):
        B, N = y.shape
        out = empty((B, N), y)
        mean, invstd = empty((N,), y), empty((N,), y)      # batch statistics, or what the running estimates give
        track = bn.track_running_stats
        name, act = ('pdae_bn_relu_dropout', ()) if slope is None else ('pdae_bn_lrelu_dropout', (float(slope),))
        _lib.call(name, y, B, N, _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta), float(bn.eps),
                  float(bn.momentum), _lib.ptr(bn.running_mean) if track else None,
                  _lib.ptr(bn.running_var) if track else None,
                  _lib.ptr(bn.num_batches_tracked) if track else None, int(training), *act, float(p), _lib.ptr(u),
                  _lib.ptr(out), _lib.ptr(mean), _lib.ptr(invstd))
        ctx.save_for_backward(y, gamma, beta, mean, invstd, u)
        ctx.p, ctx.training, ctx.slope = p, training, slope
        return out

    @staticmethod
    def backward(ctx, g):
        what = 'bn_relu_dropout' if ctx.slope is None else 'bn_lrelu_dropout'
        y, gamma, beta, mean, invstd, u = ctx.saved_tensors
        g = g.contiguous()
        B, N = y.shape
        dy, dgamma, dbeta = empty((B, N), g), empty((N,), g), empty((N,), g)
        act = () if ctx.slope is None else (float(ctx.slope),)
        name = 'pdae_%s_%s' % (what, 'grad' if ctx.training == 1 else 'eval_grad')
        _lib.call(name, g, B, N, _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(invstd), *act,
                  float(ctx.p), _lib.ptr(u), _lib.ptr(g), _lib.ptr(dy), _lib.ptr(dgamma), _lib.ptr(dbeta))
        return dy, dgamma, dbeta, None, None, None, None, None


def _bn_act_dropout(what, y, bn, p, u, keep, slope, dropout=None):
    _gpu(y, what)
    if bn.momentum is None:
        raise NotImplementedError(what + ': cumulative moving average (momentum=None) is not supported')
    if not bn.affine:
        raise NotImplementedError(what + ': BatchNorm1d without affine parameters is not supported')
    if keep is not None:
        u = keep.to(torch.float32)              # 1.0 >= p keeps, 0.0 < p drops (0 < p < 1)
    if u is not None:
        u = _lib.require(u.contiguous(), 'u', dim=2)
        if tuple(u.shape) != tuple(y.shape):
            raise ValueError(f'{what}: the draw has shape {tuple(u.shape)}, the activation {tuple(y.shape)}')
    if dropout is None:
        dropout = bn.training
    if not dropout or p == 0:
        u = None
    mode = 1 if bn.training else (2 if u is not None else 0)
    return _BnReluDropout.apply(_lib.require(y.contiguous(), 'y', dim=2), bn.weight, bn.bias, bn, mode, p, u, slope)


def bn_relu_dropout(y, bn, p, u=None, keep=None, dropout=None):
    """Dropout(p)(ReLU(bn(y))) for y (B, N) and an nn.BatchNorm1d `bn`.  bn's mode decides the statistics: training-mode
    batch statistics and running-estimate updates, or the running estimates (nothing written).  `dropout` decides
    whether the draw applies -- the MODEL's training flag; None: bn's mode (a frozen BatchNorm inside a training-mode
    model, runner_finetune.set_bn_eval, keeps its Dropout live).  The draw is `u` (B, N uniforms: an element is kept
    when u >= p) or `keep` (a boolean keep mask, injected by tests); neither = no dropout."""
    return _bn_act_dropout('bn_relu_dropout', y, bn, p, u, keep, None, dropout)


def bn_lrelu_dropout(y, bn, p, slope, u=None, keep=None, dropout=None):
    """Dropout(p)(LeakyReLU(slope)(bn(y))), otherwise as bn_relu_dropout (the head of DGCNN, models/PointCAE_DGCNN.py:
    579-588; p = 0 for its first block, which has no Dropout).  0 <= slope < 1; slope 0 gives bn_relu_dropout's bits."""
    if not 0.0 <= float(slope) < 1.0:
        raise ValueError(f'bn_lrelu_dropout: 0 <= slope < 1 required, got {slope}')
    return _bn_act_dropout('bn_lrelu_dropout', y, bn, p, u, keep, float(slope), dropout)


class _SoftmaxXent(torch.autograd.Function):
    """eps None: pdae_softmax_xent (one-hot target); a float: pdae_softmax_xent_smooth (label smoothing eps)."""

    @staticmethod
    def forward(ctx, logits, labels, eps):
        B, K = logits.shape
        loss, correct = empty((), logits), empty((), logits)
        name, target = ('pdae_softmax_xent', ()) if eps is None else ('pdae_softmax_xent_smooth', (float(eps),))
        _lib.call(name, logits, B, K, *target, _lib.ptr(logits), _lib.ptr(labels), _lib.ptr(loss), _lib.ptr(correct))
        ctx.save_for_backward(logits, labels)
        ctx.name, ctx.target = name, target
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, dloss, _dcorrect):
        logits, labels = ctx.saved_tensors
        B, K = logits.shape
        dloss = dloss.contiguous()
        dl = empty((B, K), logits)
        _lib.call(ctx.name + '_grad', logits, B, K, *ctx.target, _lib.ptr(logits), _lib.ptr(labels), _lib.ptr(dloss),
                  _lib.ptr(dl))
        return dl, None, None


def softmax_xent(logits, labels):
    """nn.CrossEntropyLoss()(logits, labels) (mean, no label smoothing) for logits (B, K <= 64) and int64 labels in
    [0, K) -> (loss, correct): two device scalars, correct = the number of rows whose argmax (first on ties) is the label."""
    _gpu(logits, 'softmax_xent')
    labels = _lib.require(labels.to(torch.int64).contiguous(), 'labels', torch.int64, dim=1)
    return _SoftmaxXent.apply(_lib.require(logits.contiguous(), 'logits', dim=2), labels, None)


def softmax_xent_smooth(logits, labels, eps):
    """The label-smoothed cross-entropy of DGCNN.get_loss_acc with smoothloss (models/PointCAE_DGCNN.py:592-600):
    -(t * log_softmax(logits)).sum(1).mean() with t = one_hot (1 - eps) + (1 - one_hot) eps / (K - 1), for logits
    (B, 2 <= K <= 64) and int64 labels in [0, K) -> (loss, correct) as softmax_xent.  eps = 0 gives softmax_xent's bits."""
    _gpu(logits, 'softmax_xent_smooth')
    if not 0.0 <= float(eps) <= 1.0:
        raise ValueError(f'softmax_xent_smooth: 0 <= eps <= 1 required, got {eps}')
    labels = _lib.require(labels.to(torch.int64).contiguous(), 'labels', torch.int64, dim=1)
    return _SoftmaxXent.apply(_lib.require(logits.contiguous(), 'logits', dim=2), labels, float(eps))


class GradNormClip:
    """The coefficient torch.nn.utils.clip_grad_norm_(params, max_norm) multiplies the gradients by, for a flat fp32
    gradient buffer, on the device: coef = min(1, max_norm / (||g||_2 + 1e-6)).  The buffers are allocated once, so
    the launches can be captured in a graph."""

    def __init__(self, flat_grad, max_norm):
        _gpu(flat_grad, 'GradNormClip')
        self.grad = _lib.require(flat_grad, 'flat_grad', dim=1)
        self.max_norm = float(max_norm)
        parts = _lib.lib().pdae_grad_norm_parts(self.grad.numel())
        self.partials = torch.empty(parts, dtype=torch.float64, device=flat_grad.device)
        self.out = torch.empty(2, dtype=torch.float32, device=flat_grad.device)     # [norm, coef]
        self.norm, self.coef = self.out[0:1], self.out[1:2]

    def __call__(self):
        _lib.call('pdae_grad_norm_clip', self.grad, self.grad.numel(), _lib.ptr(self.grad), self.max_norm,
                  _lib.ptr(self.partials), _lib.ptr(self.norm), _lib.ptr(self.coef))
        return self.coef
