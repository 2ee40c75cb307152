"""DGCNN part segmentation on ShapeNetPart, MI355X host side: the reference's other segmentation network
(segmentation/models/dgcnn_partseg.py get_model on dgcnn_encoder_partseg, segmentation/models/dgcnn_util.py:140-193) in
evaluation mode, forward only.

Same parameter and buffer names and shapes as the reference's get_model(50) -- bn1..bn6 of the encoder and bn7..bn10 of the
head are registered directly AND inside their conv Sequentials, so the state_dict carries both key sets, as the
reference's does --, so its segmentation checkpoints load (load_segmentation_checkpoint: strict, no renaming), and a
pretraining checkpoint with a dgcnn_encoder.* of this layout loads through the inherited load_model_from_ckpt with the
head missing and the decoder unexpected.

    model = MODELS.build(cfg.model)                         # cfg.model.NAME == 'DGCNNPartSeg'
    model.load_segmentation_checkpoint(path)
    logits = model(points, cls_label)                       # (B, N, 50) raw logits, fp32 (this network has no log-softmax)

PDAE_PARTSEG=hip.  Activations are rows (points) x channels.
  Encoder.  The three graphs are rebuilt in the space of each EdgeConv's input (point_cae_dgcnn.feature_knn).  The first
  layer of every EdgeConv is conv([x_j - x_i, x_i]) = p[j] + q[i]: one row GEMM per POINT on the stacked weight
  [W1; W2 - W1].  EdgeConvs 1 and 2 are two layers deep (conv1 + conv2, conv3 + conv4): pdae_edge2_eval_forward
  (csrc/edge2_eval.hip) gathers p, forms the first layer's activation in LDS, runs the 64 x 64 second layer on
  fp32-input MFMA tiles and takes the max over the k edges on chip -- no (B N k, 64) tensor exists.  EdgeConv 3 (conv5)
  is one layer: pdae_edge_gather_stats picks the winning edge by the sign of gamma, pdae_bn_lrelu_rows applies the
  affine.  Every x_i is written a second time into the (B N, 192) concatenation; conv6 runs on the row GEMM, its
  BatchNorm + LeakyReLU + max over the points as pdae_cloud_pool_stats + pdae_bn_lrelu_rows.
  Head.  Two identities, exact in real arithmetic: (a) conv8's 1088 columns [global feature | label feature] are the
  same for every point of a cloud: one (B, 1088) product gives a per-cloud bias, added where the layer's LeakyReLU is
  applied (pdae_partseg_cloud_bias_lrelu) behind the 192 per-point columns on the row GEMM, bn8's scale folded into the
  weight; the label feature is conv7 on a one-hot = column cls of its weight; (b) bn10 + LeakyReLU + conv11 + the
  range-restricted argmax + the metric's counts are one pass over a 128-wide row (pdae_partseg_logits_tail).  No
  (B N, 1280) tensor exists.  Dropout is the identity in evaluation mode.

PDAE_PARTSEG=layers keeps the model as the reference writes it -- the per-edge tensor by index gather, five EdgeConv
layers and the concatenations -- on kernels that predate csrc/edge2_eval.hip plus framework glue: the fallback for
layouts the new entries refuse, the error yardstick of the tests and the timing baseline of
tools/bench_dgcnn_partseg.py.  There is no CPU path and no training.
"""
import logging
import os

import torch
import torch.nn as nn

from . import _lib, partseg_ops
from .arena import begin_step
from .classifier import Classifier
from .point_cae_dgcnn import K_GRAPH, feature_knn
from .registry import MODELS
from .rows import bn_eval_affine, empty, linear_any, rows_gemm

LRELU_SLOPE = 0.2
# of PDAE_PARTSEG for this model.  The issue's rule: hip stays the default only if the whole forward beats layers by more than
# the baseline's spread -- tools/bench_dgcnn_partseg.py, 16 x 2048 points: the figures stand in DESIGN.md 7
DEFAULT_MODE = 'hip'
XYZ_TOPK_MAX = 6144        # pdae_xyz_topk keeps a cloud in LDS


def mode():
    """PDAE_PARTSEG for this model: 'hip' or 'layers'."""
    m = os.environ.get('PDAE_PARTSEG', DEFAULT_MODE)
    if m not in partseg_ops.MODES:
        raise ValueError('PDAE_PARTSEG=%s: expected one of %s' % (m, ', '.join(partseg_ops.MODES)))
    return m


def _act():
    return nn.LeakyReLU(negative_slope=LRELU_SLOPE)


class dgcnn_encoder_partseg(nn.Module):
    """The parameters of segmentation/models/dgcnn_util.py:140-167; the forward is DGCNNPartSeg.encode."""

    def __init__(self, channel=3):
        super().__init__()
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm2d(64), nn.BatchNorm2d(64), nn.BatchNorm2d(64)
        self.bn4, self.bn5, self.bn6 = nn.BatchNorm2d(64), nn.BatchNorm2d(64), nn.BatchNorm1d(1024)
        self.conv1 = nn.Sequential(nn.Conv2d(channel * 2, 64, kernel_size=1, bias=False), self.bn1, _act())
        self.conv2 = nn.Sequential(nn.Conv2d(64, 64, kernel_size=1, bias=False), self.bn2, _act())
        self.conv3 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn3, _act())
        self.conv4 = nn.Sequential(nn.Conv2d(64, 64, kernel_size=1, bias=False), self.bn4, _act())
        self.conv5 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn5, _act())
        self.conv6 = nn.Sequential(nn.Conv1d(192, 1024, kernel_size=1, bias=False), self.bn6, _act())


# ---- the kernels' wrappers ---------------------------------------------------------------------------------------------
def edge2_supported(k, C1=64, C2=64):
    return bool(_lib.lib().pdae_edge2_eval_supported(int(k), int(C1), int(C2)))


def edge2_eval(pq, idx, scale1, shift1, w2, scale2, shift2, out2=None, col=0):
    """pdae_edge2_eval_forward: pq (B*N, 2 C1) = [p | q], idx (B, N, k) int32 -> (B*N, C2); out2 (B*N, W) receives a second
    copy in its columns col .. col + C2.  RuntimeError when the layout is refused."""
    B, N, k = idx.shape
    C2, C1 = w2.shape
    pq, idx, scale1, shift1, w2, scale2, shift2 = (t.contiguous() for t in (pq, idx, scale1, shift1, w2, scale2, shift2))
    out = empty((B * N, C2), pq)
    _lib.call('pdae_edge2_eval_forward', pq, B, N, k, C1, C2, _lib.ptr(pq), _lib.ptr(idx), _lib.ptr(scale1),
              _lib.ptr(shift1), _lib.ptr(w2), _lib.ptr(scale2), _lib.ptr(shift2), _lib.ptr(out),
              out2.data_ptr() + 4 * col if out2 is not None else None, out2.shape[1] if out2 is not None else 0)
    return out


def bn_lrelu_rows(e, scale, shift, out2=None, col=0):
    """pdae_bn_lrelu_rows: lrelu(e scale + shift), slope 0.2, on (R, C) rows [+ a second copy into out2's columns]."""
    R, C = e.shape
    out = empty((R, C), e)
    _lib.call('pdae_bn_lrelu_rows', e, R, C, _lib.ptr(e), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(out),
              out2.data_ptr() + 4 * col if out2 is not None else None, out2.shape[1] if out2 is not None else 0)
    return out


def cloud_bias_lrelu(y, gbias, B, N, slope=LRELU_SLOPE):
    """y (B*N, C) <- lrelu(y + gbias[b]) in place."""
    gbias = gbias.contiguous()
    _lib.call('pdae_partseg_cloud_bias_lrelu', y, B, N, y.shape[1], _lib.ptr(y), _lib.ptr(gbias), float(slope))
    return y


def logits_tail(y, scale, shift, w, bias, S, N, seg=None, lo=None, hi=None, counts=None, slope=LRELU_SLOPE):
    """pdae_partseg_logits_tail on y (S*N, 128) -> (logits (S*N, 50), pred (S*N,) int32); with seg (S, N) and counts the
    counts of these S shapes are added at counts.filled."""
    y, scale, shift, w = (t.contiguous() for t in (y, scale, shift, w))
    bias = bias.contiguous() if bias is not None else None
    logits = empty((S * N, w.shape[0]), y)
    pred = empty((S * N,), y, torch.int32)
    iu = sc = seen = correct = None
    if seg is not None:
        if counts is None or lo is None or hi is None:
            raise ValueError('partseg logits tail: seg goes with counts and the part ranges')
        seg = seg.to(torch.int32).contiguous()
        f = counts.filled
        if f + S > counts.shape_correct.shape[0]:
            raise ValueError('partseg logits tail: the counts hold %d shapes' % counts.shape_correct.shape[0])
        iu, sc = counts.shape_iu[f:f + S], counts.shape_correct[f:f + S]
        seen, correct = counts.part_seen, counts.part_correct
    _lib.call('pdae_partseg_logits_tail', y, S, N, y.shape[1], w.shape[0], _lib.ptr(y), _lib.ptr(scale), _lib.ptr(shift),
              float(slope), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(seg), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(logits),
              _lib.ptr(pred), _lib.ptr(iu), _lib.ptr(sc), _lib.ptr(seen), _lib.ptr(correct))
    return logits, pred


def _w(conv):
    return conv.weight.reshape(conv.weight.shape[0], -1)


@MODELS.register_module()
class DGCNNPartSeg(Classifier):
    """segmentation/models/dgcnn_partseg.py:10-140.  Never trained here: forward only, evaluation mode only."""
    late_grad_prefixes = ()

    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.cls_dim = config.get('cls_dim', 50)
        self.num_categories = config.get('num_categories', 16)
        self.dgcnn_encoder = dgcnn_encoder_partseg(channel=3)
        self.part_num = self.cls_dim
        self.bn7, self.bn8 = nn.BatchNorm1d(64), nn.BatchNorm1d(256)
        self.bn9, self.bn10 = nn.BatchNorm1d(256), nn.BatchNorm1d(128)
        self.conv7 = nn.Sequential(nn.Conv1d(self.num_categories, 64, kernel_size=1, bias=False), self.bn7, _act())
        self.conv8 = nn.Sequential(nn.Conv1d(1280, 256, kernel_size=1, bias=False), self.bn8, _act())
        self.dp1 = nn.Dropout(p=0.5)
        self.conv9 = nn.Sequential(nn.Conv1d(256, 256, kernel_size=1, bias=False), self.bn9, _act())
        self.dp2 = nn.Dropout(p=0.5)
        self.conv10 = nn.Sequential(nn.Conv1d(256, 128, kernel_size=1, bias=False), self.bn10, _act())
        self.conv11 = nn.Conv1d(128, self.part_num, kernel_size=1, bias=False)

    def fusable(self, k=K_GRAPH):
        """Whether the new entries take this model's layout: k neighbours, 64-wide EdgeConv layers, a 128 -> 50 last layer."""
        return (edge2_supported(k) and self.conv11.weight.shape[0] == partseg_ops.NUM_PART
                and self.conv11.weight.shape[1] == 128)

    def partseg_mode(self, k=K_GRAPH):
        """The backend forward RUNS (what runner_finetune.part_seg_test prints): PDAE_PARTSEG, and `layers` wherever the
        new entries refuse the layout."""
        return 'hip' if mode() == 'hip' and self.fusable(k) else 'layers'

    # ---- the hip form's constant operands ---------------------------------------------------------------------------
    def prepared(self):
        """The operands of the hip form that depend on the weights alone -- the stacked EdgeConv weights [W1; W2 - W1], every
        BatchNorm's evaluation affine, conv8 with bn8's scale folded in and cut into its per-cloud and per-point columns,
        the contiguous 2-D views of the other weights -- made once and kept until a parameter or buffer changes (its
        version counter or its storage: load_state_dict, .to(), an optimiser step)."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        hit = getattr(self, '_prepared', None)
        if hit is not None and hit[0] == key:
            return hit[1]
        enc = self.dgcnn_encoder
        firsts = (enc.conv1, enc.conv3, enc.conv5)
        like = enc.conv1[0].weight
        cos, cins, kps = [64, 64, 64], [3, 64, 64], [4, 64, 64]
        stacked = [empty((2 * co, kp), like) for co, kp in zip(cos, kps)]
        _lib.edge_weights_multi('pdae_edge_weight_stack_multi', like, cos, cins, kps,
                                [c[0].weight.detach().contiguous() for c in firsts], stacked)
        P = {'stacked': stacked}
        for name, bn in (('1', enc.bn1), ('2', enc.bn2), ('3', enc.bn3), ('4', enc.bn4), ('5', enc.bn5), ('6', enc.bn6),
                         ('7', self.bn7), ('8', self.bn8), ('9', self.bn9), ('10', self.bn10)):
            P['s' + name], P['t' + name] = (t.detach() for t in bn_eval_affine(bn)[:2])
        n_glob = 1024 + self.conv7[0].weight.shape[0]
        w8 = _w(self.conv8[0]).detach() * P['s8'][:, None]
        P['w8_glob'], P['w8_point'] = w8[:, :n_glob].contiguous(), w8[:, n_glob:].contiguous()
        for name, conv in (('w2', enc.conv2[0]), ('w4', enc.conv4[0]), ('w6', enc.conv6[0]), ('w9', self.conv9[0]),
                           ('w10', self.conv10[0]), ('w11', self.conv11)):
            P[name] = _w(conv).detach().contiguous()
        self._prepared = (key, P)
        return P

    # ---- checkpoints ------------------------------------------------------------------------------------------------
    def load_segmentation_checkpoint(self, path, log=None):
        """A segmentation checkpoint of the reference (segmentation/main.py:303-312: a dict with model_state_dict), with
        or without the `module.` prefix.  strict: nothing may be missing or unexpected.  -> [] (nothing is renamed)."""
        log = log or logging.getLogger('Transformer').info
        ckpt = torch.load(path, map_location='cpu')
        if 'model_state_dict' not in ckpt:
            raise RuntimeError('%s: no model_state_dict (a pretraining checkpoint loads through load_model_from_ckpt)' % path)
        src = {k[len('module.'):] if k.startswith('module.') else k: v for k, v in ckpt['model_state_dict'].items()}
        self.load_state_dict(src, strict=True)
        log(f'[DGCNNPartSeg] Successful Loading the ckpt from {path}')
        return []

    # ---- the encoder ------------------------------------------------------------------------------------------------
    def _graph(self, li, x, B, N, k, graphs, own, used, want_own):
        """The graph of EdgeConv li: the model's own selection on the features at hand, or graphs[li]."""
        if graphs is None or want_own:
            feature_knn(x, B, N, k, out=own[li], xyz=(li == 0 and N <= XYZ_TOPK_MAX))
        if graphs is None:
            return own[li]
        used[li].copy_(graphs[li])
        return used[li]

    def encode(self, pts, fused, graphs=None, capture=None):
        """pts (B, N, 3) -> (cat (B*N, 192) = [x1 | x2 | x3], g (B, 1024)) (dgcnn_util.py:169-193)."""
        enc = self.dgcnn_encoder
        B, N, _ = pts.shape
        R, k = B * N, min(K_GRAPH, N)
        want_own = capture is not None
        own = empty((3, B, N, k), pts, torch.int32)
        used = empty((3, B, N, k), pts, torch.int32) if graphs is not None else own
        x = empty((R, 4), pts)
        _lib.call('pdae_rows_pad', pts, R, 3, 4, _lib.ptr(pts), _lib.ptr(x))
        cat = empty((R, 192), pts)
        firsts = (enc.conv1, enc.conv3, enc.conv5)
        seconds = (enc.conv2, enc.conv4, None)
        P = self.prepared() if fused else None
        xs = []
        for li in range(3):
            idx = self._graph(li, x, B, N, k, graphs, own, used, want_own)
            if not fused:
                s1, t1, _, _ = bn_eval_affine(firsts[li][1])
                x = self._edgeconv_layers(x, idx, li, firsts[li], seconds[li], s1, t1, cat)
                xs.append(x)
                continue
            f, sc = str(2 * li + 1), str(2 * li + 2)                 # conv1 + conv2, conv3 + conv4, conv5
            s1, t1 = P['s' + f], P['t' + f]
            pq = rows_gemm(x, P['stacked'][li])
            if seconds[li] is not None:
                x = edge2_eval(pq, idx, s1, t1, P['w' + sc], P['s' + sc], P['t' + sc], out2=cat, col=64 * li)
            else:
                co = 64
                esel, psum, sel = empty((R, co), x), empty((R, co), x), empty((R, co), x, torch.int16)
                part = empty((_lib.lib().pdae_edge_parts(), 2 * co), x, torch.float64)
                sums = empty((2 * co,), x, torch.float64)
                _lib.call('pdae_edge_gather_stats', x, B, N, k, co, _lib.ptr(pq), _lib.ptr(idx.contiguous()),
                          _lib.ptr(firsts[li][1].weight), _lib.ptr(esel), _lib.ptr(sel), _lib.ptr(psum), _lib.ptr(part),
                          _lib.ptr(sums))
                x = bn_lrelu_rows(esel, s1, t1, out2=cat, col=64 * li)
            xs.append(x)
        if fused:
            s6, t6, w6 = P['s6'], P['t6'], P['w6']
            C6 = w6.shape[0]
            y6 = rows_gemm(cat, w6)
            ysel, arow = empty((B, C6), x), empty((B, C6), x, torch.int32)
            rs = _lib.lib().pdae_cloud_pool_splits(B, N)
            pv, pr = empty((B, rs, C6), x), empty((B, rs, C6), x, torch.int32)
            part, sums = empty((B * rs, 2 * C6), x, torch.float64), empty((2 * C6,), x, torch.float64)
            _lib.call('pdae_cloud_pool_stats', x, B, N, C6, _lib.ptr(y6), _lib.ptr(enc.bn6.weight), _lib.ptr(ysel),
                      _lib.ptr(arow), _lib.ptr(pv), _lib.ptr(pr), _lib.ptr(part), _lib.ptr(sums))
            g = bn_lrelu_rows(ysel, s6, t6)
        else:
            s6, t6, _, _ = bn_eval_affine(enc.bn6)
            g = bn_lrelu_rows(linear_any(cat, _w(enc.conv6[0]).contiguous()), s6, t6).reshape(B, N, -1).amax(1)
        if capture is not None:
            capture.update(graphs_own=own, graphs=used, x1=xs[0], x2=xs[1], x3=xs[2])
            capture['global'] = g
        return cat, g

    @staticmethod
    def _edgeconv_layers(x, idx, li, first, second, s1, t1, cat):
        """One EdgeConv as the reference writes it (dgcnn_util.py:14-35,172-184): the (B N k, 2 C) edge tensor
        [x_j - x_i | x_i] by index gather, one or two conv + BatchNorm + LeakyReLU layers, the max over k."""
        B, N, k = idx.shape
        C = 3 if li == 0 else x.shape[1]
        feat = x[:, :C].reshape(B, N, C)
        flat = (idx.long() + (torch.arange(B, device=x.device) * N).view(B, 1, 1)).reshape(-1)
        nbr = feat.reshape(B * N, C)[flat].reshape(B, N, k, C)
        ctr = feat.unsqueeze(2).expand(B, N, k, C)
        e = torch.cat([nbr - ctr, ctr], dim=3).reshape(B * N * k, 2 * C)
        h = bn_lrelu_rows(linear_any(e, _w(first[0])), s1, t1)
        if second is not None:
            s2, t2, _, _ = bn_eval_affine(second[1])
            h = bn_lrelu_rows(linear_any(h, _w(second[0])), s2, t2)
        out = h.reshape(B * N, k, -1).amax(1)
        cat[:, 64 * li:64 * li + out.shape[1]] = out
        return out

    # ---- the head ---------------------------------------------------------------------------------------------------
    def label_feature(self, cls):
        """conv7 on a one-hot = column cls of its weight, bn7's affine, LeakyReLU -> (B, 64)."""
        scale, shift, _, _ = bn_eval_affine(self.bn7)
        v = self.conv7[0].weight[:, :, 0].t()[cls.long()] * scale + shift
        return torch.where(v > 0, v, v * LRELU_SLOPE)

    def head_layers(self, cat, g, cls, B, N):
        """The head as the reference writes it (dgcnn_partseg.py:124-140) -> logits (B*N, cls_dim)."""
        glob = torch.cat([g, self.label_feature(cls)], 1)                                           # (B, 1088)
        x = torch.cat([glob.unsqueeze(1).expand(B, N, glob.shape[1]).reshape(B * N, -1), cat], 1)    # (B*N, 1280)
        for conv in (self.conv8, self.conv9, self.conv10):
            s, t, _, _ = bn_eval_affine(conv[1])
            x = bn_lrelu_rows(linear_any(x, _w(conv[0])), s, t)
        return linear_any(x, _w(self.conv11))

    def head_hip(self, cat, g, cls, B, N, seg, lo, hi, counts):
        P = self.prepared()
        v = self.conv7[0].weight[:, :, 0].t()[cls.long()] * P['s7'] + P['t7']
        glob = torch.cat([g, torch.where(v > 0, v, v * LRELU_SLOPE)], 1)                             # (B, 1088)
        gbias = linear_any(glob, P['w8_glob'], P['t8'])                                              # (a) once per cloud
        y = cloud_bias_lrelu(rows_gemm(cat, P['w8_point']), gbias, B, N)
        y = bn_lrelu_rows(rows_gemm(y, P['w9']), P['s9'], P['t9'])
        y = rows_gemm(y, P['w10'])
        return logits_tail(y, P['s10'], P['t10'], P['w11'], None, B, N, seg, lo, hi, counts)        # (b)

    @torch.no_grad()
    def forward(self, pts, cls_label, seg=None, counts=None, capture=None, graphs=None):
        """pts (B, N, 3+), cls_label (B,) the category id (not a one-hot) -> logits (B, N, cls_dim) fp32.  With seg (B, N)
        and counts (partseg_ops.Counts): -> (logits, pred (B, N) over each shape's own part range), the metric's counts
        added on the device.  graphs: a (3, B, N, k) int32 tensor used in place of the model's own three graphs."""
        name = type(self).__name__
        if self.training:
            raise NotImplementedError('%s: evaluation mode only -- part-segmentation training is not built' % name)
        if not pts.is_cuda:
            raise RuntimeError('%s: points must be on the GPU (there is no CPU path)' % name)
        if cls_label.dim() != 1 or cls_label.shape[0] != pts.shape[0]:
            raise ValueError('%s: cls_label is the (B,) category id, not a one-hot' % name)
        B, N = pts.shape[:2]
        if not 1 <= N <= 65535:
            raise ValueError('%s: %d points per cloud; the graph kernels take 1 to 65535' % (name, N))
        k = min(K_GRAPH, N)
        if graphs is not None:
            if tuple(graphs.shape) != (3, B, N, k) or graphs.dtype != torch.int32 or graphs.device != pts.device:
                raise ValueError('%s: graphs is a (3, B, N, k = %d) int32 tensor on the points\' device' % (name, k))
        pts = pts[:, :, :3].contiguous()
        cls = cls_label.to(pts.device)
        begin_step(pts.device)
        fused = self.partseg_mode(k) == 'hip'
        if capture is not None:
            capture['partseg'] = 'hip' if fused else 'layers'
        cat_ = lo = hi = None
        if seg is not None:
            if counts is None:
                raise ValueError('%s: seg goes with counts' % name)
            cat_, lo, hi = partseg_ops.shape_ranges(seg)
        feats, g = self.encode(pts, fused, graphs, capture)
        pred = None
        if fused:
            logits, pred = self.head_hip(feats, g, cls, B, N, seg, lo, hi, counts)
            logits = logits.reshape(B, N, -1)
            pred = pred.reshape(B, N) if seg is not None else None
        else:
            logits = self.head_layers(feats, g, cls, B, N).reshape(B, N, -1)
            if seg is not None:
                pred = partseg_ops.restricted_argmax(logits, lo, hi)
                partseg_ops._count_glue(pred, seg, cat_, lo, hi, counts)
        if seg is not None:
            counts.shape_cat[counts.filled:counts.filled + B] = cat_
            counts.filled += B
            counts.points += B * N
        return logits if seg is None else (logits, pred)
