"""The part-segmentation head in evaluation mode, forward only (csrc/partseg.hip; include/pdae.h).

Reference: segmentation/models/pt.py:314-333 (get_model.forward behind the trunk) on PointNetFeaturePropagation
(segmentation/models/pointnet2_utils.py:262-312), and the metric of segmentation/main.py:246-295, with every BatchNorm
on its running estimates (rows.bn_eval_affine: y = x * scale + shift).

    head(model, pts, center, F, cls, seg=None, counts=None)  -> (log-probabilities (B, N, 50), pred (B, N) or None)
    Counts                                                    the metric's integer counts, resident on the device
    metrics(counts...)                                        the four numbers of the reference, float64 on the host

PDAE_PARTSEG=hip (default).  Three identities of the evaluation-mode head, all exact in real arithmetic:
  (a) the interpolation is linear and its weights sum to one, so the feature columns of propagation_0_cls's first conv
      run once per TOKEN -- T = F W0[:, 3:]^T + b0 on the row GEMM, G rows per cloud instead of N -- and
      pdae_partseg_propagate interpolates T, adds the three coordinate columns and applies affine + ReLU;
  (b) the 2368 global columns [max | mean | label] of convs1_cls are the same for all points of a cloud: one (B, 2368)
      product gives a per-cloud bias, added where that layer's activation is applied (pdae_partseg_cloud_bias_relu);
  (c) convs2's affine + ReLU, convs3, the log-softmax, the range-restricted argmax and the counts are one pass over a
      256-wide row (pdae_partseg_tail).
No (B*N, 1155) and no (B*N, 3392) tensor exists.  The affine of a layer whose product runs on the row GEMMs is folded
into its weight and bias (relu(s (x W^T + b) + t) = relu(x (s W)^T + (s b + t))): the GEMM's bias + ReLU epilogue does it.

PDAE_PARTSEG=layers keeps the head as the reference writes it -- pdae_three_nn + pdae_three_interpolate on the 1152-wide
features, the concatenations, five layers -- on kernels that predate csrc/partseg.hip plus framework glue: the fallback
for layouts pdae_partseg_supported refuses, and the timing baseline of tools/bench_partseg.py.
"""
import os

import numpy as np
import torch

from . import _lib
from .rows import bn_eval_affine, empty, linear_any, rows_gemm

MODES = ('hip', 'layers')
NUM_PART = 50

# category -> its part labels (segmentation/dataset.py:125-129 of the reference): the one place this table is written
SEG_CLASSES = {
    'Airplane': [0, 1, 2, 3], 'Bag': [4, 5], 'Cap': [6, 7], 'Car': [8, 9, 10, 11], 'Chair': [12, 13, 14, 15],
    'Earphone': [16, 17, 18], 'Guitar': [19, 20, 21], 'Knife': [22, 23], 'Lamp': [24, 25, 26, 27], 'Laptop': [28, 29],
    'Motorbike': [30, 31, 32, 33, 34, 35], 'Mug': [36, 37], 'Pistol': [38, 39, 40], 'Rocket': [41, 42, 43],
    'Skateboard': [44, 45, 46], 'Table': [47, 48, 49]}
CATEGORIES = sorted(SEG_CLASSES)                 # the order of synsetoffset2category.txt, and of the printed lines


def label_tables():
    """-> (cat_of_label (50,), lo (16,), hi (16,)) int32 numpy: a part label's category index in CATEGORIES and every
    category's first and last part label."""
    cat_of = np.zeros(NUM_PART, np.int32)
    lo, hi = np.zeros(len(CATEGORIES), np.int32), np.zeros(len(CATEGORIES), np.int32)
    for i, cat in enumerate(CATEGORIES):
        parts = SEG_CLASSES[cat]
        cat_of[parts] = i
        lo[i], hi[i] = parts[0], parts[-1]
    return cat_of, lo, hi


def mode():
    m = os.environ.get('PDAE_PARTSEG', 'hip')
    if m not in MODES:
        raise ValueError('PDAE_PARTSEG=%s: expected one of %s' % (m, ', '.join(MODES)))
    return m


def supported(G, C, K=256, P=NUM_PART):
    """Whether pdae_partseg_propagate (G centres per cloud, width C) and pdae_partseg_tail (K inputs, P labels) take
    the layout."""
    return bool(_lib.lib().pdae_partseg_supported(int(G), int(C), int(K), int(P)))


def token_pool(F, B, G):
    """F (B*G, C) rows -> (B, 2C) = [max over a cloud's tokens | their mean]."""
    C = F.shape[1]
    out = empty((B, 2 * C), F)
    _lib.call('pdae_partseg_token_pool', F, B, G, C, _lib.ptr(F), _lib.ptr(out))
    return out


def propagate(pts, center, T, w0x, scale0, shift0, want_idx=False):
    """pts (B, N, 3), center (B, G, 3), T (B*G, C) -> a0 (B*N, C) [, idx3 (B, N, 3) int32]; RuntimeError when the layout
    is refused."""
    B, N, _ = pts.shape
    G, C = center.shape[1], T.shape[1]
    pts, center, T, w0x, scale0, shift0 = (t.contiguous() for t in (pts, center, T, w0x, scale0, shift0))
    a0 = empty((B * N, C), pts)
    idx3 = empty((B, N, 3), pts, torch.int32) if want_idx else None
    _lib.call('pdae_partseg_propagate', pts, B, N, G, C, _lib.ptr(pts), _lib.ptr(center), _lib.ptr(T), _lib.ptr(w0x),
              _lib.ptr(scale0), _lib.ptr(shift0), _lib.ptr(a0), _lib.ptr(idx3))
    return (a0, idx3) if want_idx else a0


def cloud_bias_relu(y, gbias, B, N):
    """y (B*N, C) <- relu(y + gbias[b]) in place."""
    gbias = gbias.contiguous()
    _lib.call('pdae_partseg_cloud_bias_relu', y, B, N, y.shape[1], _lib.ptr(y), _lib.ptr(gbias))
    return y


class Counts:
    """The metric's integer counts of `shapes` shapes, on the device until read(): shape_iu (S, 2, 50) intersections and
    unions per shape and part label, shape_correct (S,), shape_cat (S,) the category index of each shape (from its first
    point's label), part_seen / part_correct (50,), points = the points counted (host)."""

    def __init__(self, shapes, device):
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)     # noqa: E731
        self.shape_iu, self.shape_correct, self.shape_cat = z(shapes, 2, NUM_PART), z(shapes), z(shapes)
        self.part_seen, self.part_correct = z(NUM_PART), z(NUM_PART)
        self.filled, self.points = 0, 0

    def read(self):
        """ONE read-back: every count as numpy, the used shapes only."""
        n = self.filled
        flat = torch.cat([self.shape_iu[:n].reshape(-1), self.shape_correct[:n], self.shape_cat[:n], self.part_seen,
                          self.part_correct]).cpu().numpy()
        a = n * 2 * NUM_PART
        return dict(shape_iu=flat[:a].reshape(n, 2, NUM_PART), shape_correct=flat[a:a + n], shape_cat=flat[a + n:a + 2 * n],
                    part_seen=flat[a + 2 * n:a + 2 * n + NUM_PART], part_correct=flat[a + 2 * n + NUM_PART:],
                    points=self.points)


_tables = {}


def shape_ranges(seg):
    """seg (B, N) int -> (cat (B,), lo (B,), hi (B,)) int32 on the device: the shape's category and part range from its
    FIRST point's label (segmentation/main.py:257,272)."""
    key = seg.device
    if key not in _tables:
        _tables[key] = tuple(torch.from_numpy(t).to(seg.device) for t in label_tables())
    cat_of, lo, hi = _tables[key]
    cat = cat_of[seg[:, 0].long().clamp(0, NUM_PART - 1)]
    return cat, lo[cat.long()].contiguous(), hi[cat.long()].contiguous()


def tail(y, scale, shift, w3, b3, S, N, seg=None, lo=None, hi=None, counts=None):
    """pdae_partseg_tail on y (S*N, 256) -> (logp (S*N, 50), pred (S*N,) int32); with seg (S, N) int32 and counts the
    counts of these S shapes are added at counts.filled."""
    y, scale, shift, w3, b3 = (t.contiguous() for t in (y, scale, shift, w3, b3))
    logp = empty((S * N, w3.shape[0]), y)
    pred = empty((S * N,), y, torch.int32)
    iu = sc = None
    if seg is not None:
        if counts is None or lo is None or hi is None:
            raise ValueError('partseg tail: seg goes with counts and the part ranges')
        seg = seg.to(torch.int32).contiguous()
        f = counts.filled
        if f + S > counts.shape_correct.shape[0]:
            raise ValueError('partseg tail: the counts hold %d shapes' % counts.shape_correct.shape[0])
        iu, sc = counts.shape_iu[f:f + S], counts.shape_correct[f:f + S]
    _lib.call('pdae_partseg_tail', y, S, N, y.shape[1], w3.shape[0], _lib.ptr(y), _lib.ptr(scale), _lib.ptr(shift),
              _lib.ptr(w3), _lib.ptr(b3), _lib.ptr(seg), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(logp), _lib.ptr(pred),
              _lib.ptr(iu), _lib.ptr(sc), _lib.ptr(counts.part_seen) if seg is not None else None,
              _lib.ptr(counts.part_correct) if seg is not None else None)
    return logp, pred


def _affine(conv, bn):
    """A Conv1d(k=1) + eval-mode BatchNorm1d -> (W (out, in), bias, scale, shift)."""
    scale, shift, _, _ = bn_eval_affine(bn)
    return conv.weight.reshape(conv.weight.shape[0], -1), conv.bias, scale, shift


def _folded(conv, bn):
    """-> (s W, s b + t): relu(bn(conv(x))) = relu(x (s W)^T + (s b + t))."""
    w, b, s, t = _affine(conv, bn)
    return (w * s[:, None]).contiguous(), (b * s + t).contiguous()


def label_feature(model, cls):
    """label_conv_cls on a one-hot = column cls of its weight, the BatchNorm affine, LeakyReLU(0.2) -> (B, 64)."""
    conv, bn, act = model.label_conv_cls
    scale, shift, _, _ = bn_eval_affine(bn)
    v = conv.weight[:, :, 0].t()[cls.long()] * scale + shift
    return torch.where(v > 0, v, v * act.negative_slope)


def _count_glue(pred, seg, cat, lo, hi, counts):
    """The counts of pdae_partseg_tail as framework ops (PDAE_PARTSEG=layers)."""
    S, N = seg.shape
    f = counts.filled
    labels = torch.arange(NUM_PART, device=seg.device).view(1, 1, -1)
    p, g = pred.view(S, N, 1) == labels, seg.view(S, N, 1) == labels
    inside = (labels.view(1, -1) >= lo.view(-1, 1)) & (labels.view(1, -1) <= hi.view(-1, 1))
    counts.shape_iu[f:f + S, 0] += ((p & g).sum(1) * inside).to(torch.int32)
    counts.shape_iu[f:f + S, 1] += ((p | g).sum(1) * inside).to(torch.int32)
    counts.shape_correct[f:f + S] += (pred.view(S, N) == seg).sum(1).to(torch.int32)
    counts.part_seen += g.sum((0, 1)).to(torch.int32)
    counts.part_correct += (p & g).sum((0, 1)).to(torch.int32)


def restricted_argmax(logp, lo, hi):
    """logp (S, N, 50), lo / hi (S,) -> the argmax over [lo, hi] per shape, first index on ties, (S, N) int32."""
    labels = torch.arange(logp.shape[-1], device=logp.device).view(1, 1, -1)
    inside = (labels >= lo.view(-1, 1, 1)) & (labels <= hi.view(-1, 1, 1))
    return torch.where(inside, logp, torch.full_like(logp, float('-inf'))).argmax(-1).to(torch.int32)


def head_layers(model, pts, center, F, cls, capture=None):
    """The head as the reference writes it, on kernels that predate csrc/partseg.hip -> log-probabilities (B*N, 50)."""
    from .pointnet2_utils import three_interpolate, three_nn
    B, N, _ = pts.shape
    G, C = center.shape[1], F.shape[1]
    Fb = F.reshape(B, G, C)
    glob = torch.cat([Fb.max(1)[0], Fb.mean(1), label_feature(model, cls)], 1)                      # (B, 2368)
    dist, idx = three_nn(pts, center)
    recip = 1.0 / (dist * dist + 1e-8)                    # (three_nn returns the square root of the squared distance)
    weight = recip / recip.sum(2, keepdim=True)
    interp = three_interpolate(Fb.transpose(1, 2).contiguous(), idx, weight.contiguous())           # (B, C, N)
    if capture is not None:
        capture['three_idx'] = idx
    x = torch.cat([pts.reshape(B * N, 3), interp.transpose(1, 2).reshape(B * N, C)], 1)              # (B*N, 1155)
    prop = model.propagation_0_cls
    for conv, bn in zip(prop.mlp_convs, prop.mlp_bns):
        w, b = _folded(conv, bn)
        x = linear_any(x, w, b, relu=True)
    x = torch.cat([x, glob.unsqueeze(1).expand(B, N, glob.shape[1]).reshape(B * N, -1)], 1)          # (B*N, 3392)
    x = linear_any(x, *_folded(model.convs1_cls, model.bns1_cls), relu=True)
    x = linear_any(x, *_folded(model.convs2_cls, model.bns2_cls), relu=True)
    x = linear_any(x, model.convs3_cls.weight.reshape(model.cls_dim, -1), model.convs3_cls.bias)
    return torch.log_softmax(x, dim=1)


def head(model, pts, center, F, cls, seg=None, counts=None, capture=None):
    """The evaluation-mode head on pts (B, N, 3), center (B, G, 3), F (B*G, 1152) = [tap3 | tap7 | tap11], cls (B,) ->
    (log-probabilities (B, N, 50) fp32, pred (B, N) int32 over the shape's part range or None without seg).  With seg
    (B, N) and counts (Counts) the batch's counts are added and counts.filled / counts.points advance."""
    B, N, _ = pts.shape
    G, C = center.shape[1], F.shape[1]
    prop = model.propagation_0_cls
    widths_ok = len(prop.mlp_convs) == 2 and model.convs3_cls.weight.shape[0] == NUM_PART
    cat = lo = hi = None
    if seg is not None:
        cat, lo, hi = shape_ranges(seg)
    fused = mode() == 'hip' and widths_ok and supported(G, prop.mlp_convs[0].weight.shape[0],
                                                        model.convs3_cls.weight.shape[1], model.cls_dim)
    if capture is not None:
        capture['partseg'] = 'hip' if fused else 'layers'
    if not fused:
        logp = head_layers(model, pts, center, F, cls, capture).reshape(B, N, -1)
        pred = None
        if seg is not None:
            pred = restricted_argmax(logp, lo, hi)
            _count_glue(pred, seg, cat, lo, hi, counts)
    else:
        w0, b0, s0, t0 = _affine(prop.mlp_convs[0], prop.mlp_bns[0])
        T = rows_gemm(F.contiguous(), w0[:, 3:].contiguous(), bias=b0.contiguous())                 # (a) once per token
        glob = torch.cat([token_pool(F.contiguous(), B, G), label_feature(model, cls)], 1)           # (B, 2368)
        wc, bc = _folded(model.convs1_cls, model.bns1_cls)
        n_local = prop.mlp_convs[1].weight.shape[0]
        gbias = linear_any(glob, wc[:, n_local:].contiguous(), bc)                                   # (b) once per cloud
        a0 = propagate(pts, center, T, w0[:, :3], s0, t0, want_idx=capture is not None)
        if capture is not None:
            a0, capture['three_idx'] = a0
        w1, b1 = _folded(prop.mlp_convs[1], prop.mlp_bns[1])
        a1 = rows_gemm(a0, w1, bias=b1, epi=1)
        y = cloud_bias_relu(rows_gemm(a1, wc[:, :n_local].contiguous()), gbias, B, N)
        w2, b2, s2, t2 = _affine(model.convs2_cls, model.bns2_cls)
        y = rows_gemm(y, w2.contiguous(), bias=b2.contiguous())
        logp, pred = tail(y, s2, t2, model.convs3_cls.weight.reshape(model.cls_dim, -1), model.convs3_cls.bias, B, N,
                          seg, lo, hi, counts)                                                       # (c)
        logp = logp.reshape(B, N, -1)
        pred = pred.reshape(B, N) if seg is not None else None
    if seg is not None:
        counts.shape_cat[counts.filled:counts.filled + B] = cat
        counts.filled += B
        counts.points += B * N
    return logp, pred


def metrics(c):
    """The four numbers of segmentation/main.py:261-295 from Counts.read(), in float64 as numpy forms them ->
    dict(accuracy, class_avg_accuracy, class_avg_iou, inctance_avg_iou, category_iou {name: mIoU})."""
    _, lo, hi = label_tables()
    shape_ious = {cat: [] for cat in CATEGORIES}
    every = []
    for s in range(len(c['shape_correct'])):
        k = int(c['shape_cat'][s])
        inter = c['shape_iu'][s, 0, lo[k]:hi[k] + 1].astype(np.float64)
        union = c['shape_iu'][s, 1, lo[k]:hi[k] + 1].astype(np.float64)
        # a part absent from both the prediction and the truth counts 1.0
        iou = np.where(union == 0, 1.0, inter / np.where(union == 0, 1.0, union))
        shape_ious[CATEGORIES[k]].append(np.mean(iou))
        every.append(np.mean(iou))
    with np.errstate(invalid='ignore', divide='ignore'):
        cat_iou = {cat: (np.mean(v) if v else np.float64('nan')) for cat, v in shape_ious.items()}
        class_acc = np.mean(c['part_correct'].astype(np.float64) / c['part_seen'].astype(np.float64))
    return dict(accuracy=float(c['shape_correct'].sum()) / float(c['points']), class_avg_accuracy=float(class_acc),
                class_avg_iou=float(np.mean(list(cat_iou.values()))), inctance_avg_iou=float(np.mean(every)),
                category_iou={k: float(v) for k, v in cat_iou.items()})
