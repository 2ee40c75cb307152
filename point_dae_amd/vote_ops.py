"""The voted evaluation of a fine-tuned classifier on the gfx950 kernels of csrc/vote.hip.

The reference (tools/runner_finetune.py:835-899 test_vote, :568-632 validate_vote) takes, per test batch, FPS to
point_all points once and then `times` votes: a host draw of npoints of them, the gather, test_transforms
(PointcloudScaleAndTranslate: a Python loop over the clouds), a forward; the votes' logits are concatenated, averaged,
and the argmax is scored.  Here

    draws = draw_votes(B, point_all, npoints, times, transform, device)  # the reference's np.random calls, ONE transfer
    pred, mean = vote_batch(base_model, raw, fps_idx, label, draws, correct)

PDAE_VOTE=hip (default): pdae_vote_resample prepares the point sets of all votes in one launch, the V B clouds run as
one eval forward (cut only where a forward would outgrow the kernels' index range: clouds_per_forward), and
pdae_vote_reduce forms the mean logits, the argmax and the hit count on the device.  PDAE_VOTE=torch: the reference's
loop as framework ops -- per vote index_select, the two transposing copies around gather_points, multiply and add, a
forward of the B clouds; then torch.cat(...).mean(0) and torch.max.  Both consume the same draws, so a seed gives the same
votes under either backend and the same stream of np.random draws as the reference.
"""
import os

import numpy as np
import torch

from . import _lib
from .pointnet2_utils import gather_operation

MAX_CLASSES = _lib.CONST['PDAE_VOTE_MAX_CLASSES']
# the kernels index a forward's intermediates with 32-bit element counts (the library refuses 2^31 elements); the largest
# either classifier makes per cloud is DGCNN's (N, N) Gram matrix, or its (N, 1024) conv5 rows
MAX_FORWARD_ELEMENTS = 1 << 31


def backend():
    """'hip' or 'torch', from PDAE_VOTE."""
    name = os.environ.get('PDAE_VOTE', 'hip')
    if name not in ('hip', 'torch'):
        raise ValueError('PDAE_VOTE=%r: hip or torch' % name)
    return name


def draw_votes(B, point_all, npoints, times, transform, device=None):
    """The host draws of one test batch in the reference's order (runner_finetune.py:861-866): per vote
    np.random.choice(point_all, npoints, False), then test_transforms' draws -- per cloud three scale uniforms, then
    three shift uniforms (transform.draw_host; None: no transform, A = t = None).
    -> (choice (V, npoints) int32, A (V, B, 3, 3), t (V, B, 3)) backed by ONE buffer: pinned on the host (when there is a
    GPU to pin for), or on `device` behind one non-blocking copy."""
    choice = np.empty((times, npoints), np.int32)
    A = t = None
    if transform is not None:
        A, t = np.empty((times, B, 3, 3), np.float32), np.empty((times, B, 3), np.float32)
    for k in range(times):
        choice[k] = np.random.choice(point_all, npoints, False)
        if transform is not None:
            A[k], t[k] = transform.draw_host(B)
    parts = [choice.reshape(-1)] + ([A.reshape(-1).view(np.int32), t.reshape(-1).view(np.int32)] if A is not None else [])
    buf = torch.from_numpy(np.concatenate(parts))
    if torch.cuda.is_available():
        buf = buf.pin_memory()
    if device is not None:
        buf = buf.to(device, non_blocking=True)
    n0 = times * npoints
    choice_t = buf[:n0].view(times, npoints)
    if A is None:
        return choice_t, None, None
    n1 = n0 + times * B * 9
    return choice_t, buf[n0:n1].view(torch.float32).view(times, B, 3, 3), buf[n1:].view(torch.float32).view(times, B, 3)


def reduce_host(logits, labels=None):
    """The host twin of pdae_vote_reduce on numpy: logits (V, B, K) -> (mean (B, K) fp32: the fp32 sum over the votes in
    the order 0 .. V-1 divided by fp32 V; pred (B,) int64: its argmax, ties to the lowest class, -1 for a row with a NaN
    [; the number of rows with pred == label])."""
    logits = np.asarray(logits, dtype=np.float32)
    V = logits.shape[0]
    s = logits[0].copy()
    for k in range(1, V):
        s = s + logits[k]
    mean = s / np.float32(V)
    pred = np.where(np.isnan(mean).any(-1), -1, mean.argmax(-1)).astype(np.int64)
    if labels is None:
        return mean, pred
    return mean, pred, int(((pred >= 0) & (pred == np.asarray(labels).reshape(-1))).sum())


def vote_resample(raw, fps_idx, choice, A=None, t=None, out=None):
    """pdae_vote_resample: out[k, b, n] = raw[b, fps_idx[b, choice[k, n]], :3] A[k, b] + t[k, b] -> (V, B, npoints, 3),
    bit for bit data_transforms.resample_affine per vote.  raw (B,P,C>=3) fp32, fps_idx (B,point_all) int32, choice
    (V,npoints) int32, A (V,B,3,3) / t (V,B,3) fp32 or None, all on the device."""
    _lib.require(raw, 'raw', torch.float32, 3)
    _lib.require(fps_idx, 'fps_idx', torch.int32, 2)
    _lib.require(choice, 'choice', torch.int32, 2)
    B, P, C = raw.shape
    V, npoints = choice.shape
    if fps_idx.shape[0] != B:
        raise ValueError('vote_resample: fps_idx %r for %d clouds' % (tuple(fps_idx.shape), B))
    if A is not None and tuple(_lib.require(A, 'A', torch.float32, 4).shape) != (V, B, 3, 3):
        raise ValueError('vote_resample: A %r, expected (%d, %d, 3, 3)' % (tuple(A.shape), V, B))
    if t is not None and tuple(_lib.require(t, 't', torch.float32, 3).shape) != (V, B, 3):
        raise ValueError('vote_resample: t %r, expected (%d, %d, 3)' % (tuple(t.shape), V, B))
    if out is None:
        out = torch.empty((V, B, npoints, 3), dtype=torch.float32, device=raw.device)
    elif tuple(_lib.require(out, 'out', torch.float32, 4).shape) != (V, B, npoints, 3):
        raise ValueError('vote_resample: out %r, expected (%d, %d, %d, 3)' % (tuple(out.shape), V, B, npoints))
    _lib.call('pdae_vote_resample', raw, V, B, P, C, fps_idx.shape[1], npoints, _lib.ptr(raw), _lib.ptr(fps_idx),
              _lib.ptr(choice), _lib.ptr(A), _lib.ptr(t), _lib.ptr(out))
    return out


def vote_reduce(logits, labels, correct, want_mean=True):
    """pdae_vote_reduce: logits (V, B, K) fp32, labels (B,) int64, correct: ONE int32 on the device, added to.
    -> (pred (B,) int64, mean (B, K) or None)."""
    _lib.require(logits, 'logits', torch.float32, 3)
    _lib.require(labels, 'labels', torch.int64, 1)
    _lib.require(correct, 'correct', torch.int32)
    V, B, K = logits.shape
    if labels.shape[0] != B:
        raise ValueError('vote_reduce: %d labels for %d rows' % (labels.shape[0], B))
    if correct.numel() != 1:
        raise ValueError('vote_reduce: correct must be one int32 counter, got %r' % (tuple(correct.shape),))
    mean = torch.empty((B, K), dtype=torch.float32, device=logits.device) if want_mean else None
    pred = torch.empty((B,), dtype=torch.int64, device=logits.device)
    _lib.call('pdae_vote_reduce', logits, V, B, K, _lib.ptr(logits), _lib.ptr(labels), _lib.ptr(mean), _lib.ptr(pred),
              _lib.ptr(correct))
    return pred, mean


def clouds_per_forward(clouds, npoints):
    """How many of `clouds` clouds of npoints points one forward takes: all of them unless the largest intermediate,
    npoints x max(npoints, 1024) floats per cloud, would reach MAX_FORWARD_ELEMENTS; then as many as fit."""
    return max(1, min(clouds, (MAX_FORWARD_ELEMENTS - 1) // (npoints * max(npoints, 1024))))


def forward_clouds(base_model, points):
    """The eval forward of points (M, N, 3) -> logits (M, K) in as few forwards as clouds_per_forward allows (in eval
    mode no BatchNorm statistic, Dropout or DropPath couples the clouds of a batch)."""
    if base_model.training:
        raise RuntimeError('vote_ops: the model must be in eval() (a training-mode forward couples the clouds of a batch)')
    M, N = points.shape[0], points.shape[1]
    step = clouds_per_forward(M, N)
    if step >= M:
        return base_model(points)
    return torch.cat([base_model(points[i:i + step]) for i in range(0, M, step)], 0)


def vote_batch(base_model, raw, fps_idx, label, draws, correct):
    """The votes of one test batch.  raw (B,P,C>=3) fp32, fps_idx (B,point_all) int32, label (B,) int64, draws: draw_votes'
    (choice, A, t) on the device, correct: one int32 device counter, which receives the batch's hits.
    -> (pred (B,) int64, mean logits (B, K))."""
    choice, A, t = draws
    V, B = choice.shape[0], raw.shape[0]
    label = label.reshape(-1)
    if backend() == 'hip':
        points = vote_resample(raw, fps_idx, choice, A, t)
        logits = forward_clouds(base_model, points.view(V * B, points.shape[2], 3))
        return vote_reduce(logits.detach().contiguous().view(V, B, -1), label, correct)
    xyz_t = raw[:, :, :3].transpose(1, 2).contiguous()
    local_pred = []
    for k in range(V):
        idx = fps_idx.index_select(1, choice[k].long()).contiguous()
        points = gather_operation(xyz_t, idx).transpose(1, 2).contiguous()
        if A is not None:           # test_transforms: pc * xyz1 + xyz2 per cloud, here for the batch at once
            points = points * torch.diagonal(A[k], dim1=1, dim2=2).unsqueeze(1) + t[k].unsqueeze(1)
        local_pred.append(base_model(points).detach().unsqueeze(0))
    mean = torch.cat(local_pred, dim=0).mean(0)
    _, pred = torch.max(mean, -1)
    correct += (pred == label).sum().to(torch.int32)
    return pred, mean
