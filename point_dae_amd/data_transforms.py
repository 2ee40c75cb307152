"""The runner-side point-cloud transforms of the reference (datasets/data_transforms.py) as per-cloud affine maps, and
the fine-tuning batch preparation that applies one inside its gather (csrc/resample.hip).

The reference transforms a batch in a Python loop: per cloud a host draw, a host-to-device copy of the map, a matmul (or
mul + add) and a strided write-back.  Here a transform only DRAWS -- `draw(B)` makes the reference's np.random calls in the
reference's order and precision and returns the maps (A (B,3,3), t (B,3) or None; y = x A + t) after one transfer -- and
`resample_transformed` hands them to the one launch that also does the runner's subset + gather behind FPS
(tools/runner_finetune.py:415-420).
"""
import numpy as np
import torch

from . import _lib
from .pointnet2_utils import furthest_point_sample
from .runner_finetune import POINT_ALL, subset_indices


def _ship(A, t, device):
    """A (B,3,3) [, t (B,3)] fp32 host arrays -> tensors backed by ONE buffer: pinned on the host (when there is a GPU to
    pin for), or on `device` behind one non-blocking copy."""
    B = A.shape[0]
    flat = A.reshape(-1) if t is None else np.concatenate([A.reshape(-1), t.reshape(-1)])
    buf = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32))
    if torch.cuda.is_available():
        buf = buf.pin_memory()
    if device is not None:
        buf = buf.to(device, non_blocking=True)
    return buf[:B * 9].view(B, 3, 3), (None if t is None else buf[B * 9:].view(B, 3))


class PointcloudRotate(object):
    """data_transforms.py:6-18: one rotation about the y axis per cloud, angle np.random.uniform() * 2 pi, applied as
    matmul(pc[i], R)."""

    def draw(self, B, device=None):
        A = np.zeros((B, 3, 3), np.float32)                # [[c, 0, s], [0, 1, 0], [-s, 0, c]], fp64 values cast to fp32
        A[:, 1, 1] = 1.0
        for i in range(B):
            rotation_angle = np.random.uniform() * 2 * np.pi
            cosval, sinval = np.cos(rotation_angle), np.sin(rotation_angle)
            A[i, 0, 0] = A[i, 2, 2] = cosval
            A[i, 0, 2], A[i, 2, 0] = sinval, -sinval
        return _ship(A, None, device)


class PointcloudScaleAndTranslate(object):
    """data_transforms.py:20-34: per cloud pc * U(scale_low, scale_high)^3 + U(-translate_range, translate_range)^3."""

    def __init__(self, scale_low=2. / 3., scale_high=3. / 2., translate_range=0.2):
        self.scale_low, self.scale_high, self.translate_range = scale_low, scale_high, translate_range

    def draw_host(self, B):
        """The draws alone -> host arrays A (B,3,3), t (B,3) (vote_ops.draw_votes ships the maps of all votes at once)."""
        A = np.zeros((B, 3, 3), np.float32)
        t = np.empty((B, 3), np.float32)
        for i in range(B):
            xyz1 = np.random.uniform(low=self.scale_low, high=self.scale_high, size=[3])
            xyz2 = np.random.uniform(low=-self.translate_range, high=self.translate_range, size=[3])
            A[i, [0, 1, 2], [0, 1, 2]] = xyz1.astype(np.float32)
            t[i] = xyz2.astype(np.float32)
        return A, t

    def draw(self, B, device=None):
        return _ship(*self.draw_host(B), device)


def resample_affine(raw, fps_idx, choice, A=None, t=None, out=None):
    """pdae_resample_affine: out[b, n] = raw[b, fps_idx[b, choice[n]], :3] A[b] + t[b] -> (B, npoints, 3).
    raw (B,P,C>=3) fp32, fps_idx (B,point_all) int32, choice (npoints,) int32, A (B,3,3) / t (B,3) fp32 or None, all on
    the device; sizes the kernel does not take are refused by the library."""
    _lib.require(raw, 'raw', torch.float32, 3)
    _lib.require(fps_idx, 'fps_idx', torch.int32, 2)
    _lib.require(choice, 'choice', torch.int32, 1)
    B, P, C = raw.shape
    npoints = choice.shape[0]
    if fps_idx.shape[0] != B:
        raise ValueError('resample_affine: fps_idx %r for %d clouds' % (tuple(fps_idx.shape), B))
    if A is not None and tuple(_lib.require(A, 'A', torch.float32, 3).shape) != (B, 3, 3):
        raise ValueError('resample_affine: A %r, expected (%d, 3, 3)' % (tuple(A.shape), B))
    if t is not None and tuple(_lib.require(t, 't', torch.float32, 2).shape) != (B, 3):
        raise ValueError('resample_affine: t %r, expected (%d, 3)' % (tuple(t.shape), B))
    if out is None:
        out = torch.empty((B, npoints, 3), dtype=torch.float32, device=raw.device)
    elif tuple(_lib.require(out, 'out', torch.float32, 3).shape) != (B, npoints, 3):
        raise ValueError('resample_affine: out %r, expected (%d, %d, 3)' % (tuple(out.shape), B, npoints))
    _lib.call('pdae_resample_affine', raw, B, P, C, fps_idx.shape[1], npoints, _lib.ptr(raw), _lib.ptr(fps_idx),
              _lib.ptr(choice), _lib.ptr(A), _lib.ptr(t), _lib.ptr(out))
    return out


def resample_transformed(points, npoints, transform=None, choice=None, out=None):
    """runner_finetune.resample with the runner's transform (runner_finetune.py:415-420) folded into the gather: FPS of
    each cloud to point_all points; the host's subset `choice` of the FPS order (default: a fresh draw); the transform's
    draws -- AFTER the subset draw, as the reference consumes np.random; one launch -> (B, npoints, 3), written into `out`
    when given.  points (B,P,C>=3): the gather reads the rows of a wider cloud (normals) as they are; only FPS takes a
    coordinates-only copy."""
    if npoints not in POINT_ALL:
        raise NotImplementedError('npoints %d' % npoints)
    B, P, C = points.shape
    point_all = min(POINT_ALL[npoints], P)
    raw = points.contiguous()
    fps_idx = furthest_point_sample(raw if C == 3 else raw[:, :, :3].contiguous(), point_all)
    if choice is None:
        choice = subset_indices(npoints, point_all)
    if not isinstance(choice, torch.Tensor):
        choice = np.asarray(choice)
        if choice.shape != (npoints,) or choice.min() < 0 or choice.max() >= point_all:
            raise ValueError('resample_transformed: choice must be %d indices into the %d FPS points' % (npoints, point_all))
        choice = torch.from_numpy(choice.astype(np.int32))
        if points.is_cuda:
            choice = choice.pin_memory()
    choice = choice.to(device=points.device, dtype=torch.int32, non_blocking=True)
    A, t = transform.draw(B, device=points.device) if transform is not None else (None, None)
    return resample_affine(raw, fps_idx, choice, A, t, out)
