"""The batch preparation of few-shot fine-tuning on the gfx950 kernel of csrc/fewshot.hip.

The reference (datasets/ModelNetDatasetFewShot.py:59-71, tools/runner_finetune.py:158-176) shuffles the 8192 points of
every training cloud on every access, so the loop's FPS 8192 -> 1200 starts from a different point every time and nothing
of it can be kept; around it come the batch's item select, the shuffle's gather, index_select and the two transposing
copies around gather_points.  Here the episode (50 to 200 clouds) lives on the device and a batch is

    item, perm, labels = <the loader's draws>                      # datasets.ModelNetFewShot
    choice = runner_finetune.subset_indices(npoints, point_all)    # the reference's host draw
    fill_batch(set, item, perm, choice, point_all, out)            # PDAE_FEWSHOT=hip: ONE launch into the step's input
    resample(materialise(set, item, perm), npoints, choice)        # PDAE_FEWSHOT=torch: the reference's loop

Both consume the same draws, so a seed gives bit-identical batches under either backend.  The test subset is never
shuffled: fps_points(points, npoints) is its FPS to npoints points, taken once per fold (runner_finetune).
"""
import os

import numpy as np
import torch

from . import _lib
from .datasets import _dev             # host draws -> device behind pinned staging: the host never waits for the stream


def backend():
    """'hip' or 'torch', from PDAE_FEWSHOT."""
    name = os.environ.get('PDAE_FEWSHOT', 'hip')
    if name not in ('hip', 'torch'):
        raise ValueError('PDAE_FEWSHOT=%r: hip or torch' % name)
    return name


def slot_of(choice, point_all):
    """The inverse of the host draw: slot (point_all,) int32 with slot[choice[n]] = n and -1 everywhere else -- the
    output row of every FPS column, which is what the kernel's one thread per column needs."""
    choice = np.asarray(choice).reshape(-1)
    if choice.size and (choice.min() < 0 or choice.max() >= point_all):
        raise ValueError('slot_of: choice outside 0..%d' % (point_all - 1))
    slot = np.full(point_all, -1, np.int32)
    slot[choice] = np.arange(choice.size, dtype=np.int32)
    return slot


def batch_host(set_, item, perm, m, fps=None):
    """The host twin of pdae_fewshot_batch's definition on numpy: FPS of the materialised shuffle
    sh[b][k] = set[item[b]][perm[b][k]][0:3] to m points through `fps` ((B,P,3), m -> (B,m) int32: the CPU oracle's
    furthest_point_sample in the tests), mapped back through perm.  perm None: the identity.
    -> (idx (B,m) int32 = perm[b][f[b][j]], points (B,m,3) = sh[b][f[b][j]])."""
    set_, item = np.asarray(set_, np.float32), np.asarray(item).reshape(-1)
    sh = set_[item][:, :, :3]
    if perm is not None:
        perm = np.asarray(perm)
        sh = np.take_along_axis(sh, perm[:, :, None].astype(np.int64), 1)
    sh = np.ascontiguousarray(sh)
    f = np.asarray(fps(sh, m)).astype(np.int64)
    idx = f if perm is None else np.take_along_axis(perm.astype(np.int64), f, 1)
    return idx.astype(np.int32), np.take_along_axis(sh, f[:, :, None], 1)


def fewshot_batch(set_, item, m, npoints, perm=None, slot=None, out=None, want_idx=False):
    """pdae_fewshot_batch.  set_ (S,P,C>=3) fp32, item (B,) int32, perm (B,P) int32 or None, slot (m,) int32 or None
    (then npoints == m), all on the device; out (B,npoints,3) fp32: written where a slot names a row (a fresh buffer is
    zero-filled first).  -> (out, idx (B,m) int32 or None)."""
    _lib.require(set_, 'set', torch.float32, 3)
    _lib.require(item, 'item', torch.int32, 1)
    S, P, C = set_.shape
    B = item.shape[0]
    if perm is not None and tuple(_lib.require(perm, 'perm', torch.int32, 2).shape) != (B, P):
        raise ValueError('fewshot_batch: perm %r, expected (%d, %d)' % (tuple(perm.shape), B, P))
    if slot is not None and tuple(_lib.require(slot, 'slot', torch.int32, 1).shape) != (m,):
        raise ValueError('fewshot_batch: slot %r, expected (%d,)' % (tuple(slot.shape), m))
    if out is None:
        out = torch.zeros((B, npoints, 3), dtype=torch.float32, device=set_.device)
    elif tuple(_lib.require(out, 'out', torch.float32, 3).shape) != (B, npoints, 3):
        raise ValueError('fewshot_batch: out %r, expected (%d, %d, 3)' % (tuple(out.shape), B, npoints))
    idx = torch.empty((B, m), dtype=torch.int32, device=set_.device) if want_idx else None
    _lib.call('pdae_fewshot_batch', set_, S, P, C, B, m, npoints, _lib.ptr(set_), _lib.ptr(item), _lib.ptr(perm),
              _lib.ptr(slot), _lib.ptr(out), _lib.ptr(idx))
    return out, idx


def fill_batch(set_, item, perm, choice, point_all, out):
    """The hip path of a training batch: FPS of every row's shuffled cloud to point_all points, the columns `choice`
    (host, npoints of them) of that order written straight into `out` (B,npoints,3) -- the graphed step's input -- by
    one launch.  -> out."""
    slot = _dev(slot_of(choice, point_all), set_.device)
    fewshot_batch(set_, item, point_all, out.shape[1], perm=perm, slot=slot, out=out)
    return out


def materialise(set_, item, perm):
    """The torch path: the batch's clouds, shuffled, as a (B,P,3) tensor (the item select and the permutation gather as
    framework ops); runner_finetune.resample takes it from there."""
    x = set_.index_select(0, item.long())[:, :, :3]
    if perm is None:
        return x.contiguous()
    return torch.gather(x, 1, perm.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()


def fps_points(points, npoints):
    """FPS of the unshuffled clouds points (B,P,C>=3) to npoints points -> (B,npoints,3): pdae_fewshot_batch with
    perm = slot = NULL, bit for bit misc.fps(points, npoints)[1][:, :, :3]."""
    points = points.contiguous()
    item = torch.arange(points.shape[0], dtype=torch.int32, device=points.device)
    return fewshot_batch(points, item, npoints, npoints)[0]
