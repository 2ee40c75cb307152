"""The augmented training batch of the resident ModelNet set on the gfx950 kernel of csrc/fewshot.hip.

The reference's train loader (datasets/ModelNetDataset.py:127-158, tools/builder.py:17-31) redraws augment_data's maps
for a cloud and shuffles its 8192 points on every access; the loop (tools/runner_finetune.py:158-176) then runs FPS
8192 -> 1200 on that cloud, so FPS sees other coordinates in another order every time and nothing of it can be kept.  As
framework ops a batch is item select, permutation gather, pdae_pipeline_norm_affine, FPS, index_select and the two
transposing copies around gather_points.  Here the set lives on the device (datasets.ModelNet on the reference's files) and
a batch is

    item, perm, nmaps, maps, labels = <the loader's draws>                  # datasets.ModelNet.iter_draws
    choice = runner_finetune.subset_indices(npoints, point_all)              # the reference's host draw
    fill_batch(set, item, perm, nmaps, maps, choice, point_all, out)         # PDAE_MODELNET=hip: ONE launch into the step's input
    resample(<the loader's materialised batch>, npoints, choice)             # PDAE_MODELNET=torch: the loader's __iter__

Both consume the same draws, so a seed gives bit-identical batches under either backend.
"""
import os

import numpy as np
import torch

from . import _lib
from . import fewshot_ops
from .datasets import _dev


def backend():
    """'hip' or 'torch', from PDAE_MODELNET."""
    name = os.environ.get('PDAE_MODELNET', 'hip')
    if name not in ('hip', 'torch'):
        raise ValueError('PDAE_MODELNET=%r: hip or torch' % name)
    return name


def apply_maps_host(x, nmaps, maps):
    """The host twin of the kernel's load phase on numpy float32: x (B,P,3); row b goes through its maps 0 .. nmaps[b]-1
    (maps (B,3,12): M 3x3 row-major, then t) one after the other, each as x' = ((x*m00 + y*m10) + z*m20) + t0 -- every
    product and sum rounded to float32, in this order.  nmaps None: x as it is.  -> (B,P,3) float32."""
    out = np.array(x, np.float32)[:, :, :3].copy()
    if nmaps is None:
        return out
    nmaps, maps = np.asarray(nmaps).reshape(-1), np.asarray(maps, np.float32)
    for b in range(out.shape[0]):
        if not 0 <= int(nmaps[b]) <= 3:
            raise ValueError('apply_maps_host: nmaps[%d] = %d outside 0..3' % (b, int(nmaps[b])))
        for q in range(int(nmaps[b])):
            M = maps[b, q]
            x0, y0, z0 = out[b, :, 0].copy(), out[b, :, 1].copy(), out[b, :, 2].copy()
            for j in range(3):
                out[b, :, j] = ((x0 * M[j] + y0 * M[3 + j]) + z0 * M[6 + j]) + M[9 + j]
    return out


def batch_host(set_, item, perm, nmaps, maps, m, fps=None):
    """The host twin of pdae_resident_batch's definition: fewshot_ops.batch_host on the mapped clouds -- the maps are per
    point, so mapping the selected clouds first and shuffling them second is the kernel's order of events.
    -> (idx (B,m) int32, points (B,m,3))."""
    set_, item = np.asarray(set_, np.float32), np.asarray(item).reshape(-1)
    mapped = apply_maps_host(set_[item][:, :, :3], nmaps, maps)
    return fewshot_ops.batch_host(mapped, np.arange(len(item)), perm, m, fps)


def resident_batch(set_, item, m, npoints, perm=None, nmaps=None, maps=None, slot=None, out=None, want_idx=False):
    """pdae_resident_batch.  As fewshot_ops.fewshot_batch, with nmaps (B,) int32 and maps (B,3,12) fp32 on the device
    (nmaps None: no maps, pdae_fewshot_batch bit for bit).  -> (out, idx (B,m) int32 or None)."""
    _lib.require(set_, 'set', torch.float32, 3)
    _lib.require(item, 'item', torch.int32, 1)
    S, P, C = set_.shape
    B = item.shape[0]
    if perm is not None and tuple(_lib.require(perm, 'perm', torch.int32, 2).shape) != (B, P):
        raise ValueError('resident_batch: perm %r, expected (%d, %d)' % (tuple(perm.shape), B, P))
    if nmaps is not None and tuple(_lib.require(nmaps, 'nmaps', torch.int32, 1).shape) != (B,):
        raise ValueError('resident_batch: nmaps %r, expected (%d,)' % (tuple(nmaps.shape), B))
    if maps is not None and tuple(_lib.require(maps, 'maps', torch.float32, 3).shape) != (B, 3, 12):
        raise ValueError('resident_batch: maps %r, expected (%d, 3, 12)' % (tuple(maps.shape), B))
    if slot is not None and tuple(_lib.require(slot, 'slot', torch.int32, 1).shape) != (m,):
        raise ValueError('resident_batch: slot %r, expected (%d,)' % (tuple(slot.shape), m))
    if out is None:
        out = torch.zeros((B, npoints, 3), dtype=torch.float32, device=set_.device)
    elif tuple(_lib.require(out, 'out', torch.float32, 3).shape) != (B, npoints, 3):
        raise ValueError('resident_batch: out %r, expected (%d, %d, 3)' % (tuple(out.shape), B, npoints))
    idx = torch.empty((B, m), dtype=torch.int32, device=set_.device) if want_idx else None
    _lib.call('pdae_resident_batch', set_, S, P, C, B, m, npoints, _lib.ptr(set_), _lib.ptr(item), _lib.ptr(perm),
              _lib.ptr(nmaps), _lib.ptr(maps), _lib.ptr(slot), _lib.ptr(out), _lib.ptr(idx))
    return out, idx


def fill_batch(set_, item, perm, nmaps, maps, choice, point_all, out):
    """The hip path of a training batch: every row's cloud mapped and shuffled, its FPS to point_all points, the columns
    `choice` (host, npoints of them) of that order written straight into `out` (B,npoints,3) -- the graphed step's input
    -- by one launch.  -> out."""
    slot = _dev(fewshot_ops.slot_of(choice, point_all), set_.device)
    resident_batch(set_, item, point_all, out.shape[1], perm=perm, nmaps=nmaps, maps=maps, slot=slot, out=out)
    return out


def fps_points(points, npoints):
    """FPS of the unshuffled, unmapped clouds points (B,P,C>=3) to npoints points -> (B,npoints,3): the kernel with
    perm = nmaps = slot = NULL, bit for bit misc.fps(points, npoints)[1][:, :, :3]."""
    points = points.contiguous()
    item = torch.arange(points.shape[0], dtype=torch.int32, device=points.device)
    return resident_batch(points, item, npoints, npoints)[0]
