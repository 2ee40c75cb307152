"""A PointNet++ set-abstraction level in evaluation mode, forward only (csrc/sa_eval.hip; include/pdae.h).

Reference: extensions/pointnet2/pointnet2_modules.py (PointnetSAModule.forward) with every BatchNorm2d on its running
estimates, as models/PointCAE_pointnetv2.py:936-1017 (PointNetv2_feat) runs it under --svm_classification.

    level(xyz, new_xyz, idx, features, layers)   a grouped level -> (B*np, C3), or None when the kernel refuses the layout
    group_all(xyz, features, layers)             the last level (one group per cloud) -> (B, C3)

In evaluation mode the first layer is linear per source point up to the centred coordinates, so its feature columns
run once per source point -- P = features W0f^T on the row GEMM, (B*N, C1) rows instead of (B*np*ns, C1) -- and
pdae_sa_eval_forward does the rest of the level in one launch: no (B*np*ns, .) tensor exists.  The group-all level has
128 rows per cloud and needs no new kernel: the forward of the training chain (sa_mlp.mlp_max_forward) with the
running-estimate scale / shift as the next layer's prologue (each layer's batch statistics are computed and ignored).

PDAE_SA_EVAL=hip (default) | layers: `layers` keeps the layer-by-layer form of PointnetSAModule.forward (the fallback for
layouts the kernel refuses, and the timing baseline of tools/bench_sa_eval.py).
"""
import os

from . import _lib, sa_mlp
from .rows import bn_eval_affine, empty, insert_zero_col, rows_gemm

MODES = ('hip', 'layers')


def mode():
    m = os.environ.get('PDAE_SA_EVAL', 'hip')
    if m not in MODES:
        raise ValueError('PDAE_SA_EVAL=%s: expected one of %s' % (m, ', '.join(MODES)))
    return m


def layer_affines(layers):
    """The level's _ConvBN modules -> [(weight (C_l, C_{l-1}), scale, shift)] of their eval-mode form."""
    out = []
    for layer in layers:
        scale, shift, _, _ = bn_eval_affine(layer.bn.bn)
        out.append((layer.conv.weight.reshape(layer.conv.weight.shape[0], -1), scale, shift))
    return out


def supported(ns, widths):
    """widths = (C0, C1, C2, C3): whether pdae_sa_eval_forward takes the level."""
    return len(widths) == 4 and bool(_lib.lib().pdae_sa_eval_supported(int(ns), *[int(c) for c in widths]))


def forward(xyz, new_xyz, idx, features, affines):
    """pdae_sa_eval_forward on xyz (B,N,3), new_xyz (B,np,3), idx (B,np,ns) i32, features (B*N, C0) rows or None and
    affines = [(W_l, scale_l, shift_l)] x 3 with W_0 (C1, 3 + C0) -> (B*np, C3); RuntimeError when the layout is refused."""
    B, N, _ = xyz.shape
    _, npoint, ns = idx.shape
    (w0, s0, t0), (w1, s1, t1), (w2, s2, t2) = affines
    C0 = 0 if features is None else features.shape[1]
    if w0.shape[1] != 3 + C0:
        raise ValueError('sa_eval: the first weight has %d columns for 3 + %d inputs' % (w0.shape[1], C0))
    xyz, new_xyz, idx = xyz.contiguous(), new_xyz.contiguous(), idx.contiguous()
    w0x = w0[:, :3].contiguous()
    P = rows_gemm(features.contiguous(), w0[:, 3:].contiguous()) if C0 else None      # once per source point
    s0, t0, w1, s1, t1, w2, s2, t2 = (t.contiguous() for t in (s0, t0, w1, s1, t1, w2, s2, t2))
    out = empty((B * npoint, w2.shape[0]), xyz)
    _lib.call('pdae_sa_eval_forward', xyz, B, N, npoint, ns, C0, w0.shape[0], w1.shape[0], w2.shape[0], _lib.ptr(xyz),
              _lib.ptr(new_xyz), _lib.ptr(idx), _lib.ptr(P), _lib.ptr(w0x), _lib.ptr(s0), _lib.ptr(t0), _lib.ptr(w1),
              _lib.ptr(s1), _lib.ptr(t1), _lib.ptr(w2), _lib.ptr(s2), _lib.ptr(t2), _lib.ptr(out))
    return out


def level(xyz, new_xyz, idx, features, layers):
    """A grouped level of PointnetSAModule in evaluation mode -> (B*np, C3), or None when the kernel refuses its layout
    (the caller then takes the layer-by-layer form)."""
    affines = layer_affines(layers)
    C0 = 0 if features is None else features.shape[1]
    if len(affines) != 3 or C0 % 4 != 0 or not supported(idx.shape[2], [C0] + [a[0].shape[0] for a in affines]):
        return None
    return forward(xyz, new_xyz, idx, features, affines)


def group_all(xyz, features, layers):
    """The group-all level in evaluation mode: xyz (B,N,3), features (B*N, C) rows -> (B, C_last).  None when N > 256
    or C is not a multiple of 4 (the pooling kernel, the row GEMMs)."""
    B, N, _ = xyz.shape
    if N > 256 or features is None or features.shape[1] % 4 != 0:
        return None
    x = sa_mlp.all_rows(xyz.reshape(B * N, 3), features)                        # [xyz | 0 | features], K a multiple of 4
    affines = layer_affines(layers)
    ws = [(insert_zero_col(w, 3) if i == 0 else w).contiguous() for i, (w, _, _) in enumerate(affines)]
    # (each layer's batch statistics are computed and ignored; the winners reach no backward, so ARG_HOOK is not asked)
    return sa_mlp.mlp_max_forward(x, None, None, ws, lambda i, stats: affines[i][1:], N, hook=False)[0]
