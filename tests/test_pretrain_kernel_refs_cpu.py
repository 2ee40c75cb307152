"""The fp64 reference functions of tests/test_gpu_pretrain_kernels.py against the CPU oracle: what that file holds the
HIP kernels to is itself held to oracle.model / oracle.ops here, on a machine without a GPU."""
import random

import numpy as np
import torch
import torch.nn as nn

from conftest import make_clouds
from test_gpu_pretrain_kernels import (U, gamma, ref_chamfer_mean_grad, ref_drop_path_keep, ref_gelu, ref_mean_sum2,
                                       ref_patch_affine, ref_patch_affine_magnitudes, ref_pos_embed_module, ref_pos_fc1,
                                       ref_rows_to_steps, ref_steps_to_rows)


def _seed(s):
    random.seed(s), np.random.seed(s), torch.manual_seed(s)


def _inside(got, ref, bound):
    err = (got.double() - ref).abs()
    assert (err <= bound).all(), float((err / bound.clamp_min(1e-300)).max())


def test_patch_affine_reference_reproduces_apply_corruption_on_the_oracles_steps():
    from oracle import model as om
    from point_dae_amd import corrupt_util_tensor as cut
    B, G, K = 4, 3, 5
    counts = set()
    for seed in range(8):
        rng = np.random.default_rng(seed)
        center = torch.from_numpy(rng.uniform(-1, 1, (B, G, 3)).astype(np.float32))
        nbr = torch.from_numpy((0.2 * rng.standard_normal((B, G, K, 3))).astype(np.float32))
        _seed(seed)
        steps = om.draw_corruption(['affine_r3'], B)
        steps = [(k, p.float()) for k, p in steps]                # (shear is drawn in fp64; the kernel's table is fp32)
        counts.add(len(steps))
        gt, tn, tc = ref_patch_affine(nbr, center, steps)
        absolute = nbr.double() + center.double().unsqueeze(2)
        P, T = om.apply_corruption(absolute, center.double(), [(k, p.double()) for k, p in steps])
        assert torch.equal(tn, P - T.unsqueeze(2)) and torch.equal(tc, T) and torch.equal(gt, absolute - center.double().unsqueeze(2))
        # the oracle's own fp32 run of the same steps stays inside the bound the kernel is held to: whatever the order
        # of a 3-term product sum, a leaf passes at most `cost` roundings in the steps; the inputs here are fl(nbr + c)
        # (one rounding) and c, and P32 - T32 adds one
        a32 = nbr + center.unsqueeze(2)
        P32, T32 = om.apply_corruption(a32, center, steps)
        AP, AT, cost = ref_patch_affine_magnitudes(nbr.double().abs() + center.double().abs().unsqueeze(2),
                                                   center.double().abs(), steps)
        _inside(P32 - T32.unsqueeze(2), tn, gamma(cost + 2) * (AP + AT.unsqueeze(2)))
        _inside(T32, tc, gamma(cost) * AT)
        # the two step formats: the oracle's list <-> the product's (nsteps, B, 10) rows of the same host draws.  The
        # kinds agree exactly; a rotation is built from the same fp32 angles by two expressions of a 3-matrix product
        # (entries <= 1: a few roundings, 16 u taken), everything else is copied
        rows = ref_steps_to_rows(steps, B)
        assert rows.shape == (len(steps), B, 10)
        back = ref_rows_to_steps(rows)
        assert all(k1 == k2 and torch.equal(p1, p2) for (k1, p1), (k2, p2) in zip(steps, back))
        _seed(seed)
        mine = cut.draw_corruption(['affine_r3'], B)
        assert mine.shape == rows.shape and torch.equal(mine[:, :, 0], rows[:, :, 0])
        assert (mine - rows).abs().max().item() <= 16 * U
    assert counts == {1, 2, 3}


def test_drop_path_reference_equals_the_wrappers_cpu_branch():
    from point_dae_amd import nn_ops
    probs = [0.0, 0.05, 0.1, 0.0, 0.25]
    keep = nn_ops.drop_path_keep_buffer(probs)
    B = 37
    torch.manual_seed(5)
    got = nn_ops.draw_drop_path(B, probs, True, keep)
    torch.manual_seed(5)
    want = ref_drop_path_keep(torch.rand((2 * len(probs), B)), keep)
    for i, p in enumerate(probs):
        if p == 0.0:
            assert got[i] == (None, None)
        else:
            assert torch.equal(got[i][0], want[2 * i]) and torch.equal(got[i][1], want[2 * i + 1])
            assert ((want[2 * i] == 0) | (want[2 * i] == 1.0 / keep[2 * i])).all()
    # the edge the GPU test plants: with keep = 1 the largest draw rounds up to 2
    assert ref_drop_path_keep(torch.tensor([[1.0 - 2.0 ** -24]]), torch.tensor([1.0])).item() == 2.0


def test_pos_embed_reference_reproduces_the_oracles_pos_embed():
    from oracle.model import _pos_embed
    torch.manual_seed(9)
    seq = _pos_embed(384)
    x = torch.rand(50, 3) * 2 - 1
    w1, b1, w2, b2 = (p.detach() for p in seq.parameters())
    ref = ref_pos_embed_module(w1, b1, w2, b2)
    y64 = ref(x.double()).detach()
    z, h, gp, Az = ref_pos_fc1(x, w1, b1)
    # the closed forms against nn.GELU and its autograd derivative in fp64: a handful of fp64 roundings on |z| < 3
    zz = z.clone().requires_grad_(True)
    hh = nn.GELU()(zz)
    assert (hh.detach() - h).abs().max().item() <= 64 * 2.0 ** -53 * 3
    assert (torch.autograd.grad(hh.sum(), zz)[0] - gp).abs().max().item() <= 64 * 2.0 ** -53 * 3
    assert (ref[0](x.double()).detach() - z).abs().max().item() <= 8 * 2.0 ** -53 * Az.max().item()
    assert torch.equal(ref_gelu(z)[0], h)
    # the oracle's fp32 module: z32 within gamma(4) A_z (three products and the bias, in any order); GELU is 1.13-
    # Lipschitz and the host's erff / product add a few units of |z| (8 u |z| taken); the second layer's dot product of
    # H = 128 terms and the bias: gamma(H + 1) on A_y, plus the first layer's error through |W2|
    H = w1.shape[0]
    dh = 1.13 * gamma(4) * Az + 8 * U * z.abs()
    bound = gamma(H + 1) * (h.abs() @ w2.double().abs().T + b2.double().abs()) + dh @ w2.double().abs().T
    _inside(seq(x).detach(), y64, bound)


def test_chamfer_mean_gradient_reference_equals_the_oracles_backward(oracle_ops):
    for B, n, m, g in ((3, 40, 17, 1.0), (2, 9, 64, -0.37), (4, 25, 1, 1.0)):
        a, b = make_clouds(83, B, n), make_clouds(84, B, m)
        _, _, i1, i2 = oracle_ops.chamfer_forward(a, b)
        g = float(np.float32(g))
        (r1, S1, c1), (r2, S2, c2) = ref_chamfer_mean_grad(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(i1),
                                                           torch.from_numpy(i2), g)
        assert c1.sum().item() == B * m and c2.sum().item() == B * n
        # the oracle in fp64 with the constant gradients of the two means: the same terms, c + 3 fp64 roundings each
        w1, w2 = oracle_ops.chamfer_backward(a.astype(np.float64), b.astype(np.float64), i1, i2,
                                             np.full((B, n), g / (B * n)), np.full((B, m), g / (B * m)))
        _inside(torch.from_numpy(w1), r1, (c1 + 3) * 2.0 ** -53 * S1 * 2)
        _inside(torch.from_numpy(w2), r2, (c2 + 3) * 2.0 ** -53 * S2 * 2)
        # and in fp32, under the bound the kernels are held to (the constants rounded once, as the kernel's division is)
        v1, v2 = oracle_ops.chamfer_backward(a, b, i1, i2, np.full((B, n), np.float32(g) / np.float32(B * n), np.float32),
                                             np.full((B, m), np.float32(g) / np.float32(B * m), np.float32))
        _inside(torch.from_numpy(v1), r1, gamma(1) * (c1 + 3) * S1)
        _inside(torch.from_numpy(v2), r2, gamma(1) * (c2 + 3) * S2)


def test_mean_sum2_reference_equals_the_oracles_l2_loss(oracle_ops):
    a, b = make_clouds(85, 3, 40), make_clouds(86, 3, 17)
    d1, d2, _, _ = oracle_ops.chamfer_forward(a, b)
    want, bound = ref_mean_sum2(torch.from_numpy(d1).reshape(-1), torch.from_numpy(d2).reshape(-1))
    # the oracle means in fp32 (numpy's pairwise sum: fewer roundings than the kernels' chain)
    assert abs(float(oracle_ops.chamfer_distance_l2(a, b)) - want) <= bound
    assert abs(bound - gamma(19) * want) <= 1e-12 * bound                      # 120 and 51 elements: one chain step each
    # fp64 distances of the same clouds: an fp32 distance (dx dx + dy dy) + dz dz passes 4 roundings per term
    l64 = oracle_ops.chamfer_distance_l2(a.astype(np.float64), b.astype(np.float64))
    assert abs(l64 - want) <= gamma(4) * want
