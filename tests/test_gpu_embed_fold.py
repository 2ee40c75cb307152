"""The embedder backward's three folded sweeps (patch_embed.FOLD): BatchNorm-1's backward formed inside the first conv's
weight gradient (csrc/embed.hip), the groups' row sums of f out of the conv2 forward's epilogue and the max-pool gradient
added where df is stored (csrc/rows3_kernel.h conv3_kernel's epilogue).  Two of the three are compared bit for bit with the
launches they replace: the group sums add a group's rows in the sweep's row order, so they are compared bit for bit too (and
against the bound of a 32-term sum in any order); a deterministic step computes the same bits with the folds and without."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from point_dae_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


class _arith:
    """the GEMM arithmetic for a block: 1 = exact-split bf16 (the default), 0 = fp32-input MFMA (PDAE_GEMM=f32mfma)"""

    def __init__(self, arith):
        self.arith = arith

    def __enter__(self):
        self.prev = _lib().gemm_arith()
        _lib().set_gemm_arith(self.arith)

    def __exit__(self, *exc):
        _lib().set_gemm_arith(self.prev)


# ---- 1. BatchNorm-1 backward + first conv's weight gradient -------------------------------------------------------

def _bn1_case(R, C):
    g = _gen(100 + R + C)
    y1 = torch.randn(R, C, device='cuda', generator=g) * 0.7 + torch.linspace(-1.0, 2.0, C, device='cuda')   # off-centre channels
    d1 = torch.randn(R, C, device='cuda', generator=g) + 0.25
    x = torch.randn(R, 3, device='cuda', generator=g) + torch.tensor([0.5, -0.3, 0.1], device='cuda')
    gamma = torch.rand(C, device='cuda', generator=g) + 0.5
    beta = torch.randn(C, device='cuda', generator=g) * 0.3
    if R:
        mean, var = y1.mean(0), y1.var(0, unbiased=False)
    else:
        mean, var = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    invstd = (var + 1e-5).rsqrt()
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    on = (y1 * scale + shift) > 0
    t = torch.where(on, d1, torch.zeros_like(d1)).double()
    xhat = (y1.double() - mean.double()) * invstd.double()
    S = torch.stack([t.sum(0), (t * xhat).sum(0)]).float().contiguous()
    return dict(y1=y1, d1=d1, x=x, gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift, S=S, t=t, xhat=xhat)


@pytest.mark.parametrize('R,C', [(32, 128), (1056, 128), (2080, 64), (0, 128)])
def test_bnrelu_backward_conv1_weight_equals_the_two_launches(R, C):
    """pdae_embed_bnrelu_backward_conv1_weight against pdae_bnrelu_backward_apply (in place) + pdae_embed_conv1_backward_weight:
    part and dW1 bit for bit, d1 untouched; (1056, 128) also against fp64 within test_gpu_gemm.py::test_conv1_backward_weight's
    bound (2e-5 of the largest entry of dW)."""
    L = _lib()
    c = _bn1_case(R, C)
    p = L.ptr
    parts = L.lib().pdae_embed_conv1_backward_weight_parts(R)
    d_pair = c['d1'].clone()
    part_pair = torch.full((parts, 3, C), float('nan'), device='cuda')
    L.call('pdae_bnrelu_backward_apply', d_pair, R // 32, C, p(d_pair), p(c['y1']), p(c['scale']), p(c['shift']), p(c['mean']),
           p(c['invstd']), p(c['gamma']), p(c['S']), None, R // 32, None, None, None)
    L.call('pdae_embed_conv1_backward_weight', d_pair, R, C, p(d_pair), p(c['x']), p(part_pair))
    d_keep = c['d1'].clone()
    part = torch.full((parts, 3, C), float('nan'), device='cuda')
    L.call('pdae_embed_bnrelu_backward_conv1_weight', d_keep, R, C, p(d_keep), p(c['y1']), p(c['scale']), p(c['shift']),
           p(c['mean']), p(c['invstd']), p(c['gamma']), p(c['S']), p(c['x']), p(part))
    assert torch.equal(d_keep, c['d1'])
    assert torch.equal(part, part_pair)
    dw, dw_pair = torch.full((C, 3), float('nan'), device='cuda'), torch.full((C, 3), float('nan'), device='cuda')
    L.call('pdae_partials_sum_t', part, parts, 3, C, p(part), p(dw))
    L.call('pdae_partials_sum_t', part, parts, 3, C, p(part_pair), p(dw_pair))
    assert torch.equal(dw, dw_pair)
    if R == 1056:
        k = (c['gamma'] * c['invstd']).double()
        dx = k * (c['t'] - c['S'][0].double() / R - c['xhat'] * (c['S'][1].double() / R))
        want = dx.t() @ c['x'].double()                                  # (C, 3)
        err = (dw.double() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        print('dW1 against fp64: %.3g of its largest entry' % err)
        assert err <= 2e-5, err


# ---- 2. group sums out of the conv2 forward's epilogue ---------------------------------------------------------------

@pytest.mark.parametrize('arith', [1, 0])
@pytest.mark.parametrize('M,N,K', [(32, 32, 32), (160, 256, 128), (16640, 256, 128)])
def test_store_groupmax_sum(M, N, K, arith):
    """pdae_embed_bnrelu_conv_store_groupmax_sum: f, g, arg2 bit for bit the plain entry's; gsum against the fp64 sum of the 32
    stored fp32 values within the bound of a 32-term fp32 sum in any order, 31 * 2^-24 * sum |f_r| (31 roundings, each at most half
    an ulp of a partial sum that |.| bounds by sum |f_r|), and bit for bit pdae_group_sum_listed's sums of the stored rows (the
    epilogue adds the rows in that sweep's order: the training step's numbers do not change with the fold)."""
    L = _lib()
    p = L.ptr
    G = M // 32
    g = _gen(200 + M)
    x = torch.randn(M, K, device='cuda', generator=g) + torch.linspace(-0.5, 1.0, K, device='cuda')
    sc = torch.rand(K, device='cuda', generator=g) + 0.5
    sh = torch.randn(K, device='cuda', generator=g) * 0.3
    w = torch.randn(N, K, device='cuda', generator=g) / K ** 0.5
    b = torch.randn(N, device='cuda', generator=g)
    with _arith(arith):
        y0, gm0 = torch.full((M, N), float('nan'), device='cuda'), torch.full((G, N), float('nan'), device='cuda')
        ga0 = torch.full((G, N), 255, device='cuda', dtype=torch.uint8)
        L.call('pdae_embed_bnrelu_conv_store_groupmax', x, M, N, K, p(x), p(sc), p(sh), p(w), p(b), p(y0), p(gm0), p(ga0))
        y, gm, gs = (torch.full((M, N), float('nan'), device='cuda'), torch.full((G, N), float('nan'), device='cuda'),
                     torch.full((G, N), float('nan'), device='cuda'))
        ga = torch.full((G, N), 255, device='cuda', dtype=torch.uint8)
        L.call('pdae_embed_bnrelu_conv_store_groupmax_sum', x, M, N, K, p(x), p(sc), p(sh), p(w), p(b), p(y), p(gm), p(ga), p(gs))
    assert torch.equal(y, y0) and torch.equal(gm, gm0) and torch.equal(ga, ga0)
    f64 = y.double().view(G, 32, N)
    err = (gs.double() - f64.sum(1)).abs()
    bound = 31 * 2.0 ** -24 * f64.abs().sum(1)
    print('gsum: worst error / bound = %.3g' % float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    every = torch.arange(G, device='cuda', dtype=torch.int32)
    swept = torch.full((G, N), float('nan'), device='cuda')
    L.call('pdae_group_sum_listed', y, G, N, p(y), p(every), p(swept))
    assert torch.equal(gs, swept)


@pytest.mark.parametrize('Gm,BG,C3,C2', [(6016, 8192, 512, 256), (1, 4, 8, 4), (0, 4, 8, 4)])
def test_masked_prep_fsum(Gm, BG, C3, C2):
    """pdae_embed_masked_prep_fsum: xe and wv bit for bit pdae_embed_masked_prep's, fsum_m = gsum[masked] bit for bit."""
    L = _lib()
    p = L.ptr
    g = _gen(300 + Gm)
    uv, gb, wl = (torch.randn(2, C3, device='cuda', generator=g), torch.randn(BG, C3, device='cuda', generator=g),
                  torch.randn(C3, C2, device='cuda', generator=g))
    gsum = torch.randn(BG, C2, device='cuda', generator=g)
    masked = torch.randperm(BG, device='cuda', generator=g)[:Gm].to(torch.int32)
    xe0, wv0 = torch.empty(Gm, C3, device='cuda'), torch.empty(C3, C2, device='cuda')
    L.call('pdae_embed_masked_prep', uv, Gm, C3, C2, p(uv), p(gb), p(masked), p(wl), p(xe0), p(wv0))
    xe, wv = torch.full((Gm, C3), float('nan'), device='cuda'), torch.full((C3, C2), float('nan'), device='cuda')
    fs = torch.full((Gm, C2), float('nan'), device='cuda')
    L.call('pdae_embed_masked_prep_fsum', uv, Gm, C3, C2, p(uv), p(gb), p(masked), p(wl), p(xe), p(wv), p(gsum), p(fs))
    assert torch.equal(xe, xe0) and torch.equal(wv, wv0)
    assert torch.equal(fs, gsum.index_select(0, masked.long()))


# ---- 3. the max-pool gradient added where df is stored ---------------------------------------------------------------

def _scatter_case(BG, lists, N, K, arith):
    """df from the two listed products: reference = pdae_group_gemm_scatter twice + pdae_group_scatter_add over all groups;
    folded = pdae_group_gemm_scatter_add twice.  The first list gathers its rows and has a per-group bias, the second reads a
    compact operand (the embedder's two calls)."""
    L = _lib()
    p = L.ptr
    g = _gen(400 + BG + K)
    src = torch.randn(BG * 32, K, device='cuda', generator=g)
    w = torch.randn(N, K, device='cuda', generator=g) / K ** 0.5
    dg = torch.randn(BG, N, device='cuda', generator=g)
    arg = torch.randint(0, 32, (BG, N), device='cuda', generator=g).to(torch.uint8)
    arg[:, 0], arg[:, 1] = 0, 31
    arg[:, N - 1] = 31
    la, lb = [torch.tensor(l, device='cuda', dtype=torch.int32) for l in lists]
    gbias = torch.randn(max(la.numel(), 1), N, device='cuda', generator=g)
    rows_b = (lb.long().unsqueeze(1) * 32 + torch.arange(32, device='cuda')).reshape(-1)
    xb = src[rows_b].contiguous() if lb.numel() else src[:0]
    out = []
    with _arith(arith):
        for fold in (False, True):
            df = torch.full((BG * 32, N), float('nan'), device='cuda')
            if fold:
                L.call('pdae_group_gemm_scatter_add', src, la.numel() * 32, N, K, p(src), p(la), p(w), p(gbias), p(df), N, p(la),
                       p(dg), p(arg))
                L.call('pdae_group_gemm_scatter_add', src, lb.numel() * 32, N, K, p(xb), None, p(w), None, p(df), N, p(lb),
                       p(dg), p(arg))
            else:
                L.call('pdae_group_gemm_scatter', src, la.numel() * 32, N, K, p(src), p(la), p(w), p(gbias), p(df), N, p(la))
                L.call('pdae_group_gemm_scatter', src, lb.numel() * 32, N, K, p(xb), None, p(w), None, p(df), N, p(lb))
                L.call('pdae_group_scatter_add', src, BG, N, p(dg), p(arg), p(df))
            out.append(df)
    assert not torch.isnan(out[0]).any()
    assert torch.equal(out[0], out[1])
    # (the add did happen: the reference differs from the plain products at the arg-max rows)
    assert float(dg.abs().min()) > 0


@pytest.mark.parametrize('arith', [1, 0])
@pytest.mark.parametrize('N,K', [(256, 256), (256, 512)])
def test_group_gemm_scatter_add_five_groups(N, K, arith):
    _scatter_case(5, ([0, 3], [1, 2, 4]), N, K, arith)


def test_group_gemm_scatter_add_one_list_empty():
    _scatter_case(1, ([0], []), 256, 256, 1)
    _scatter_case(1, ([], [0]), 256, 256, 1)


def test_group_gemm_scatter_add_persistent_form():
    """The first list is 132 row tiles of 128 rows, x 2 column tiles = 264 tiles: 33 per XCD > 32 with K / 32 = 8, so the
    persistent blocks walk more than one tile (an epilogue while the next tile's loads are in flight)."""
    BG = 132 * 4 + 8
    perm = torch.randperm(BG, generator=torch.Generator().manual_seed(7)).tolist()
    _scatter_case(BG, (perm[:132 * 4], perm[132 * 4:]), 256, 256, 1)


def test_group_gemm_scatter_add_without_a_gradient_is_the_plain_scatter():
    L = _lib()
    p = L.ptr
    g = _gen(9)
    src = torch.randn(64, 64, device='cuda', generator=g)
    w = torch.randn(32, 64, device='cuda', generator=g)
    lst = torch.tensor([1, 0], device='cuda', dtype=torch.int32)
    a, b = torch.zeros(64, 32, device='cuda'), torch.zeros(64, 32, device='cuda')
    L.call('pdae_group_gemm_scatter', src, 64, 32, 64, p(src), None, p(w), None, p(a), 32, p(lst))
    L.call('pdae_group_gemm_scatter_add', src, 64, 32, 64, p(src), None, p(w), None, p(b), 32, p(lst), None, None)
    assert torch.equal(a, b)


# ---- 4. the step ------------------------------------------------------------------------------------------------------

def _step_runs(monkeypatch, settings):
    """test_gpu_glue.py's step (depth 2 + 1, B = 8, drop-path 0, the same seeds) once per (FOLD, FOLD_PARTS) setting ->
    [(loss, loss_n, flat_grad, [(name, offset, count)], names of the entries the step called)]"""
    import random
    import numpy as np
    from point_dae_amd import _lib, builder, patch_embed
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.graph_step import GraphedTrainStep
    from point_dae_amd.synthetic import shapenet_like_clouds
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    config = cfg_from_yaml_file(os.path.join(root, 'cfgs', 'pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml'))
    config.model.transformer_config.drop_path_rate = 0.0
    config.model.transformer_config.depth = 2
    config.model.transformer_config.decoder_depth = 1
    B = 8
    x = torch.from_numpy(shapenet_like_clouds(B, 1024, seed=9)).cuda()
    out = []
    for fold, parts in settings:
        monkeypatch.setattr(patch_embed, 'FOLD', fold)
        monkeypatch.setattr(patch_embed, 'FOLD_PARTS', parts)
        torch.manual_seed(0)
        model = FlatDataParallel(builder.model_builder(config.model).cuda().train())
        opt, _ = builder.build_opti_sche(model, config)
        step = GraphedTrainStep(model, opt, config, B, 1024, warmup_eager=1)
        step.pts.copy_(x)
        random.seed(4), np.random.seed(4), torch.manual_seed(4)
        called = set()
        monkeypatch.setattr(_lib, 'CALL_HOOK', lambda name, args: called.add(name))
        lx, ln = step._fwd_bwd(step._draw())
        monkeypatch.setattr(_lib, 'CALL_HOOK', None)
        torch.cuda.synchronize()
        out.append((lx.clone(), ln.clone(), model.flat_grad.clone(), [(n, o, c) for n, (o, c) in zip(model.names, model.offsets)],
                    called))
    return out


_FOLDED = {'a': 'pdae_embed_bnrelu_backward_conv1_weight', 'b': 'pdae_embed_bnrelu_conv_store_groupmax_sum',
           'c': 'pdae_group_gemm_scatter_add'}
_SWEEPS = {'a': 'pdae_embed_conv1_backward_weight', 'b': 'pdae_group_sum_listed', 'c': 'pdae_group_scatter_add'}


def _check_calls(called, parts):
    """the step ran the folded entry of every part in `parts` and the stand-alone sweep of every other part"""
    for k in 'abc':
        assert ((_FOLDED if k in parts else _SWEEPS)[k] in called) and ((_SWEEPS if k in parts else _FOLDED)[k] not in called), (k, parts)


def test_a_step_with_the_folded_sweeps_equals_the_step_without(monkeypatch):
    """FOLD on against off: the losses agree bit for bit (the forward changes no stored value) and every gradient within
    test_gpu_glue.py's bound for re-associated backward sums, 2e-6 max|tensor| + 1e-7 max|flat_grad|."""
    on, off = _step_runs(monkeypatch, [(True, 'abc'), (False, 'abc')])
    _check_calls(on[4], 'abc'), _check_calls(off[4], '')
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    gmax = float(off[2].abs().max())
    worst = 0.0
    for name, o, n in on[3]:
        a, b = on[2][o:o + n], off[2][o:o + n]
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        worst = max(worst, err / (2e-6 * scale + 1e-7 * gmax))
        assert err <= 2e-6 * scale + 1e-7 * gmax, (name, err, scale, gmax)
    print('worst gradient difference / bound = %.3g' % worst)


def test_a_folded_step_is_bit_identical_in_deterministic_mode(monkeypatch):
    """In deterministic mode the loss and every gradient of the step with all three folds, and with the group sums left to their
    sweep (BatchNorm-1 into the weight gradient and the pool gradient into df's stores alone), equal the unfolded step's bit for
    bit."""
    L = _lib()
    L.set_deterministic(True)
    try:
        on, two, off = _step_runs(monkeypatch, [(True, 'abc'), (True, 'ac'), (False, 'abc')])
    finally:
        L.set_deterministic(False)
    _check_calls(on[4], 'abc'), _check_calls(two[4], 'ac'), _check_calls(off[4], '')
    for got in (on, two):
        assert torch.equal(got[0], off[0]) and torch.equal(got[1], off[1])
        for name, o, n in got[3]:
            assert torch.equal(got[2][o:o + n], off[2][o:o + n]), name


# ---- 5. argument checks -------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    L = _lib()
    t = torch.empty(32 * 128, device='cuda')
    p = L.ptr(t)
    bad = [
        ('pdae_embed_bnrelu_backward_conv1_weight', (32, 128, None, p, p, p, p, p, p, p, p, p)),            # null d
        ('pdae_embed_bnrelu_backward_conv1_weight', (32, 128, p, p, p, p, p, p, p, p, p, None)),            # null part
        ('pdae_embed_bnrelu_backward_conv1_weight', (32, 24, p, p, p, p, p, p, p, p, p, p)),                # C/4 = 6
        ('pdae_embed_bnrelu_conv_store_groupmax_sum', (32, 32, 32, p, p, p, p, p, p, p, p, None)),          # null gsum
        ('pdae_embed_bnrelu_conv_store_groupmax_sum', (40, 32, 32, p, p, p, p, p, p, p, p, p)),             # M % 32
        ('pdae_group_gemm_scatter_add', (40, 32, 32, p, None, p, None, p, 32, p, p, p)),                    # M % 32
        ('pdae_group_gemm_scatter_add', (32, 32, 32, p, None, p, None, p, 32, None, p, p)),                 # null c_groups
        ('pdae_group_gemm_scatter_add', (32, 32, 32, p, None, p, None, p, 32, p, p, None)),                 # sgrad without sarg
        ('pdae_embed_masked_prep_fsum', (1, 8, 4, p, p, p, p, p, p, None, p)),                              # null gsum
        ('pdae_embed_masked_prep_fsum', (1, 6, 4, p, p, p, p, p, p, p, p)),                                 # C3 % 4
    ]
    for name, args in bad:
        with pytest.raises(RuntimeError):
            L.call(name, t, *args)
