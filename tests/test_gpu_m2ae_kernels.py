"""The eight entry points of csrc/m2ae.hip one by one: each is called directly (through its wrapper of
point_dae_amd/point_m2ae.py where it has one, and through point_dae_amd._lib with the wrapper's argument list) and held to
a plain reference of the same operation.  tests/test_gpu_m2ae.py reaches seven of them only inside the two token embedders
and H_Encoder.forward, at one model.

Conventions: every test is seeded; output buffers are NaN-filled (int32 outputs: SENTINEL) and nothing may keep its fill;
the outputs of pack, unpack, compact, embed_tail (and of the three per-patch kernels) are carved out of a larger filled
allocation whose GUARD rows on both sides must keep their fill; errors are max norms relative to the largest reference
output (test_gpu_m2ae._rel).  The references are the plain functions ref_*; tests/test_m2ae_kernel_refs_cpu.py holds them
to tests/m2ae_restatement.py on a machine without a GPU.

    kernel                  reference                       yardstick                            tolerance rule             error / yardstick per case, measured on an MI355X
    m2ae_embed_tail         the literal formula, fp64       e_layers: linear_any(relu) +         err <= 4 e_layers and      0.87 1.57 1.27 1.69 2.79 1.66 0.89 (error <= 6.7e-7)
                                                            rows_gemm + torch max, fp32 MFMA     err <= 1e-5
                            a patch with gb = -1000         --                                   tok[p] bit-equal to b4     exact
    m2ae_group_max          torch max over the patch, fp32  --                                   bit-equal                  exact
    m2ae_gather_max         x[idx] max over k, fp32         --                                   bit-equal, no inf          exact
    m2ae_gather_add_relu    relu(x[idx] + g[patch]), fp32   --                                   bit-equal, no inf          exact
    m2ae_compact            ascending visible indices       --                                   equal                      exact
    m2ae_pack / unpack      plain indexing                  --                                   bit-equal, zeros behind    exact
                                                                                                 len, other rows untouched
    attention_local         R.attention on R.attention_mask e_old: the unmasked core against     err <= 4 e_old             1.94 1.21 2.18 0.82 1.04 1.30 (e_old 3.773e-7)
      (score std 2)         in fp64                         fp64 at (2, 64, 6, 64)
    attention_local         the same                        R.attention in fp32 torch on the     err <= 4 yardstick         1.16 (kernel 1.923e-6, yardstick 1.655e-6)
      (score std 8)                                         device, the fp64-decided mask

The 4 of embed_tail is what tests/test_gpu_partseg.py and tests/test_gpu_sa_eval.py give a new kernel of the arithmetic
class of its yardstick, the 1e-5 the project's pin for evaluation-mode features; the 4 of the peaked attention case is the
rule of tests/test_gpu_pretrain_kernels.py (two bits for a different, equally legitimate evaluation order).  ReLU, max and
the softmax are continuous and no attention case has a mask decision within 1e-6 of the radius (asserted), so no element
is left out of any comparison (radius 0 leaves a padded query no key: there the kernel's exact zeros are asserted).
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import m2ae_restatement as R  # noqa: E402
from test_gpu_m2ae import _qkv, _rel, _split64, e_old  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FACTOR = 4.0
PIN = 1e-5
GUARD = 8
SENTINEL = -7777


def _L():
    from point_dae_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(rows, cols, dtype=torch.float32):
    """-> (whole, out): out = rows GUARD .. GUARD + rows of a (rows + 2 GUARD, cols) allocation filled with NaN / SENTINEL."""
    whole = torch.full((rows + 2 * GUARD, cols), float('nan') if dtype.is_floating_point else SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows]


def _guards_kept(*wholes):
    for w in wholes:
        for g in (w[:GUARD], w[-GUARD:]):
            kept = torch.isnan(g).all() if w.dtype.is_floating_point else (g == SENTINEL).all()
            assert bool(kept), 'a kernel wrote outside its output buffer'


def _written(*outs):
    for t in outs:
        assert bool(torch.isfinite(t).all() if t.dtype.is_floating_point else (t != SENTINEL).all()), 'an output kept its fill'


# ===================================================================================================================
# 1. pdae_m2ae_embed_tail
# ===================================================================================================================
EMBED_TAIL_CASES = [(1, 4, 8, 128, 32),        # one block holding four rows; K is one step; three waves without an output tile
                    (9, 4, 8, 128, 32),        # R = 36: the last block holds one patch
                    (67, 4, 24, 128, 128),     # all four waves own output tiles; R = 268
                    (5, 8, 64, 256, 64),       # R = 40
                    (3, 16, 256, 512, 96),     # the shipped widths; R = 48, a half-filled last block
                    (1, 32, 256, 512, 128),    # one patch fills the block
                    (3, 32, 40, 384, 96)]      # N3 spans three activation steps


def embed_tail_inputs(P, n, K, N3, N4):
    gen = torch.Generator().manual_seed(100000 * P + 1000 * n + K + N3 + N4)
    F = torch.randn(P * n, K, generator=gen)
    Wl = torch.randn(N3, K, generator=gen) / K ** 0.5
    gb = torch.randn(P, N3, generator=gen)
    W4 = torch.randn(N4, N3, generator=gen) / N3 ** 0.5
    b4 = 0.1 * torch.randn(N4, generator=gen)
    return F, Wl, gb, W4, b4


def ref_embed_tail(F, n, Wl, gb, W4, b4):
    """tok[p] = max_j(relu(F[p n + j] . Wl^T + gb[p]) . W4^T) + b4, in fp64 (fp64 inputs stay what they are)."""
    F, Wl, gb, W4, b4 = (t.double() for t in (F, Wl, gb, W4, b4))
    h = torch.relu(F @ Wl.t() + gb.repeat_interleave(n, 0))
    return (h @ W4.t()).reshape(-1, n, W4.shape[0]).max(1)[0] + b4


def layers_embed_tail(F, n, Wl, gb, W4, b4):
    """The same formula on kernels older than m2ae.hip, in the fp32-input MFMA arithmetic: relu(F Wl^T + gb[patch]) as one
    linear_any(relu=True) on the rows [F | one-hot(patch)] against [Wl | gb^T] (the patch's term enters as an exact
    product with 1), rows_gemm with b4 on the (R, N3) rows, torch's max over the patch."""
    from point_dae_amd import _lib
    from point_dae_amd.rows import linear_any, rows_gemm
    P = gb.shape[0]
    onehot = torch.eye(P, device=F.device).repeat_interleave(n, 0)
    before = _lib.gemm_arith()
    _lib.set_gemm_arith(_lib.GEMM_F32MFMA)
    try:
        with torch.no_grad():
            h = linear_any(torch.cat([F, onehot], 1).contiguous(), torch.cat([Wl, gb.t()], 1).contiguous(), None, relu=True)
            t = rows_gemm(h.contiguous(), W4, False, b4)
        torch.cuda.synchronize()
    finally:
        _lib.set_gemm_arith(before)
    return t.reshape(P, n, -1).max(1)[0]


def run_embed_tail(F, n, Wl, gb, W4, b4):
    """the direct call into a guarded NaN-filled buffer"""
    L = _L()
    R_, K = F.shape
    whole, tok = _guarded(R_ // n, W4.shape[0])
    L.call('pdae_m2ae_embed_tail', F, R_, n, K, Wl.shape[0], W4.shape[0], L.ptr(F), L.ptr(Wl), L.ptr(gb), L.ptr(W4),
           L.ptr(b4), L.ptr(tok))
    torch.cuda.synchronize()
    _guards_kept(whole)
    _written(tok)
    return tok


@pytest.mark.parametrize('P,n,K,N3,N4', EMBED_TAIL_CASES)
def test_embed_tail_against_the_fp64_formula(P, n, K, N3, N4):
    from point_dae_amd.point_m2ae import embed_tail
    host = embed_tail_inputs(P, n, K, N3, N4)
    F, Wl, gb, W4, b4 = (t.to(DEV).contiguous() for t in host)
    tok = run_embed_tail(F, n, Wl, gb, W4, b4)
    again = embed_tail(F, n, Wl, gb, W4, b4)                       # the wrapper: the same call once more, the same bits
    assert tok.shape == (P, N4) and _same_bits(again, tok)
    want = ref_embed_tail(host[0], n, *host[1:])
    err = _rel(tok, want)
    e_layers = _rel(layers_embed_tail(F, n, Wl, gb, W4, b4), want)
    print('embed_tail P %d n %d K %d N3 %d N4 %d: error %.3e, e_layers %.3e (ratio %.2f)'
          % (P, n, K, N3, N4, err, e_layers, err / max(e_layers, 1e-30)))
    # a patch whose activations are all zero: 0 . W4^T = 0 and 0 + b4 = b4 exactly; every other patch keeps its bits
    p = P // 2
    gb_dead = gb.clone()
    gb_dead[p] = -1000.0
    assert float((host[0].double() @ host[1].double().t()).abs().max()) < 100.0
    dead = run_embed_tail(F, n, Wl, gb_dead, W4, b4)
    assert _same_bits(dead[p], b4)
    keep = torch.arange(P) != p
    assert _same_bits(dead.cpu()[keep], tok.cpu()[keep])
    assert float(ref_embed_tail(host[0], n, host[1], gb_dead.cpu(), host[3], host[4])[p].sub(host[4].double()).abs().max()) == 0.0
    assert err <= FACTOR * e_layers and err <= PIN, (err, e_layers)


# ===================================================================================================================
# 2. pdae_m2ae_group_max, pdae_m2ae_gather_max, pdae_m2ae_gather_add_relu
# ===================================================================================================================
def ref_group_max(x, P, n):
    return x.reshape(P, n, -1).max(1)[0]


def ref_gather_max(x, idx, P, k):
    return x[idx].reshape(P, k, -1).max(1)[0]


def ref_gather_add_relu(x, idx, g, k):
    return torch.relu(x[idx] + g.repeat_interleave(k, 0))


@pytest.mark.parametrize('P,n,C', [(1, 1, 4), (7, 3, 12), (5, 32, 96), (300, 16, 256)])
def test_group_max_bit_for_bit(P, n, C):
    from point_dae_amd.point_m2ae import group_max
    L = _L()
    gen = torch.Generator().manual_seed(1000 * P + 10 * n + C)
    x = torch.randn(P * n, C, generator=gen) - 3.0               # most maxima negative, no exact zero
    want = ref_group_max(x, P, n)
    assert float((want < 0).float().mean()) > 0.5 and not bool((x == 0).any())
    xd = x.to(DEV)
    whole, out = _guarded(P, C)
    L.call('pdae_m2ae_group_max', xd, P, n, C, L.ptr(xd), L.ptr(out))
    torch.cuda.synchronize()
    _guards_kept(whole)
    assert _same_bits(out, want) and _same_bits(group_max(xd, P, n), want)
    assert _same_bits(xd, x)                                       # the input is read only


GATHER_CASES = [(1, 1, 1, 4), (72, 24, 8, 96), (40, 10, 4, 192), (100, 515, 8, 8)]


def gather_inputs(S, P, k, C):
    """table x (S, C), per-patch term g (P, C), idx (P*k,) int64: drawn below the top quarter of the table, some rows
    repeated, rows 0 and S - 1 always among them (S - 1 is the one referenced row of the top quarter); every row idx does
    not name is +inf, which fmaxf would keep and a sum would keep."""
    gen = torch.Generator().manual_seed(1000 * S + 10 * P + k + C)
    x = torch.randn(S, C, generator=gen)
    g = torch.randn(P, C, generator=gen)
    idx = torch.randint(0, S - S // 4, (P * k,), generator=gen)
    if P * k >= 8:
        idx[:3] = idx[3:6]                                         # repeats, whatever was drawn
        idx[-1], idx[-2] = S - 1, 0
    unref = torch.ones(S, dtype=torch.bool)
    unref[idx] = False
    x[unref] = float('inf')
    return x, g, idx, unref


@pytest.mark.parametrize('S,P,k,C', GATHER_CASES)
def test_gather_max_and_gather_add_relu_bit_for_bit(S, P, k, C):
    L = _L()
    x, g, idx, unref = gather_inputs(S, P, k, C)
    assert idx.dtype == torch.int64 and int(idx.min()) == 0 and int(idx.max()) == S - 1
    if S >= 4:
        assert bool(unref[S - S // 4:S - 1].all()) and len(set(idx.tolist())) < idx.numel()
    xd, gd, idxd = x.to(DEV), g.to(DEV), idx.to(DEV)
    whole_m, out_m = _guarded(P, C)
    L.call('pdae_m2ae_gather_max', xd, P, k, C, L.ptr(xd), L.ptr(idxd), L.ptr(out_m))
    whole_a, out_a = _guarded(P * k, C)
    L.call('pdae_m2ae_gather_add_relu', xd, P, k, C, L.ptr(xd), L.ptr(idxd), L.ptr(gd), L.ptr(out_a))
    torch.cuda.synchronize()
    _guards_kept(whole_m, whole_a)
    _written(out_m, out_a)                                         # finite: no NaN fill left and no inf read
    assert _same_bits(out_m, ref_gather_max(x, idx, P, k))
    assert _same_bits(out_a, ref_gather_add_relu(x, idx, g, k))
    assert _same_bits(xd, x) and torch.equal(idxd.cpu(), idx)


# ===================================================================================================================
# 3. pdae_m2ae_compact, pdae_m2ae_pack, pdae_m2ae_unpack
# ===================================================================================================================
COMPACT_G = [1, 63, 64, 65, 72, 256, 512]


def compact_rows(G):
    """name -> masked (G,) bool, in the order of the batch"""
    gen = torch.Generator().manual_seed(G)
    ar = torch.arange(G)
    rows = {'all visible': torch.zeros(G, dtype=torch.bool), 'all masked': torch.ones(G, dtype=torch.bool),
            'alternating': ar % 2 == 1, 'last only': ar != G - 1}
    if G >= 65:
        rows['63 and 64'] = ~((ar == 63) | (ar == 64))
    rows['0.8 masked'] = torch.rand(G, generator=gen) < 0.8
    rows['0.2 masked'] = torch.rand(G, generator=gen) < 0.2
    return rows


def ref_compact(masked):
    """masked (B, G) bool -> lens (B,) int32 = the visible count, ids (B, G) int32 = the visible indices ascending, then -1"""
    B, G = masked.shape
    lens = torch.zeros(B, dtype=torch.int32)
    ids = torch.full((B, G), -1, dtype=torch.int32)
    for b in range(B):
        vis = [g for g in range(G) if not bool(masked[b, g])]
        lens[b] = len(vis)
        ids[b, :len(vis)] = torch.tensor(vis, dtype=torch.int32)
    return lens, ids


def ref_pack(tokens, centres, ids, lens, B, G, Tp):
    """tokens (B*G, C), centres (B*G, 3) -> x (B*Tp, C), cen (B*Tp, 3): plain indexing, zeros behind len[b]"""
    C = tokens.shape[1]
    x, cen = tokens.new_zeros(B, Tp, C), centres.new_zeros(B, Tp, 3)
    for b in range(B):
        n = int(lens[b])
        x[b, :n] = tokens.reshape(B, G, C)[b, ids[b, :n].long()]
        cen[b, :n] = centres.reshape(B, G, 3)[b, ids[b, :n].long()]
    return x.reshape(B * Tp, C), cen.reshape(B * Tp, 3)


def ref_unpack(table, x, ids, lens, B, G, Tp):
    """rows t < len[b] of x (B*Tp, C) -> rows ids[b][t] of a copy of table (B*G, C); every other row is the table's"""
    C = table.shape[1]
    out = table.clone().reshape(B, G, C)
    for b in range(B):
        n = int(lens[b])
        out[b, ids[b, :n].long()] = x.reshape(B, Tp, C)[b, :n]
    return out.reshape(B * G, C)


@pytest.mark.parametrize('G', COMPACT_G)
def test_compact_counts_and_ascending_ids(G):
    from point_dae_amd.point_m2ae import compact_visible
    L = _L()
    rows = compact_rows(G)
    masked = torch.stack(list(rows.values()))
    B = masked.shape[0]
    assert B == (7 if G >= 65 else 6)
    want_lens, want_ids = ref_compact(masked)
    assert int(want_lens[0]) == G and int(want_lens[1]) == 0 and int(want_lens[3]) == 1
    lens, ids = compact_visible(masked.to(DEV))                    # the wrapper, on a bool mask
    assert torch.equal(lens.cpu(), want_lens) and torch.equal(ids.cpu(), want_ids)
    m8 = (masked.to(torch.uint8) * 255).to(DEV)                    # any non-zero byte is "masked"
    whole_l, lens_g = _guarded(B, 1, torch.int32)
    whole_i, ids_g = _guarded(B, G, torch.int32)
    L.call('pdae_m2ae_compact', m8, B, G, L.ptr(m8), L.ptr(lens_g), L.ptr(ids_g))
    torch.cuda.synchronize()
    _guards_kept(whole_l, whole_i)
    assert torch.equal(lens_g.cpu().reshape(-1), want_lens) and torch.equal(ids_g.cpu(), want_ids)


PACK_CASES = [(3, 72, 96, ['0.2 masked', 'all masked', 'alternating']),
              (2, 512, 4, ['0.2 masked', 'all masked']),
              (4, 65, 384, ['all visible', 'all masked', '63 and 64', '0.8 masked'])]      # max len = G: T_pad = G either way


def pack_inputs(B, G, C, names):
    rows = compact_rows(G)
    masked = torch.stack([rows[n] for n in names])
    lens, ids = ref_compact(masked)
    gen = torch.Generator().manual_seed(1000 * B + G + C)
    tokens = torch.randn(B * G, C, generator=gen)
    centres = torch.randn(B * G, 3, generator=gen)
    return masked, lens, ids, tokens, centres


def run_pack(B, G, Tp, C, ids, lens, tokens, centres):
    L = _L()
    whole_x, x = _guarded(B * Tp, C)
    whole_c, cen = _guarded(B * Tp, 3)
    L.call('pdae_m2ae_pack', tokens, B, G, Tp, C, L.ptr(ids), L.ptr(lens), L.ptr(tokens), L.ptr(centres), L.ptr(x), L.ptr(cen))
    torch.cuda.synchronize()
    _guards_kept(whole_x, whole_c)
    return x, cen


def run_unpack(B, G, Tp, C, ids, lens, x, table):
    """table: host (B*G, C); it is copied into a guarded buffer, unpacked into in place and returned"""
    L = _L()
    whole, t = _guarded(B * G, C)
    t.copy_(table)
    L.call('pdae_m2ae_unpack', t, B, G, Tp, C, L.ptr(ids), L.ptr(lens), L.ptr(x), L.ptr(t))
    torch.cuda.synchronize()
    _guards_kept(whole)
    return t


@pytest.mark.parametrize('full_pad', [False, True], ids=['T_pad=max_len', 'T_pad=G'])
@pytest.mark.parametrize('B,G,C,names', PACK_CASES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_pack_and_unpack_against_plain_indexing(B, G, C, names, full_pad):
    masked, lens, ids, tokens, centres = pack_inputs(B, G, C, names)
    assert int(lens.min()) == 0                                    # one sample has no visible token
    Tp = G if full_pad else int(lens.max())
    idsd, lensd, tokd, ctrd = (t.to(DEV) for t in (ids, lens, tokens, centres))
    # pack
    x, cen = run_pack(B, G, Tp, C, idsd, lensd, tokd, ctrd)
    want_x, want_cen = ref_pack(tokens, centres, ids, lens, B, G, Tp)
    assert _same_bits(x, want_x) and _same_bits(cen, want_cen)
    behind = (torch.arange(Tp).unsqueeze(0) >= lens.unsqueeze(1)).reshape(-1)
    assert behind.any() and bool((_bits(x)[behind] == 0).all()) and bool((_bits(cen)[behind] == 0).all())      # +0.0, every bit
    assert _same_bits(tokd, tokens) and _same_bits(ctrd, centres)
    # unpack: rows of x behind len[b] are NaN and must never arrive
    gen = torch.Generator().manual_seed(7 + B + G + C)
    rows = torch.randn(B * Tp, C, generator=gen)
    rows[behind] = float('nan')
    table = run_unpack(B, G, Tp, C, idsd, lensd, rows.to(DEV), tokens)
    assert not bool(torch.isnan(table).any())
    vis = (~masked).reshape(-1)
    valid = ~behind
    assert _same_bits(table.cpu()[vis], rows[valid])               # both run sample by sample in ascending token order
    assert _same_bits(table.cpu()[~vis], tokens[~vis])             # dropped tokens keep their rows
    assert _same_bits(table, ref_unpack(tokens, rows, ids, lens, B, G, Tp))
    # pack, then unpack into a table whose visible rows were wiped: the table is back, bit for bit
    wiped = tokens.clone()
    wiped[vis] = 777.0
    assert _same_bits(run_unpack(B, G, Tp, C, idsd, lensd, x, wiped), tokens)


# ===================================================================================================================
# 4. pdae_attention_local_forward
# ===================================================================================================================
STD2, STD8 = 2.0 ** 0.5, 8.0 ** 0.5
#               B, T,   H, D,  lens,          radius, padded centres zeroed, q / k factor, min | |centre| - radius | (not zeroed: over the pairs)
ATTENTION_CASES = [(2, 200, 6, 64, [200, 187], 0.64, True, STD2, 1.1e-4),      # D = 64 (two d-tiles) with padding and a radius that bites
                   (2, 96, 6, 32, [0, 96], 0.64, True, STD2, 1.1e-3),          # a sample with no visible token
                   (2, 40, 6, 64, [40, 31], 0.0, True, STD2, None),            # radius 0: padded rows zero, valid rows compared
                   (1, 130, 1, 16, [129], 0.32, True, STD2, 1.1e-2),           # H = 1, two rows into a second query block
                   (3, 65, 3, 16, [65, 1, 64], 0.32, True, STD2, 1.4e-3),      # H = 3, one row into a second key stage
                   (2, 150, 6, 32, [140, 150], 0.64, False, STD2, 2.1e-3),     # padded rows keep their centres: 2900 pairs
                   (2, 133, 6, 32, [133, 120], 0.64, True, STD8, 6.9e-3)]      # score standard deviation near 8
MARGIN = 1e-6


def attention_inputs(B, T, H, D, lens, radius, zeroed, qk):
    """test_gpu_m2ae's generator (seed 100 T + D; _qkv, then centres uniform in the unit ball): the first H of _qkv's six
    heads, q and k at the factor qk -> qkv (B, T, 3, H, D), cen (B, T, 3), lens (B,) int32, valid (B, T)"""
    gen = torch.Generator().manual_seed(100 * T + D)
    qkv = _qkv(gen, B, T, D)[:, :, :, :H].contiguous()
    qkv[:, :, :2] *= qk / STD2                                     # (_qkv scaled q and k by 2^0.5)
    direction = torch.randn(B, T, 3, generator=gen)
    cen = direction / direction.norm(dim=-1, keepdim=True) * torch.rand(B, T, 1, generator=gen) ** (1.0 / 3.0)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    valid = torch.arange(T).unsqueeze(0) < lens_t.unsqueeze(1)
    if zeroed:
        cen = cen * valid.unsqueeze(-1)
    return qkv, cen, lens_t, valid


def ref_attention_margin(cen, valid, radius):
    """min |distance - radius| in fp64 over the pairs the radius decides (not both valid) -> (margin, pairs)"""
    c = cen.double()
    d = (c.unsqueeze(2) - c.unsqueeze(1)).pow(2).sum(-1).sqrt()
    decided = ~(valid.unsqueeze(2) & valid.unsqueeze(1))
    return float((d - radius).abs()[decided].min()), int(decided.sum())


def ref_attention(qkv, cen, lens_t, radius, dtype=torch.float64, device='cpu'):
    """R.attention on the explicit (B, T, T) mask, which is always decided in fp64 -> (B, T, H D) in `dtype`"""
    B, T, _, H, D = qkv.shape
    mask = R.attention_mask(cen.double(), lens_t.long(), radius)
    q, k, v = (t.to(device) for t in _split64(qkv))
    o = R.attention(q.to(dtype), k.to(dtype), v.to(dtype), D ** -0.5, mask.to(dtype).to(device))
    return o.transpose(1, 2).reshape(B, T, H * D)


@pytest.mark.parametrize('B,T,H,D,lens,radius,zeroed,qk,stated', ATTENTION_CASES,
                         ids=lambda v: str(v) if isinstance(v, list) else None)
def test_attention_local_against_the_fp64_definition(B, T, H, D, lens, radius, zeroed, qk, stated):
    from point_dae_amd.point_m2ae import attention_local
    qkv, cen, lens_t, valid = attention_inputs(B, T, H, D, lens, radius, zeroed, qk)
    if radius > 0:                       # no mask decision of the case hangs on rounding
        margin, pairs = ref_attention_margin(cen, valid, radius)
        assert margin >= MARGIN and pairs > 0, margin
    o = attention_local(qkv.reshape(B * T, 3 * H * D).to(DEV), cen.reshape(B * T, 3).to(DEV), lens_t.to(DEV), B, T, H,
                        D ** -0.5, radius)
    torch.cuda.synchronize()
    o = o.reshape(B, T, H * D).cpu()
    _written(o)
    want = ref_attention(qkv, cen, lens_t, radius)
    if radius == 0:
        assert bool((o[~valid] == 0).all())
        o, want = o[valid], want[valid]
    err = _rel(o, want)
    if qk == STD2:
        yard, name = e_old(), 'e_old'
    else:                                # e_old is measured at another score scale
        yard, name = _rel(ref_attention(qkv, cen, lens_t, radius, torch.float32, DEV), want), 'fp32 torch'
        scores = (_split64(qkv)[0] @ _split64(qkv)[1].transpose(-2, -1)) * D ** -0.5
        assert 6.0 < float(scores.std()) < 10.0
    print('attention_local B %d T %d H %d D %d lens %s radius %g: error %.3e, %s %.3e (ratio %.2f)'
          % (B, T, H, D, lens, radius, err, name, yard, err / yard))
    assert err <= FACTOR * yard, (err, yard)


# ===================================================================================================================
# 5. refusals: null pointers everywhere, so a refusal that comes late faults nothing -- it answers "null pointer"
# ===================================================================================================================
def test_refused_arguments_return_their_status_before_anything_is_read():
    from point_dae_amd import _lib
    lib = _lib.lib()
    BAD, UNSUPPORTED, OK = _lib.CONST['PDAE_ERR_BAD_ARG'], _lib.CONST['PDAE_ERR_UNSUPPORTED'], _lib.CONST['PDAE_OK']
    nan = float('nan')

    def attention(B=2, T=64, H=6, D=32, radius=0.5):
        return lib.pdae_attention_local_forward(B, T, H, D, 0.125, radius, None, None, None, None, None)

    def pack(B=2, G=72, Tp=40, C=96):
        return lib.pdae_m2ae_pack(B, G, Tp, C, None, None, None, None, None, None, None)

    def unpack(B=2, G=72, Tp=40, C=96):
        return lib.pdae_m2ae_unpack(B, G, Tp, C, None, None, None, None, None)

    def group_max(P=5, n=8, C=96):
        return lib.pdae_m2ae_group_max(P, n, C, None, None, None)

    def gather_max(P=5, k=8, C=96):
        return lib.pdae_m2ae_gather_max(P, k, C, None, None, None, None)

    def gather_add_relu(P=5, k=8, C=96):
        return lib.pdae_m2ae_gather_add_relu(P, k, C, None, None, None, None, None)

    def embed_tail(R_=48, n=16, K=256, N3=512, N4=96):
        return lib.pdae_m2ae_embed_tail(R_, n, K, N3, N4, None, None, None, None, None, None, None)

    def compact(B=2, G=72):
        return lib.pdae_m2ae_compact(B, G, None, None, None, None)

    table = [
        (attention, 'attention_local', [(dict(D=48), UNSUPPORTED), (dict(T=513), UNSUPPORTED), (dict(T=0), BAD),
                                        (dict(radius=-1.0), BAD), (dict(radius=nan), BAD)], dict(B=0)),
        (pack, 'm2ae_pack', [(dict(Tp=73), BAD), (dict(C=6), BAD), (dict(Tp=0), BAD),
                             (dict(B=1 << 20, G=1 << 20, Tp=1 << 20, C=4), UNSUPPORTED)], dict(B=0)),
        (unpack, 'm2ae_unpack', [(dict(Tp=73), BAD), (dict(C=6), BAD), (dict(Tp=0), BAD),
                                 (dict(B=1 << 20, G=1 << 20, Tp=1 << 20, C=4), UNSUPPORTED)], dict(B=0)),
        (group_max, 'm2ae_group_max', [(dict(C=6), BAD), (dict(n=0), BAD)], dict(P=0)),
        (gather_max, 'm2ae_gather_max', [(dict(C=6), BAD), (dict(k=0), BAD)], dict(P=0)),
        (gather_add_relu, 'm2ae_gather_add_relu', [(dict(C=6), BAD), (dict(k=0), BAD)], dict(P=0)),
        (embed_tail, 'm2ae_embed_tail', [(dict(n=5, R_=50), BAD), (dict(R_=12, n=8), BAD), (dict(K=260), UNSUPPORTED),
                                         (dict(K=12), UNSUPPORTED), (dict(N3=192), UNSUPPORTED), (dict(N4=160), UNSUPPORTED),
                                         (dict(N4=48), UNSUPPORTED)], dict(R_=0)),
        (compact, 'm2ae_compact', [(dict(G=0), BAD)], dict(B=0)),
    ]
    for entry, name, refused, empty in table:
        # the defaults are a shape the entry takes: with them only the pointers are wrong
        assert entry() == BAD and lib.pdae_last_error() == (name + ': null pointer').encode()
        for kwargs, status in refused:
            assert entry(**kwargs) == status, (name, kwargs)
            msg = lib.pdae_last_error()
            assert name.encode() in msg and b'null pointer' not in msg, (name, kwargs, msg)
            if 'B' in kwargs and kwargs['B'] == 1 << 20:
                assert msg == (name + ': too many elements').encode()
        assert entry(**empty) == OK, (name, empty)                 # nothing to do: OK with null pointers
