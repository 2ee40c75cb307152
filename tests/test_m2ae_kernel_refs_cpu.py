"""The references of tests/test_gpu_m2ae_kernels.py on a machine without a GPU: what that file holds the kernels of
csrc/m2ae.hip to is itself held to tests/m2ae_restatement.py here (which tests/test_m2ae_cpu.py holds to the live
reference's fp64 features), and the conditions its attention cases rest on are asserted for their seeds."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import m2ae_restatement as R  # noqa: E402
import weights  # noqa: E402
from test_gpu_m2ae import _rel  # noqa: E402
from test_gpu_m2ae_kernels import (ATTENTION_CASES, COMPACT_G, MARGIN, STD2, attention_inputs, compact_rows, ref_attention,
                                   ref_attention_margin, ref_compact, ref_embed_tail, ref_gather_add_relu, ref_gather_max,
                                   ref_group_max, ref_pack, ref_unpack)  # noqa: E402
from test_m2ae_cpu import build_model  # noqa: E402

NUM_GROUPS, GROUP_SIZES = [72, 40, 8], [16, 8, 4]
_cache = {}


def small_model64():
    if not _cache:
        model = weights.fill_state(build_model(NUM_GROUPS, GROUP_SIZES), 7).double().eval()
        _cache['model'] = model
        _cache['sd'] = dict(model.state_dict())
    return _cache['model'], _cache['sd']


def test_embed_tail_formula_composed_as_the_level0_embedder_composes_it():
    from point_dae_amd.point_m2ae import _folded
    model, sd = small_model64()
    te = model.h_encoder.token_embed[0]
    gen = torch.Generator().manual_seed(3)
    P, n = 3 * 72, 16
    patches = (0.15 * torch.randn(P, n, 3, generator=gen)).double()
    with torch.no_grad():
        w1, b1 = _folded(te.first_conv[0], te.first_conv[1])
        y = torch.relu(patches.reshape(P * n, 3) @ w1.t() + b1)
        f = y @ te.first_conv[3].weight.squeeze(-1).t() + te.first_conv[3].bias
        c2 = f.shape[1]
        g = ref_group_max(f, P, n)
        w3, b3 = _folded(te.second_conv[0], te.second_conv[1])
        gb = g @ w3[:, :c2].t() + b3                               # the global half enters as the per-patch term
        got = ref_embed_tail(f, n, w3[:, c2:], gb, te.second_conv[3].weight.squeeze(-1), te.second_conv[3].bias)
    want = R.token_embed(sd, 'h_encoder.token_embed.0', patches)
    assert got.dtype == torch.float64 and got.shape == want.shape == (P, 96)
    assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize('level,S,P,k', [(1, 72, 40, 8), (2, 40, 8, 4)])
def test_split_form_of_the_merging_embedder(level, S, P, k):
    from point_dae_amd.point_m2ae import _folded
    model, sd = small_model64()
    te = model.h_encoder.token_embed[level]
    gen = torch.Generator().manual_seed(10 + level)
    B = 3
    table = torch.randn(B * S, te.in_c, generator=gen).double()
    local = torch.randint(0, S - S // 4, (B, P * k), generator=gen)
    local[:, :3] = local[:, 3:6]
    idx = (local + torch.arange(B).unsqueeze(1) * S).reshape(-1)
    with torch.no_grad():
        w1, b1 = _folded(te.first_conv[0], te.first_conv[1])
        f = torch.relu(table @ w1.t() + b1) @ te.first_conv[3].weight.squeeze(-1).t() + te.first_conv[3].bias
        c_in = f.shape[1]
        w3, b3 = _folded(te.second_conv[0], te.second_conv[1])
        u = f @ w3[:, c_in:].t()                                   # per source row: the local half
        gb = ref_gather_max(f, idx, B * P, k) @ w3[:, :c_in].t() + b3
        h = ref_gather_add_relu(u, idx, gb, k)
        t = h @ te.second_conv[3].weight.squeeze(-1).t() + te.second_conv[3].bias
        got = ref_group_max(t, B * P, k)
    want = R.token_embed(sd, 'h_encoder.token_embed.%d' % level, table[idx].reshape(B * P, k, -1))
    assert got.shape == want.shape == (B * P, te.out_c) and _rel(got, want) <= 1e-12


def _pyramid(B, seed):
    """a seeded pyramid in the layout of point_m2ae_group.HierarchicalGroup: patches of level 0, centres per level, and
    per level i > 0 the flat rows of level i - 1 its patches merge (never the top quarter of a sample: masked tokens)"""
    gen = torch.Generator().manual_seed(seed)
    nb = [(0.15 * torch.randn(B, NUM_GROUPS[0], GROUP_SIZES[0], 3, generator=gen)).double()]
    centers = [(0.4 * torch.randn(B, G, 3, generator=gen)).double() for G in NUM_GROUPS]
    idxs = [None]
    for i in range(1, len(NUM_GROUPS)):
        Gc = NUM_GROUPS[i - 1]
        local = torch.randint(0, Gc - Gc // 4, (B, NUM_GROUPS[i] * GROUP_SIZES[i]), generator=gen)
        idxs.append((local + torch.arange(B).unsqueeze(1) * Gc).reshape(-1))
    return nb, centers, idxs


def _forward_on_the_refs(nb, centers, idxs, sd, num_heads=6, local_radius=(0.32, 0.64, 1.28)):
    """R.forward with its masked indexing replaced by ref_compact / ref_pack / ref_unpack"""
    pre = 'h_encoder.'
    B = centers[0].shape[0]
    masks = R.visibility(centers, idxs)
    levels, table = [], None
    for i in range(len(centers)):
        G = centers[i].shape[1]
        if i == 0:
            tokens = R.token_embed(sd, pre + 'token_embed.0', nb[0].reshape(B * G, -1, 3))
        else:
            k = idxs[i].numel() // (B * G)
            tokens = R.token_embed(sd, pre + 'token_embed.%d' % i, table[idxs[i]].reshape(B * G, k, -1))
        C = tokens.shape[1]
        lens, ids = ref_compact(masks[i])
        Tp = int(lens.max())
        x, cen = ref_pack(tokens, centers[i].reshape(B * G, 3), ids, lens, B, G, Tp)
        x, cen = x.reshape(B, Tp, C), cen.reshape(B, Tp, 3)
        mask = R.attention_mask(cen, lens.long(), local_radius[i])
        pos = R._linear(sd, pre + 'encoder_pos_embeds.%d.2' % i, F.gelu(R._linear(sd, pre + 'encoder_pos_embeds.%d.0' % i, cen)))
        j = 0
        while pre + 'encoder_blocks.%d.blocks.%d.norm1.weight' % (i, j) in sd:
            x = R.block(sd, pre + 'encoder_blocks.%d.blocks.%d' % (i, j), x + pos, mask, num_heads)
            j += 1
        valid = torch.arange(Tp).unsqueeze(0) < lens.unsqueeze(1)
        levels.append(dict(lens=lens, T_pad=Tp, rows=x[valid], masked=masks[i]))
        if i < len(centers) - 1:
            behind = x.clone()
            behind[~valid] = float('nan')                          # rows behind len[b] must never arrive in the table
            table = ref_unpack(tokens, behind.reshape(B * Tp, C), ids, lens, B, G, Tp)
            assert not bool(torch.isnan(table).any())
    x = R._ln(sd, pre + 'encoder_norms.%d' % (len(centers) - 1), x)
    return dict(feature=x.mean(1) + x.max(1)[0], levels=levels)


def test_compact_pack_unpack_expectations_are_what_the_restatement_does():
    _, sd = small_model64()
    nb, centers, idxs = _pyramid(3, 5)
    with torch.no_grad():
        want = R.forward(nb, centers, idxs, sd)
        got = _forward_on_the_refs(nb, centers, idxs, sd)
    partly = 0
    for g, w in zip(got['levels'], want['levels']):
        assert g['T_pad'] == w['T_pad'] and g['lens'].tolist() == w['lens'].tolist()
        assert g['rows'].shape == w['rows'].shape and _rel(g['rows'], w['rows']) <= 1e-12
        partly += int(0 < int(g['lens'].min()) < g['T_pad'] < g['masked'].shape[1])
    assert partly >= 2                                             # two levels drop tokens, and unevenly over the batch
    assert _rel(got['feature'], want['feature']) <= 1e-12


@pytest.mark.parametrize('G', COMPACT_G)
def test_compact_reference_on_its_own_rows(G):
    rows = compact_rows(G)
    masked = torch.stack(list(rows.values()))
    lens, ids = ref_compact(masked)
    assert lens.tolist() == (~masked).sum(1).tolist()
    for b in range(masked.shape[0]):
        n = int(lens[b])
        assert ids[b, :n].tolist() == torch.nonzero(~masked[b]).flatten().tolist() and bool((ids[b, n:] == -1).all())
    if G >= 65:
        assert ids[list(rows).index('63 and 64'), :3].tolist() == [63, 64, -1]
    if G >= 64:                                                    # the drawn rows are what their names say
        assert 0.1 * G < int(lens[-2]) < 0.3 * G and 0.7 * G < int(lens[-1]) < 0.9 * G


@pytest.mark.parametrize('case', ATTENTION_CASES, ids=lambda c: str(c[:6]))
def test_no_mask_decision_of_an_attention_case_hangs_on_rounding(case):
    B, T, H, D, lens, radius, zeroed, qk, stated = case
    qkv, cen, lens_t, valid = attention_inputs(B, T, H, D, lens, radius, zeroed, qk)
    assert qkv.shape == (B, T, 3, H, D) and cen.dtype == torch.float32
    assert bool((cen[~valid] == 0).all()) == (zeroed or bool(valid.all()))
    if radius > 0:
        margin, pairs = ref_attention_margin(cen, valid, radius)
        print('attention case %s: margin %.2e over %d pairs' % (case[:6], margin, pairs))
        assert margin >= MARGIN
        # the figure recorded with the case: with zeroed padded centres a decided pair's distance is a centre's norm
        plain = float((cen.double().norm(dim=-1) - radius).abs().min()) if zeroed else margin
        assert abs(plain / stated - 1.0) < 0.05 and margin >= plain
        mask = R.attention_mask(cen.double(), lens_t.long(), radius)
        decided = ~(valid.unsqueeze(2) & valid.unsqueeze(1))
        assert int(mask[decided].sum()) < pairs                    # the radius masks some of the pairs it decides, not all
        assert int(mask[decided].sum()) > 0 or min(lens) == 0      # (a sample without a visible token has every centre at 0)
        if not zeroed:
            assert pairs == 2900 and float(cen[~valid].norm(dim=-1).min()) > 0.1
    want = ref_attention(qkv, cen, lens_t, radius)
    assert want.shape == (B, T, H * D) and bool(torch.isfinite(want).all())
    # the fp32 evaluation of the same definition (the peaked case's yardstick, here on the host) sits at fp32 rounding
    # level of it: the -100000 of the mask costs nothing where it matters
    # (radius 0 leaves a padded query no key: -100000 + s in fp32 rounds s to 2^-7, and the kernel writes zeros there)
    keep = valid if radius == 0 else torch.ones_like(valid)
    assert _rel(ref_attention(qkv, cen, lens_t, radius, torch.float32)[keep], want[keep]) < (1e-5 if qk != STD2 else 2e-6)
