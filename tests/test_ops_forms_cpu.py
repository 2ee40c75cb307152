"""CPU side of tests/test_gpu_ops_forms.py: what that module takes for granted, checked without a GPU.

* the `n <= K` ladders and the size limits it restates are read out of the kernels' SOURCE TEXT and compared with its
  tables, and every threshold has a case on both sides: retuning a ladder fails here, loudly, instead of moving a GPU
  case off its edge;
* its integer-valued gradient inputs make the oracle's fp32 scatter-adds equal to an int64 scatter, exactly: the
  condition under which the GPU tests may demand equality from sums whose order is unspecified.
"""
import os
import re

import numpy as np
import pytest

import test_gpu_ops_forms as forms

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'point_dae_amd', 'csrc')


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _entry(text, name):
    """The body of one extern "C" entry (up to the next one)."""
    start = text.index('extern "C" int ' + name + '(')
    end = text.find('extern "C"', start + 1)
    return text[start:end if end >= 0 else len(text)]


def test_fps_ladder_in_the_source_is_the_tested_one():
    body = _entry(_source('fps.hip'), 'pdae_furthest_point_sampling')
    ladder = [(int(k), (int(t), int(p))) for k, t, p in re.findall(r'n <= (\d+)\) launch_fps<(\d+), (\d+)>', body)]
    assert ladder == forms.FPS_LADDER
    (above,) = re.findall(r'\n\s*else launch_fps<(\d+), (\d+)>', body)
    assert tuple(map(int, above)) == forms.FPS_ABOVE
    assert len(re.findall(r'launch_fps<', body)) == len(ladder) + 1          # no rung the pattern missed
    assert re.findall(r'n > (\d+)\) return unsupported', body) == [str(forms.FPS_MAX_N)]
    assert 'lds_bytes <= 96 * 1024' in _source('fps.hip') and forms.FPS_LDS_BYTES == 96 * 1024
    # every rung has a case on it and one past it, and every case names the form the ladder gives
    for k, _ in ladder:
        assert k in forms.FPS_NS and k + 1 in forms.FPS_NS
    assert forms.FPS_MAX_N in forms.FPS_NS and 8192 in forms.FPS_NS and 8193 in forms.FPS_NS
    assert {n: forms.fps_form(n) for n in forms.FPS_NS} == forms.FPS_FORMS
    for n in forms.FPS_NS:
        t, p = forms.fps_form(n)
        assert t * p >= n


def test_knn_ladder_in_the_source_is_the_tested_one():
    body = _entry(_source('knn.hip'), 'pdae_knn')
    ladder = [(int(k), int(p)) for k, p in re.findall(r'n <= (\d+)\) PDAE_KNN_LAUNCH\((\d+)\)', body)]
    assert ladder == forms.KNN_LADDER
    assert len(re.findall(r'PDAE_KNN_LAUNCH\(\d+\)', body)) == len(ladder) and body.count('knn_stream_kernel') == 1
    assert re.findall(r'k > (\d+)\) return unsupported', body) == [str(forms.KNN_MAX_K)]
    assert re.findall(r'qpw\) < (\d+)\) qpw >>= 1', body) == [str(forms.KNN_QPW_WAVES)] and 'int qpw = 8;' in body
    assert re.findall(r'b > (\d+)\) return unsupported', body) == [str(forms.MAX_GRID_Y)]
    for k, ppl in ladder:
        assert k in forms.KNN_NS and k + 1 in forms.KNN_NS and 64 * ppl >= k
    assert {n: forms.knn_form(n) for n in forms.KNN_NS} == forms.KNN_FORMS


def test_limits_in_the_sources_are_the_tested_ones():
    ball = _source('ball_group.hip')
    body = _entry(ball, 'pdae_ball_query')
    assert 'lds > 150 * 1024' in body and 'n > 12800 not implemented' in body and forms.BALL_LDS_BYTES == 12800 * 12
    assert re.findall(r'cpw\) < (\d+)\) cpw >>= 1', body) == [str(forms.BALL_CPW_WAVES)] and 'int cpw = 8;' in body
    assert '<= 128 * 1024' in _entry(ball, 'pdae_group_points_grad') and forms.GROUP_GRAD_LDS_BYTES == 32768 * 4
    body = _entry(ball, 'pdae_sa_group_rows_grad')
    assert 'C > 1024' in body and 'N > 4096 || lds > 150 * 1024' in body
    assert 'sizeof(int) * ((size_t)2 * N + 1 + (size_t)rows)' in body
    interp = _source('interpolate.hip')
    assert 'constexpr int TNN_TILE = 1024;' in interp and forms.TNN_TILE == 1024
    assert 'sizeof(float) > 160 * 1024' in _entry(interp, 'pdae_three_interpolate_grad')
    assert forms.INTERP_GRAD_LDS_BYTES == 40960 * 4


def test_host_formulas_give_the_forms_the_cases_name(oracle_ops):
    assert [forms.knn_qpw(b, g) for b, g in ((64, 250), (16, 509), (8, 513), (2, 7))] == [8, 4, 2, 1]
    assert [forms.ball_cpw(b, m) for b, m in ((64, 515), (32, 509), (16, 513), (2, 9))] == [8, 4, 2, 1]
    assert [forms.group_grad_form(n) for n in forms.GROUP_NS] == ['lds', 'atomic']
    for n in forms.FPS_NS + [1, 2, 3, 100, 1500]:
        assert forms.ref_block_size(n) == oracle_ops.opt_n_threads(n)


@pytest.mark.parametrize('variant', ['far_last', 'skip_last'])
@pytest.mark.parametrize('n', [64, 65, 513, 4097, 32768])
def test_fps_built_cloud_is_decided_by_the_tie_rank(oracle_ops, n, variant):
    """The cloud the GPU cases use: its second sample is the planted farthest point, its third the plateau point the
    reference's block layout prefers -- not the lowest index, not the lowest thread."""
    p, far, plateau = forms.fps_built_cloud(n, variant, 7)
    idx = oracle_ops.furthest_point_sample(p[None], 12)[0]
    bs = forms.ref_block_size(n)
    winner = min(plateau, key=lambda k: forms.fps_tie_rank(k, bs))
    assert idx[0] == 0 and idx[1] == far and idx[2] == winner
    assert winner != min(plateau) and winner % bs != min(k % bs for k in plateau)
    if -(-n // bs) > 2:
        assert len({k // bs for k in plateau}) >= 2        # the plateau spans columns of the block layout
    assert len(set(idx)) == 12
    if variant == 'skip_last':
        assert far < n - 1 and not (idx > far).any()
        assert (((p[far + 1:] ** 2).sum(1)) <= 1e-3).all()
    else:
        assert far == n - 1


@pytest.mark.parametrize('kind', forms.GROUP_INDEX_KINDS)
@pytest.mark.parametrize('npnt,ns', forms.GROUP_SHAPES)
@pytest.mark.parametrize('n', forms.GROUP_NS)
def test_integer_gradients_make_group_scatter_exact(oracle_ops, n, npnt, ns, kind):
    f, idx, go = forms.group_inputs(n, npnt, ns, kind, 5000 + n + ns)
    assert idx.min() >= 0 and idx.max() < n and np.abs(go).max() <= 4 and np.array_equal(go, np.round(go))
    want = forms.scatter_int64(go.reshape(2, 3, -1), idx.reshape(2, -1), n)
    assert np.abs(want).max() < 2 ** 24
    got = oracle_ops.grouping_operation_grad(go, idx, n)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    if kind != 'random':
        assert np.abs(want).max() > 4                     # sums really accumulate: many gradients per slot
    # the same inputs through gather (nsample = 1)
    f, idx, go = forms.group_inputs(n, npnt, 1, kind, 5100 + n + npnt)
    idx, go = idx[:, :, 0].copy(), go[:, :, :, 0].copy()
    np.testing.assert_array_equal(oracle_ops.gather_operation_grad(go, idx, n), forms.scatter_int64(go, idx, n))


@pytest.mark.parametrize('kind', ['random', 'one_point'])
@pytest.mark.parametrize('m', forms.INTERP_MS)
def test_integer_gradients_make_interpolate_scatter_exact(oracle_ops, m, kind):
    pts, idx, w, g = forms.interp_inputs(m, kind, 6100 + m)
    assert idx.min() >= 0 and idx.max() < m
    assert (np.sort(w, axis=2) == np.float32([0.25, 0.25, 0.5])).all()
    assert len({tuple(r) for r in w.reshape(-1, 3)}) == 3               # all three placements of the 1/2 occur
    want = forms.interp_grad_int64(g, idx, w, m)
    got = oracle_ops.three_interpolate_grad(g, idx, w, m)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
