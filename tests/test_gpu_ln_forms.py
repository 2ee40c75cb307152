"""The one-trip LayerNorm kernels and the guarded tail_rows_scatter (csrc/block.hip, the default) against the forms they
replace (PDAE_LN=0): every output bit for bit, plus the identities both forms must satisfy exactly.

The switch is read once per process, so each form runs in a fresh child process: this file run as a script with
--worker OUT computes every case once under the PDAE_LN of its environment and writes, per case, a 64-bit digest of
every output's bit pattern (sum of odd weight x int32 pattern, mod 2^64: any single changed bit changes it) and the
results of the exact checks.  The tests below compare the two children's files; nothing is skipped or left out."""
import itertools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CS = (4, 128, 384, 512, 516, 2048)
MS = (1, 5, 37, 130)
BIG_MS = (6143, 6144, 6150)          # backward, C = 384: both sides of the two-rows-per-wave threshold, ragged last block
SLABS = (1, 2, 3, 4, 5, 8)
TS = (1, 13, 64)
EPS = 1e-5
ATOMIC_TOL = 2e-5                    # tests/test_gpu_block.py's bound for the parameter gradients against fp64

REFUSALS = {
    'fwd_c': 'layernorm forward: C must be a multiple of 4, at most 2048; T > 0; 1..8 slabs',
    'fwd_slabs': 'layernorm forward: C must be a multiple of 4, at most 2048; T > 0; 1..8 slabs',
    'fwd_null': 'layernorm forward: null pointer',
    'fwd_res_null': 'residual_layernorm_forward: null pointer',
    'bwd_dacc': 'layernorm backward: bad dacc',
    'bwd_c': 'layernorm backward: C must be a multiple of 4, at most 2048; T > 0; 1..8 slabs',
    'bwd_null': 'layernorm backward: null pointer',
    'bwd_res_null': 'residual_layernorm_backward: null pointer',
    'tail_shape': 'tail_rows: B >= 0, 0 < tail <= T, C a positive multiple of 4',
    'tail_null': 'tail_rows_scatter: null pointer',
}


def _rows(M, T):
    """M = B * T rows for a keep of B samples: the grid's M rounded up to whole samples."""
    return -(-M // T) * T


def forward_cases():
    for C, M in itertools.product(CS, MS):
        for pos in (0, 1):
            yield ('add', C, M, 1, 1, 0, 0, pos)
        for S, bias, keep, pos in itertools.product(SLABS, (0, 1), (0, 1), (0, 1)):
            for T in (TS if keep else (1,)):
                yield ('res', C, _rows(M, T), T, S, bias, keep, pos)


# backward variants: 0 = layernorm_backward; residual_layernorm_backward with 1 = dbias, 2 = dbias + da, 3 = dbias + da + keep
def backward_cases():
    grid = list(itertools.product(CS, MS)) + [(384, M) for M in BIG_MS]
    n = 0
    for (C, M), S, dres, var, mode in itertools.product(grid, SLABS, (0, 1), (0, 1, 2, 3), (0, 1, 2)):
        T = TS[n % 3] if var == 3 else 1
        n += var == 3
        yield (C, _rows(M, T) if M not in BIG_MS else M, 1 if M in BIG_MS else T, S, dres, var, mode)


def ordered_cases():
    """deterministic mode and parked reductions: the parameter gradients; dres alternates, dacc_mode 0"""
    grid = list(itertools.product(CS, MS)) + [(384, M) for M in BIG_MS]
    for n, ((C, M), S, var) in enumerate(itertools.product(grid, SLABS, (0, 1, 2, 3))):
        T = TS[n % 3] if var == 3 and M not in BIG_MS else 1
        yield (C, _rows(M, T), T, S, n & 1, var, 0)


def tail_cases():
    return list(itertools.product((1, 3), (1, 41, 64), (4, 384), (0, 1)))      # B, tail, C, with db; T = 64


def _key(*parts):
    return '-'.join(str(p) for p in parts)


# ---- the worker ----------------------------------------------------------------------------------------------------------

def _worker(out_path):
    sys.path.insert(0, ROOT)
    import random
    import numpy as np
    import torch
    from point_dae_amd import _lib
    from point_dae_amd.graph_step import use_created_stream
    use_created_stream()
    dev = 'cuda'
    torch.manual_seed(1234)
    pool = torch.randn(11 * 6150 * 384 + 4096, device=dev)

    def odd_weights(n):
        return (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 + 12345) | 1

    weights = odd_weights(6150 * 384)
    P = _lib.ptr
    res = {'form': os.environ.get('PDAE_LN', ''), 'digest': {}, 'failed': [], 'atomic_err': 0.0, 'refusal': {}}
    pending = []                    # (key, device scalar): one transfer at the end

    def take(n, at):
        return pool[at:at + n]

    def digest(key, *tensors):
        for i, t in enumerate(tensors):
            v = t.contiguous().view(-1).view(torch.int32).to(torch.int64)
            w = weights[:v.numel()] if v.numel() <= weights.numel() else odd_weights(v.numel())
            pending.append((key + ':' + str(i), (v * w).sum()))

    def check(key, what, ok):
        if not bool(ok):
            res['failed'].append(key + ' ' + what)

    # -- forward
    for idx, case in enumerate(forward_cases()):
        entry, C, M, T, S, bias, keep, pos = case
        key = _key('fwd', idx, *case)
        n = M * C
        x = take(n, 0).view(M, C)
        br = take(S * n, n).view(S, M, C)
        p = take(n, 9 * 6150 * 384).view(M, C) if pos else None
        g, be, b = take(C, 7), take(C, 3001), (take(C, 5003) if bias else None)
        k = ((take(M // T, 6007) > -0.8).float() / 0.9) if keep else None
        xsum, y = torch.full((M, C), float('nan'), device=dev), torch.empty(M, C, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        if entry == 'add':
            _lib.call('pdae_add_layernorm_forward', x, M, C, P(x), P(p), P(g), P(be), EPS, P(xsum) if pos else None, P(y),
                      P(mean), P(rstd))
            want = x + p if pos else None
        else:
            _lib.call('pdae_residual_layernorm_forward', x, M, C, T, P(br), S, P(b), P(k), P(x), P(p), P(g), P(be), EPS,
                      P(xsum), P(y), P(mean), P(rstd))
            t = br[0]
            for q in range(1, S):
                t = t + br[q]
            if bias:
                t = t + b
            if keep:
                t = t * k.repeat_interleave(T)[:, None]
            want = x + t
            if pos:
                want = want + p
        if want is not None:
            check(key, 'xsum differs from the fp32 restatement', torch.equal(xsum, want))
            digest(key, xsum, y, mean, rstd)
        else:
            check(key, 'xsum written although s = x', bool(torch.isnan(xsum).all()))
            digest(key, y, mean, rstd)

    # -- backward
    def backward(case, zero_first):
        C, M, T, S, dres, var, mode = case
        n = M * C
        dy = take(S * n, 0).view(S, M, C)
        x = take(n, 8 * 6150 * 384).view(M, C)
        dr = take(n, 9 * 6150 * 384).view(M, C) if dres else None
        g = take(C, 11)
        mean, rstd = take(M, 4001) * 0.1, 1.0 + 0.1 * take(M, 9001).abs()
        k = ((take(M // T, 6007) > -0.8).float() / 0.9) if var == 3 else None
        dx = torch.empty(M, C, device=dev)
        da = torch.empty(M, C, device=dev) if var >= 2 else None
        old = take(n, 10 * 6150 * 384).view(M, C).clone() if mode else None
        dacc = old.clone() if mode else None
        par = torch.full((3, C), float('nan'), device=dev)
        acc = 0 if zero_first else 1
        if not zero_first:
            par.zero_()
        if var == 0:
            _lib.call('pdae_layernorm_backward', x, M, C, P(dy), S, P(x), P(mean), P(rstd), P(g), P(dr), P(dx), P(par[0]),
                      P(par[1]), acc, P(dacc), mode)
        else:
            _lib.call('pdae_residual_layernorm_backward', x, M, C, T, P(dy), S, P(x), P(mean), P(rstd), P(g), P(dr), P(k), P(dx),
                      P(da), P(par[0]), P(par[1]), P(par[2]), acc, P(dacc), mode)
        return dy, x, mean, rstd, k, dx, da, old, dacc, par

    for idx, case in enumerate(backward_cases()):
        C, M, T, S, dres, var, mode = case
        key = _key('bwd', idx, *case)
        dy, x, mean, rstd, k, dx, da, old, dacc, par = backward(case, zero_first=False)
        digest(key, dx, *([da] if da is not None else []), *([dacc] if mode else []))
        if var == 3:
            check(key, 'da != keep * dx', torch.equal(da, dx * k.repeat_interleave(T)[:, None]))
        elif var == 2:
            check(key, 'da != dx', torch.equal(da, dx))
        if mode == 1:
            check(key, 'dacc != dx', torch.equal(dacc, dx))
        elif mode == 2:
            check(key, 'dacc != old + dx', torch.equal(dacc, old + dx))
        # the parameter gradients (atomics: order of arrival) against fp64
        d64 = dy.double().sum(0)
        xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
        want = [(d64 * xh).sum(0), d64.sum(0)] + ([(da if da is not None else dx).double().sum(0)] if var else [])
        for i, w in enumerate(want):
            err = float((par[i].double() - w).abs().max() / (w.abs().max() + 1e-12))
            res['atomic_err'] = max(res['atomic_err'], err)
            check(key, 'parameter gradient %d off fp64 by %.3g' % (i, err), err <= ATOMIC_TOL)

    # -- the parameter gradients where their bits are defined: deterministic mode, parked reductions
    _lib.set_deterministic(True)
    try:
        for idx, case in enumerate(ordered_cases()):
            out = backward(case, zero_first=True)
            digest(_key('det', idx, *case), out[9][:3 if case[5] else 2])
    finally:
        _lib.set_deterministic(False)
    for idx, case in enumerate(ordered_cases()):
        _lib.deferred_begin()
        out = backward(case, zero_first=True)
        _lib.deferred_flush(out[5])
        digest(_key('parked', idx, *case), out[9][:3 if case[5] else 2])

    # -- tail_rows_scatter
    T = 64
    for B, tail, C, with_db in tail_cases():
        key = _key('tail', B, tail, C, with_db)
        a_t, b_t = take(B * tail * C, 17).view(B, tail, C), take(B * tail * C, 100003).view(B, tail, C)
        da = torch.full((B, T, C), float('nan'), device=dev)
        db = torch.full((B, T, C), float('nan'), device=dev) if with_db else None
        _lib.call('pdae_tail_rows_scatter', a_t, B, T, tail, C, P(a_t), P(b_t) if with_db else None, P(da), P(db))
        for name, full, src in (('da', da, a_t), ('db', db, b_t)):
            if full is not None:
                check(key, name + ' tail rows', torch.equal(full[:, T - tail:], src))
                check(key, name + ' not zero outside the tail', bool((full[:, :T - tail] == 0).all()))
        digest(key, da, *([db] if with_db else []))

    # -- refusals
    t = torch.empty(64 * 8, device=dev)
    p = P(t)
    bad = {
        'fwd_c': ('pdae_add_layernorm_forward', (8, 6, p, None, p, p, EPS, None, p, p, p)),
        'fwd_slabs': ('pdae_residual_layernorm_forward', (8, 8, 1, p, 9, None, None, p, None, p, p, EPS, p, p, p, p)),
        'fwd_null': ('pdae_add_layernorm_forward', (8, 8, p, p, p, p, EPS, None, p, p, p)),
        'fwd_res_null': ('pdae_residual_layernorm_forward', (8, 8, 1, None, 1, None, None, p, None, p, p, EPS, p, p, p, p)),
        'bwd_dacc': ('pdae_layernorm_backward', (8, 8, p, 1, p, p, p, p, None, p, p, p, 1, None, 1)),
        'bwd_c': ('pdae_layernorm_backward', (8, 2052, p, 1, p, p, p, p, None, p, p, p, 1, None, 0)),
        'bwd_null': ('pdae_layernorm_backward', (8, 8, None, 1, p, p, p, p, None, p, p, p, 1, None, 0)),
        'bwd_res_null': ('pdae_residual_layernorm_backward', (8, 8, 1, p, 1, p, p, p, p, None, None, p, None, p, p, None, 1, None, 0)),
        'tail_shape': ('pdae_tail_rows_scatter', (1, 8, 9, 8, p, None, p, None)),
        'tail_null': ('pdae_tail_rows_scatter', (1, 8, 4, 8, None, None, p, None)),
    }
    for name, (entry, args) in bad.items():
        try:
            _lib.call(entry, t, *args)
            res['refusal'][name] = 'accepted'
        except RuntimeError as e:
            res['refusal'][name] = str(e)

    # -- one deterministic graphed optimisation step of the flagship model at a reduced size
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.graph_step import GraphedTrainStep
    from point_dae_amd.synthetic import shapenet_like_clouds
    config = cfg_from_yaml_file(os.path.join(
        ROOT, 'cfgs', 'pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml'))
    B, N = 4, 1024
    _lib.set_deterministic(True)
    try:
        torch.manual_seed(0)
        model = FlatDataParallel(builder.model_builder(config.model).cuda().train())
        opt, _ = builder.build_opti_sche(model, config)
        model.zero_grad()
        step = GraphedTrainStep(model, opt, config, B, N, warmup_eager=1)
        clouds = torch.from_numpy(shapenet_like_clouds(B, N, seed=4)).cuda()
        random.seed(7), np.random.seed(7), torch.manual_seed(7)
        losses = []
        for _ in range(3):
            lx, ln = step(clouds)
            losses.append(lx.clone()), losses.append(ln.clone().reshape(-1))
        torch.cuda.synchronize()
        res['step_graphs'] = len(step.graphs)
        digest('step', torch.cat([v.reshape(-1) for v in losses]), model.flat_param, model.flat_grad)
    finally:
        _lib.set_deterministic(False)

    torch.cuda.synchronize()
    values = torch.stack([v for _, v in pending]).cpu().tolist()
    res['digest'] = {k: v for (k, _), v in zip(pending, values)}
    with open(out_path, 'w') as f:
        json.dump(res, f)


# ---- the tests -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def forms(tmp_path_factory):
    """{'0': the legacy forms' results, '1': the new forms'}, each from its own child process."""
    out = {}
    for form in ('0', '1'):
        path = str(tmp_path_factory.mktemp('ln_forms') / ('form%s.json' % form))
        env = dict(os.environ, PDAE_LN=form)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', path], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        with open(path) as f:
            out[form] = json.load(f)
        assert out[form]['form'] == form
    assert out['0']['digest'].keys() == out['1']['digest'].keys()
    return out


def _differing(forms, prefix):
    old, new = forms['0']['digest'], forms['1']['digest']
    keys = [k for k in new if k.startswith(prefix + '-') or k.startswith(prefix + ':')]
    assert keys, prefix
    return len(keys), [k for k in keys if new[k] != old[k]]


def _failed(forms, prefix):
    return [m for form in ('0', '1') for m in forms[form]['failed'] if m.startswith(prefix + '-')]


def test_forward_xsum_is_the_fp32_restatement_exactly(forms):
    """xsum = x + keep * (slab 0 + slab 1 + ... + bias) + pos in that order, element-wise fp32: torch.equal; and xsum is
    left alone where s = x.  Every case of forward_cases() (both entries, every bias / keep / pos combination)."""
    assert len(list(forward_cases())) == 6 * 4 * (2 + 6 * (4 + 4 * 3))
    assert not _failed(forms, 'fwd'), _failed(forms, 'fwd')[:20]


def test_forward_outputs_equal_the_legacy_form_bit_for_bit(forms):
    """xsum, y, mean, rstd of every forward case"""
    n, bad = _differing(forms, 'fwd')
    assert n == 4 * len(list(forward_cases())) - 6 * 4          # (add_layernorm without pos leaves xsum alone)
    assert not bad, (len(bad), bad[:20])


def test_backward_outputs_equal_the_legacy_form_bit_for_bit(forms):
    """dx, da, dacc of every backward case"""
    n, bad = _differing(forms, 'bwd')
    assert n == sum(1 + (var >= 2) + (mode > 0) for _, _, _, _, _, var, mode in backward_cases())
    assert not bad, (len(bad), bad[:20])


def test_backward_identities_hold_exactly_and_atomic_sums_stay_within_bound(forms):
    """da == keep[row / T] * dx, mode 1: dacc == dx, mode 2: dacc == old + dx (torch.equal); dgamma / dbeta / dbias by
    atomics within 2e-5 max|.| of fp64 (the bound of tests/test_gpu_block.py) -- in both forms."""
    print('largest parameter-gradient error against fp64 / max|.|: legacy %.3g, new %.3g'
          % (forms['0']['atomic_err'], forms['1']['atomic_err']))
    assert len(list(backward_cases())) == 27 * 6 * 2 * 4 * 3
    assert not _failed(forms, 'bwd'), _failed(forms, 'bwd')[:20]
    assert forms['1']['atomic_err'] <= ATOMIC_TOL


@pytest.mark.parametrize('mode', ['det', 'parked'])
def test_parameter_gradients_equal_the_legacy_form_bit_for_bit(forms, mode):
    """dgamma, dbeta, dbias in deterministic mode and between pdae_deferred_begin / _flush"""
    n, bad = _differing(forms, mode)
    assert n == len(list(ordered_cases())) == 27 * 6 * 4
    assert not bad, (len(bad), bad[:20])


def test_tail_rows_scatter_equals_the_legacy_form_and_zeroes_the_rest(forms):
    n, bad = _differing(forms, 'tail')
    assert n == sum(1 + with_db for _, _, _, with_db in tail_cases())
    assert not bad, bad
    assert not _failed(forms, 'tail'), _failed(forms, 'tail')


def test_refusals_keep_status_and_message(forms):
    for form in ('0', '1'):
        for name, msg in REFUSALS.items():
            got = forms[form]['refusal'][name]
            assert got.endswith('failed with status -1: ' + msg), (form, name, got)


def test_a_deterministic_graphed_step_equals_the_legacy_form_bit_for_bit(forms):
    """B = 4, N = 1024, depth as the YAML, three updates (the first eager, then hipGraph replays): the losses, the
    parameters and the gradients"""
    assert forms['0']['step_graphs'] >= 1 and forms['1']['step_graphs'] >= 1
    n, bad = _differing(forms, 'step')
    assert n == 3
    assert not bad, bad


if __name__ == '__main__':
    assert sys.argv[1] == '--worker'
    _worker(sys.argv[2])
