"""What hipcc makes of csrc/block.hip (compile only, no GPU; skipped without hipcc): no kernel reads through flat loads or
owns a private segment -- the signs of `cond ? *ptr : zero` compiled as a select between an address and a stack slot --
and the LayerNorm instantiations of the flagship step make one trip to memory per row.

The three *_legacy_kernel forms are what PDAE_LN=0 launches: they are kept as they were (flat loads and stack slot
included) as the A/B reference until the switch is retired, and are the only kernels left out of the first check."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import asm_skeleton  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(asm_skeleton.HIPCC) or shutil.which(asm_skeleton.HIPCC)),
                                reason='hipcc is not installed')

LEGACY = ('add_layernorm_fwd_legacy_kernel', 'layernorm_bwd_legacy_kernel', 'tail_rows_scatter_legacy_kernel')


@pytest.fixture(scope='module')
def kernels():
    found = asm_skeleton.kernels(asm_skeleton.device_asm(os.path.join(ROOT, 'point_dae_amd', 'csrc', 'block.hip')))
    assert len(found) > 40
    return found


def _is_legacy(name):
    return any(re.search(r'\bpdae::%s\b' % k, name) for k in LEGACY)


def test_no_kernel_uses_flat_loads_or_a_private_segment(kernels):
    legacy = [n for n in kernels if _is_legacy(n)]
    assert len(legacy) == 4, legacy          # forward, backward <2,16> and <8,4>, tail scatter: nothing else hides here
    for name, k in kernels.items():
        if _is_legacy(name):
            continue
        flat = [ln for ln in k['body'] if ln.startswith(('flat_load', 'scratch_'))]
        assert not flat, (name, flat[:4])
        assert k['private'] == 0, (name, k['private'])
    for name in ('pdae::tail_rows_scatter_kernel(', 'pdae::layernorm_bwd_kernel<2, 16, 3, 1, true>(',
                 'pdae::add_layernorm_fwd_kernel<2, 3, true, false>('):
        assert any(name in n for n in kernels), name


def _step_instantiations(kernels):
    """(name, kernel, 16-byte loads of the first row): two column slots (C <= 512) and every compile-time slab count the
    dispatch sends there -- a superset of what pdae_rows_gemm_plan gives for K = 384 / 1152 / 1536 at M = 2944 and 8192
    (1 and 3 slabs on a 256-CU part), so the test does not depend on the plan of the machine it runs on."""
    out = []
    for name, k in kernels.items():
        m = re.search(r'pdae::add_layernorm_fwd_kernel<2, (\d), (true|false), (true|false)>', name)
        if m:
            slabs, bias, pos = int(m.group(1)), m.group(2) == 'true', m.group(3) == 'true'
            out.append((name, k, 2 * (1 + slabs + bias + pos + 2)))                # x, slabs, bias, pos, gamma, beta
        m = re.search(r'pdae::layernorm_bwd_kernel<2, 16, (\d), ([12]), (true|false)>', name)
        if m:
            slabs, dres = int(m.group(1)), m.group(3) == 'true'
            out.append((name, k, 2 + 2 * (slabs + 1 + dres)))                      # gamma; dy slabs, x, dres
    assert len(out) == (2 + 4 * 4) + 2 * (4 + 3), len(out)
    return out


def test_step_layernorms_issue_a_rows_loads_before_the_first_wait(kernels):
    for name, k, first_row in _step_instantiations(kernels):
        body = k['body']
        wait = next(i for i, ln in enumerate(body) if ln.startswith('s_waitcnt') and 'vmcnt' in ln)
        early = sum(ln.startswith('global_load_dwordx4') for ln in body[:wait])
        assert early >= first_row, (name, early, first_row)
        if 'add_layernorm_fwd' in name or re.search(r'16, \d, 1, ', name):     # one row per wave: there are no other loads
            assert early == sum(ln.startswith('global_load_dwordx4') for ln in body), name


def test_step_layernorms_have_no_one_load_loop_behind_a_full_wait(kernels):
    """the shape of `for (q = 1; q < slabs; ++q) t += slab[q]` with a runtime trip count: a loop whose every trip is one
    load and s_waitcnt vmcnt(0)"""
    for name, k, _ in _step_instantiations(kernels):
        body = k['body']
        for first, last in asm_skeleton.loops(body):
            span = body[first:last + 1]
            loads = sum(ln.startswith(('global_load', 'flat_load', 'buffer_load')) for ln in span)
            full = any(ln.startswith('s_waitcnt') and 'vmcnt(0)' in ln for ln in span)
            assert not (loads == 1 and full), (name, span[:12])
