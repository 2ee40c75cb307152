"""bench.py's launcher contract on the CPU side: `--gpus N` is binding."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, drop=('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'PDAE_BENCH_BACKEND')):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=300)


def test_gpus_n_without_devices_is_refused():
    """No launcher, --gpus 8, fewer than 8 visible GPUs: exit != 0 and no result line (the driver
    must never record a single-GPU number as an 8-GPU point)."""
    import torch
    if torch.cuda.device_count() >= 8:
        return
    r = _run(['--gpus', '8', '--steps', '1', '--warmup', '0'])
    assert r.returncode != 0
    assert '{"metric"' not in r.stdout
    assert 'refusing' in r.stderr


def test_world_size_mismatch_is_refused():
    r = _run(['--gpus', '4', '--steps', '1', '--warmup', '0'],
             {'RANK': '0', 'WORLD_SIZE': '2', 'LOCAL_RANK': '0'})
    assert r.returncode != 0 and 'does not match' in (r.stderr + r.stdout)
    assert '{"metric"' not in r.stdout


def test_ddp_model_expected_maximum_matches_a_monte_carlo_draw():
    """bench.py's `ddp_model` (the only scaling figure a one-GPU pool can give): E[max over n ranks of the replay time of
    each rank's own T_vis draw], computed from the exact distribution of T_vis, against a direct simulation -- the mask
    ratio drawn as MaskTransformer._mask_center_rand draws it (uniform in [0.5, 0.8), num_mask = int(ratio * G))."""
    import importlib.util
    import os
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    G = 64
    p = bench.tvis_distribution(G)
    assert abs(sum(p.values()) - 1.0) < 1e-12 and min(p) == G - int(0.8 * G) and max(p) == G - int(0.5 * G)
    rng = np.random.default_rng(0)
    table = {t: 9.0 + 0.18 * t + 0.3 * np.sin(t) for t in p}           # ms per replay, not monotone in T_vis
    ratio = rng.uniform(0.5, 0.8, size=(400000, 8))
    tvis = G - (ratio * G).astype(np.int64)
    emp = {t: float((tvis == t).mean()) for t in p}
    assert max(abs(emp[t] - p[t]) for t in p) < 2e-3                    # the distribution itself
    ms = np.vectorize(table.get)(tvis)
    model = bench.ddp_model(table, G, ms_per_step=ms[:, 0].mean() + 0.4)
    assert abs(model['expected_replay_ms'] - ms[:, 0].mean()) < 5e-3 and abs(model['other_ms'] - 0.4) < 5e-3
    for n in (2, 4, 8):
        sim = ms[:, :n].max(axis=1).mean()
        got = model['predicted'][str(n)]
        assert abs(got['expected_max_replay_ms'] - sim) < 5e-3, (n, got, sim)
        assert abs(got['speedup'] - n * (ms[:, 0].mean() + 0.4) / (sim + 0.4)) < 5e-3


def test_steps_below_one_is_refused():
    r = _run(['--steps', '0', '--warmup', '0'])
    assert r.returncode != 0 and '--steps' in r.stderr
    assert '{"metric"' not in r.stdout


def test_full_is_off_by_default(monkeypatch):
    """A plain run measures the headline only; --full asks for every other measurement and check."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1'])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--full'])
    assert bench.parse().full is True


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_the_extras():
    """Without --full the line holds the headline figure and none of the extra measurements; with --full (here without
    the other workloads' legs and the CPU baseline) the rooflines, the T_vis table and the box calibration come back."""
    import json
    import proc_util
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'PDAE_BENCH_BACKEND')}
    base = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '16']
    lines = {}
    for name, extra in (('plain', []), ('full', ['--full', '--no-also', '--no-cpu-baseline', '--probe-steps', '1'])):
        r = proc_util.run(base + extra, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-4000:]
        got = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
        assert len(got) == 1, r.stdout[-2000:]
        lines[name] = json.loads(got[0])
    for d in lines.values():
        assert d['metric'] == 'pretrain point-clouds/sec (N=1024,G=64)' and d['unit'] == 'clouds/s'
        assert d['higher_is_better'] is True and d['value'] > 0 and d['ms_per_step'] > 0 and d['dtype']
        assert d['steps'] == 2 and d['warmup'] == 1
    plain, full = lines['plain'], lines['full']
    assert plain['full'] is False and full['full'] is True
    assert plain['roofline'] is None and plain['box_calibration'] is None and plain['timed_regions'] is None
    for key in ('roofline_geometry', 'also', 'cpu_baseline', 'tvis_table', 'ddp_model', 'whole_step'):
        assert key not in plain, key
    assert full['roofline'] is not None and full['timed_regions'] is not None and 'mfma_bf16' in full['box_calibration']
    assert full['tvis_table'] and full['ddp_model'] and full['whole_step']
    assert 'also' not in full and 'cpu_baseline' not in full


def test_dump_outputs_writes_a_fixed_sample_within_the_budget(tmp_path):
    """--dump-outputs DIR: the step's two losses and the flat parameter / gradient buffers as float32 .npy files, at most
    64 MB in all; buffers too large for that are written as the same seeded sample of elements in every run."""
    import importlib.util
    import types
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 12 * 10 ** 6                                           # 2 x 48 MB as float32: over the budget
    g = torch.Generator().manual_seed(0)
    model = types.SimpleNamespace(flat_param=torch.randn(n, generator=g), flat_grad=torch.randn(n, generator=g))
    out = (torch.tensor(0.25), torch.zeros(1))
    recs = [bench.dump_outputs(str(tmp_path / d), out, model) for d in ('a', 'b')]
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['grads.npy', 'loss.npy', 'loss2.npy', 'params.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64 * 10 ** 6
    assert recs[0]['arrays']['params']['sample_of'] == n and recs[0]['arrays']['loss']['sample_of'] is None
    a = {f: np.load(tmp_path / 'a' / f) for f in files}
    assert all(v.dtype == np.float32 for v in a.values()) and a['loss.npy'] == np.float32(0.25)
    for f in files:
        assert np.array_equal(a[f], np.load(tmp_path / 'b' / f)), f
    k = a['params.npy'].size
    idx = np.sort(np.random.default_rng(0).choice(n, k, replace=False))
    assert np.array_equal(a['params.npy'], model.flat_param.numpy()[idx])
    assert np.array_equal(a['grads.npy'], model.flat_grad.numpy()[idx])
    small = types.SimpleNamespace(flat_param=torch.arange(10.), flat_grad=torch.ones(10))
    bench.dump_outputs(str(tmp_path / 'c'), out, small)                  # within the budget: whole buffers
    assert np.array_equal(np.load(tmp_path / 'c' / 'params.npy'), np.arange(10, dtype=np.float32))
    bench.dump_outputs(str(tmp_path / 'd'), out, small, grads=False)     # the eager path: its gradient is cleared
    assert sorted(os.listdir(tmp_path / 'd')) == ['loss.npy', 'loss2.npy', 'params.npy']


@pytest.mark.gpu
def test_dump_outputs_are_the_same_every_run(tmp_path):
    """Two runs of bench.py with the same arguments compute the same last timed step, bit for bit: the inputs are seeded
    and --dump-outputs runs the step with ordered reductions (--deterministic)."""
    import numpy as np
    import proc_util
    args = ['--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '16', '--no-also', '--no-cpu-baseline',
            '--no-calibration', '--no-tvis-table', '--probe-steps', '0']
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'PDAE_BENCH_BACKEND')}
    for d in ('a', 'b'):
        r = proc_util.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args + ['--dump-outputs', str(tmp_path / d)],
                          timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-4000:]
        assert '"ms_per_step"' in r.stdout
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['grads.npy', 'loss.npy', 'loss2.npy', 'params.npy']
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)), f
