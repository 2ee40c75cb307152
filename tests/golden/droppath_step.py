"""One forward + backward of the Transformer with stochastic depth ON, in a pinned CPU numeric environment.

The model is the transformer_allpatch_cdl1_b3 fixture's (cfg3, all_patch, cdl1, depth 2 + 1) with drop_path_rate 0.1:
the reference and the oracle draw their drop-path masks from the same host RNG stream.  Weights fill_state(., 5), input
the fixture's `pts` (shapenet_like_clouds(2, 1024, seed=9) when it was made), seed_all(77) right before the forward,
loss.backward().

float32 results on the CPU depend on the thread count and on the instruction set that torch and MKL dispatch to.
PINNED_ENV fixes them (one thread, ATen's scalar kernels, MKL's conditional-reproducibility mode COMPATIBLE) and the
step runs without oneDNN.  MKL's COMPATIBLE mode is meant to give the same bits on every CPU of one vendor (on the
fixture's host the result stayed the same with MKL limited to AVX2 or SSE4.2); on another vendor's CPUs MKL sums some
products in another order (`cpu_vendor`).  torch reads these variables when it loads, hence a child process:

    env <PINNED_ENV> python tests/golden/droppath_step.py oracle|reference

prints one JSON line: the loss as float.hex, per parameter the SHA-256 of its float32 gradient bytes (-0.0 counted
as +0.0, as torch.equal does), the gradient's L2 norm and 256 evenly spaced entries of it, and `cpu_vendor`
(/proc/cpuinfo).  `reference` imports the reference from where it lies
(ref_import.py); make_fixtures.py stores its line in transformer_droppath_b2.npz, and
tests/test_model_oracle.py::test_oracle_model_matches_stored_reference_with_drop_path checks the `oracle` line
against it.
"""
import hashlib
import json
import os
import sys

PINNED_ENV = {'ATEN_CPU_CAPABILITY': 'default', 'MKL_CBWR': 'COMPATIBLE', 'OMP_NUM_THREADS': '1',
              'MKL_NUM_THREADS': '1', 'PYTHONDONTWRITEBYTECODE': '1'}

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def run(side, pts=None):
    for k, v in PINNED_ENV.items():
        if os.environ.get(k) != v:
            raise SystemExit('droppath_step.py: run with %s=%s (PINNED_ENV)' % (k, v))
    sys.path[:0] = [ROOT, os.path.dirname(HERE), HERE]
    import torch
    torch.set_num_threads(1)
    torch.backends.mkldnn.enabled = False
    from golden_util import fill_state, load_fixture, model_cfg
    import ref_import as R
    cfg = model_cfg(load_fixture('transformer_allpatch_cdl1_b3.npz'))
    cfg.transformer_config.drop_path_rate = 0.1
    if side == 'reference':
        R.setup()
        R.cpu_cuda_noop()
        import models.PointCAE_transformer as M
        from easydict import EasyDict
        model = M.PointCAE_transformer(EasyDict(cfg))
    elif side == 'oracle':
        from oracle import model as OM
        model = OM.PointCAE_transformer(cfg)
    else:
        raise SystemExit('droppath_step.py: oracle or reference, not %r' % side)
    model = fill_state(model, 5).train()
    if pts is None:
        pts = load_fixture('transformer_droppath_b2.npz')['pts']
    x = torch.from_numpy(pts)
    R.seed_all(77)
    loss, _ = model(x, x)
    loss.backward()
    from golden_util import grad_sample
    grads, norms, samples = {}, {}, {}
    for name, p in model.named_parameters():
        g = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().float() + 0.0     # -0.0 -> +0.0
        grads[name] = hashlib.sha256(g.contiguous().numpy().tobytes()).hexdigest()
        norms[name] = g.double().norm().item()
        samples[name] = [float(v) for v in grad_sample(g)]
    return {'loss': loss.item().hex(), 'grads': grads, 'norms': norms, 'samples': samples, 'cpu_vendor': cpu_vendor()}


def cpu_vendor():
    try:
        with open('/proc/cpuinfo') as f:
            return next((ln.split(':', 1)[1].strip() for ln in f if ln.startswith('vendor_id')), None)
    except OSError:
        return None


if __name__ == '__main__':
    pts = None
    if len(sys.argv) > 2 and sys.argv[2] == '--new-input':      # make_fixtures.py: the input the fixture will hold
        sys.path.insert(0, ROOT)
        from point_dae_amd.synthetic import shapenet_like_clouds
        pts = shapenet_like_clouds(2, 1024, seed=9)
    print(json.dumps(run(sys.argv[1] if len(sys.argv) > 1 else 'oracle', pts)), flush=True)
