"""Golden vectors for Point-M2AE's hierarchical encoder as the linear-SVM feature extractor, from the LIVE reference.

Runs only where the reference tree exists.  Imports models/Point_M2AE.py in place (tests/golden/ref_import.py: knn_cuda /
pointnet2_ops stubs backed by the C oracle, as for every other fixture), builds its Point_M2AE_SVMFeature, fills it with
weights.fill_state(model, 7), and runs it in evaluation mode on seeded clouds: once in fp32 as it ships and once with
the grouped tensors and the modules cast to double.  Stores inputs and expected outputs only: no weights, no reference
text.

    python tests/golden/make_m2ae_encoder_fixtures.py

  m2ae_svmfeat_{a,b,c}.npz   pts; per level len, T_pad and a strided sample of the valid output rows before the norm (fp64
                             run); the fp32 feature, the fp64 feature and the scalar distance between the two
  m2ae_svmfeat_layout.json   every state_dict key of the reference's model with its shape, and the parameter count

The generator asserts what the tests rely on: no two consecutive levels pad to the same length (the reference would
reuse the previous level's distances, Point_M2AE.py:92 -- INTEGRATION.md section 4), every centre's norm is at least
1e-5 away from its level's radius (no mask decision hangs on rounding), and on (a) and (b) the feature recomputed with
local_radius = [0, 0, 0] differs by at least NO_RADIUS_FLOOR of its largest entry (the fixture sees the padded-key
rule: measured 2.8e-3 on (a), 7.4e-4 on (b), against the tests' 1e-5 pin).
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
import weights  # noqa: E402

MODEL = dict(NAME='Point_M2AE_SVMFeature', corrupt_type=['Drop-Patch'], mask_ratio=0.8, group_sizes=[16, 8, 8],
             num_groups=[512, 256, 64], encoder_depths=[5, 5, 5], encoder_dims=[96, 192, 384],
             local_radius=[0.32, 0.64, 1.28], decoder_depths=[1, 1], decoder_dims=[384, 192], decoder_up_blocks=[1, 1],
             drop_path_rate=0.1, num_heads=6)      # cfgs/finetune_modelnet_svm_pointm2ae.yaml
#           num_groups, group_sizes, N, B, seed, T_pad per level, visible per level
FIXTURES = {'a': ([72, 40, 8], [16, 8, 4], 300, 3, 5, [72, 29, 8], [[72, 67, 72], [29, 27, 29], [8, 8, 8]]),
            'b': ([136, 72, 16], [16, 8, 4], 512, 2, 9, [133, 56, 16], [[131, 133], [56, 51], [16, 16]]),
            'c': ([512, 256, 64], [16, 8, 8], 2048, 2, 21, [512, 255, 64], [[512, 512], [252, 255], [64, 64]])}
SEED = 7
STRIDE = 7
# the least relative change of the feature under local_radius = [0, 0, 0].  (a): 1e-3 (the live reference gives 2.8e-3).
# (b): the live reference gives 7.4e-4, below 1e-3, so its floor is 1e-4 = ten times the 1e-5 pin of the GPU test: an
# encoder that hides the padded keys still misses that pin by a factor of 70 on (b)
NO_RADIUS_FLOOR = {'a': 1e-3, 'b': 1e-4}


def build(num_groups, group_sizes):
    from easydict import EasyDict
    M = importlib.import_module('models.Point_M2AE')
    cfg = EasyDict(dict(MODEL, num_groups=list(num_groups), group_sizes=list(group_sizes)))
    model = M.Point_M2AE_SVMFeature(cfg)
    return weights.fill_state(model, SEED).eval()


def group(model, pts):
    neighborhoods, centers, idxs = [], [], []
    src = pts
    for divider in model.group_dividers:
        nb, c, idx = divider(src)
        neighborhoods.append(nb), centers.append(c), idxs.append(idx)
        src = c
    return neighborhoods, centers, idxs


def run_encoder(model, neighborhoods, centers, idxs, dtype):
    """h_encoder in `dtype` -> (feature, per level (lens, T_pad, valid rows before the norm))."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    outs, hooks = [], []
    try:
        enc = model.h_encoder.to(dtype)
        for blk in enc.encoder_blocks:
            hooks.append(blk.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())))
        with torch.no_grad():
            x_list, vis_list, _ = enc([t.to(dtype) for t in neighborhoods], [t.to(dtype) for t in centers], idxs, eval=True)
        x = x_list[-1]
        feature = x.mean(1) + x.max(1)[0]
        levels = [(v.sum(1).numpy().astype(np.int32), int(v.shape[1]), o[v].numpy()) for o, v in zip(outs, vis_list)]
    finally:
        for h in hooks:
            h.remove()
        torch.set_default_dtype(prev)
        model.h_encoder.to(prev)
    return feature.numpy(), levels


def main():
    ref_import.setup()
    ref_import.cpu_cuda_noop()
    torch.Tensor.cuda = lambda self, *a, **k: self               # H_Encoder.forward calls .cuda() on fresh tensors
    from point_dae_amd.synthetic import shapenet_like_clouds
    for name, (num_groups, group_sizes, N, B, seed, t_pads, visible) in FIXTURES.items():
        model = build(num_groups, group_sizes)
        pts = shapenet_like_clouds(B, N, seed=seed)
        with torch.no_grad():
            neighborhoods, centers, idxs = group(model, torch.from_numpy(pts))
            f32_direct = model(torch.from_numpy(pts)).numpy()
        f32, _ = run_encoder(model, neighborhoods, centers, idxs, torch.float32)
        assert np.array_equal(f32, f32_direct)
        f64, levels = run_encoder(model, neighborhoods, centers, idxs, torch.float64)
        out = {'pts': pts, 'feature32': f32, 'feature64': f64,
               'dist': np.float64(np.abs(f32.astype(np.float64) - f64).max() / np.abs(f64).max())}
        for i, (lens, t_pad, rows) in enumerate(levels):
            assert t_pad == t_pads[i] and lens.tolist() == visible[i], (name, i, t_pad, lens)
            out['len%d' % i], out['T_pad%d' % i], out['rows%d_sample' % i] = lens, np.int32(t_pad), rows[::STRIDE]
            # no mask decision may hang on rounding: a padded row sits at the origin
            norms = np.linalg.norm(centers[i].numpy().astype(np.float64), axis=-1)
            margin = np.abs(norms - MODEL['local_radius'][i]).min()
            assert margin >= 1e-5, (name, i, margin)
        # the stale-distance quirk (Point_M2AE.py:92) must not occur: the product always uses the level's own centres
        assert all(a != b for a, b in zip(t_pads, t_pads[1:])), (name, t_pads)
        # the padded-key rule must be visible to the fixture
        model.h_encoder.local_radius = [0, 0, 0]
        f_norad, _ = run_encoder(model, neighborhoods, centers, idxs, torch.float64)
        rel = np.abs(f_norad - f64).max() / np.abs(f64).max()
        if name in NO_RADIUS_FLOOR:
            assert rel >= NO_RADIUS_FLOOR[name], (name, rel)
        path = os.path.join(HERE, 'm2ae_svmfeat_%s.npz' % name)
        np.savez_compressed(path, **out)
        print('wrote %s (%d bytes): T_pad %s, fp32 vs fp64 %.2e, radius [0,0,0] vs shipped %.2e'
              % (path, os.path.getsize(path), t_pads, out['dist'], rel))
    model = build(MODEL['num_groups'], MODEL['group_sizes'])
    sd = model.state_dict()
    with open(os.path.join(HERE, 'm2ae_svmfeat_layout.json'), 'w') as f:
        json.dump({'state_dict': [[k, list(v.shape)] for k, v in sd.items()],
                   'parameters': int(sum(p.numel() for p in model.parameters()))}, f, indent=1)
    print('layout: %d state_dict entries, %d parameters' % (len(sd), sum(p.numel() for p in model.parameters())))


if __name__ == '__main__':
    main()
