"""Golden vectors for PointTransformerPartSeg (point_dae_amd/part_seg.py) from the LIVE reference's segmentation model
(segmentation/models/pt.py get_model).

Runs only where the reference tree exists (tests/golden/ref_import.py: the native ops replaced by the C oracle).  pt.py
is loaded by file path; its `import pointnet2_utils` and `import logger` must find the files of segmentation/, not the
vendored extensions/pointnet2 that ref_import puts on the path, so the two names are bound in sys.modules around the
import and restored afterwards.  get_model(50) is filled with weights.fill_state(model, seed) -- non-trivial running
estimates, so the weights are never stored -- and run in evaluation mode on seeded B = 2, N = 512 clouds twice: in fp32
as shipped, and with the geometry (FPS, kNN) from fp32 copies and the dense math in fp64.

    python tests/golden/make_partseg_fixtures.py            # writes the fixtures
    python tests/golden/make_partseg_fixtures.py search     # prints the seeds below 40 whose margins hold

  partseg_{a,b}.npz      pts, cls, fps_idx, knn_idx, three_idx, sub_idx (the seeded 256 points per cloud), logp64 on
                         them, argmax64 and margin64 (the fp64 full-range argmax and top-two gap of EVERY point), dist
  partseg_layout.json    state_dict keys and shapes, the parameter count, the missing / unexpected keys of the
                         reference's own load_model_from_ckpt on this repository's pretraining checkpoint

Asserted here, relied on by the tests: every kNN k-th / (k+1)-th gap and every point's gap between its 3rd- and
4th-nearest centre is at least MARGIN; every FPS winner leads its runner-up by MARGIN or by FPS_ULPS units in the last
place of its fp32 value (make_svmfeat_fixtures.py states why a dense pass needs the ulp form); the reference's fp32
log-probabilities lie at most FP32_DIST (max-abs over max-abs) from its fp64 ones; at most 1 % of the points have an fp64
top-two gap below ARGMAX_MARGIN = 100 x the evaluation pin (1e-5) x the largest |log-probability|.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import as R  # noqa: E402
import weights  # noqa: E402

MARGIN = 1e-6
FPS_ULPS = 16.0
FP32_DIST = 1e-6
PIN = 1e-5
B, N, SUB = 2, 512, 256
SEEDS = {'a': 3, 'b': 7}
PRETRAIN = ('cfgs/pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml',
            'PointCAE_transformer_fc_global_folding_local')


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_pt():
    """segmentation/models/pt.py with `pointnet2_utils` and `logger` resolved inside segmentation/."""
    seg = os.path.join(R.REF, 'segmentation')
    saved = {k: sys.modules.get(k) for k in ('pointnet2_utils', 'logger')}
    try:
        sys.modules['pointnet2_utils'] = _load('pointnet2_utils', os.path.join(seg, 'models', 'pointnet2_utils.py'))
        sys.modules['logger'] = _load('logger', os.path.join(seg, 'logger.py'))
        pt = _load('partseg_reference_pt', os.path.join(seg, 'models', 'pt.py'))
        p2 = sys.modules['pointnet2_utils']
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return pt, p2


def run(model, pts, cls, dtype, rec_cls):
    """The reference's forward in `dtype` with the geometry recorded -> (log-probabilities (B, N, 50), recorder)."""
    onehot = torch.zeros(len(cls), 16, dtype=dtype)
    onehot[torch.arange(len(cls)), torch.from_numpy(cls)] = 1
    with rec_cls() as rec:
        old = model.group_divider.knn
        model.group_divider.knn = rec.KNN(model.group_divider.group_size, transpose_mode=True)
        try:
            model.to(dtype)
            with torch.no_grad():
                # (B, 3, N) as a transposed view: what segmentation/main.py hands over (pt.py:303,45 views it back)
                out = model(torch.from_numpy(pts).to(dtype).transpose(1, 2), onehot)
        finally:
            model.to(torch.float32)
            model.group_divider.knn = old
    return out.numpy(), rec


def fixture(pt, p2, seed):
    import make_svmfeat_fixtures as S
    from point_dae_amd.synthetic import shapenet_like_clouds
    model = weights.fill_state(pt.get_model(50), seed).eval()
    pts = shapenet_like_clouds(B, N, seed=seed)
    cls = np.random.default_rng([seed, 7]).integers(0, 16, B).astype(np.int64)
    l32, rec32 = run(model, pts, cls, torch.float32, S.Recorder)
    l64, rec = run(model, pts, cls, torch.float64, S.Recorder)
    assert torch.equal(rec32.fps[0], rec.fps[0]) and torch.equal(rec32.knn[0], rec.knn[0])
    fi = rec.fps[0].numpy()
    ctr = np.take_along_axis(pts, fi[..., None].astype(np.int64), axis=1)
    # the three nearest centres as the reference's head finds them in fp64 (its matmul-form distance, a sort)
    d_ref = p2.square_distance(torch.from_numpy(pts).double(), torch.from_numpy(ctr).double())
    three = d_ref.sort(dim=-1)[1][:, :, :3].numpy()
    diff = pts[:, :, None, :].astype(np.float64) - ctr[:, None, :, :].astype(np.float64)
    d = np.sort((diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2, axis=-1)
    lead, ulps = S.fps_margin(pts, fi)
    top2 = np.sort(l64, axis=-1)[..., -2:]
    margin64 = top2[..., 1] - top2[..., 0]
    scale = np.abs(l64).max()
    m = dict(fps=lead, fps_ulps=ulps, knn=S.knn_margin(pts, ctr, model.group_divider.group_size),
             three=float((d[..., 3] - d[..., 2]).min()), below=float((margin64 < 100 * PIN * scale).mean()))
    dist = float(np.abs(l32.astype(np.float64) - l64).max() / scale)
    sub = np.stack([np.sort(np.random.default_rng([seed, 11, b]).choice(N, SUB, replace=False)) for b in range(B)])
    out = dict(pts=pts, cls=cls, seed=np.int64(seed), fps_idx=fi.astype(np.int32), knn_idx=rec.knn[0].numpy().astype(np.int64),
               three_idx=three.astype(np.int32), sub_idx=sub.astype(np.int32),
               logp64=np.take_along_axis(l64, sub[..., None], axis=1), argmax64=l64.argmax(-1).astype(np.int32),
               margin64=margin64.astype(np.float32), scale64=np.float64(scale), dist=np.float64(dist))
    return out, m, dist


def holds(m, dist):
    return (m['knn'] >= MARGIN and m['three'] >= MARGIN and (m['fps'] >= MARGIN or m['fps_ulps'] >= FPS_ULPS)
            and m['below'] <= 0.01 and dist <= FP32_DIST)


def layout(pt):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    R.seed_all(0)
    ref = pt.get_model(50)
    sd = ref.state_dict()
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, PRETRAIN[0])).model
    pre_cfg.NAME = PRETRAIN[1]
    pre = MODELS.build(pre_cfg)
    seen = {}
    orig = ref.load_state_dict

    def capture(state, strict=True):
        seen['r'] = orig(state, strict=strict)
        return seen['r']
    ref.load_state_dict = capture
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'ckpt-last.pth')
        torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, path)
        with contextlib.redirect_stdout(io.StringIO()):          # (it prints the whole checkpoint)
            ref.load_model_from_ckpt(path)                        # the reference's own key surgery and load
    return dict(state_dict=[[k, list(v.shape)] for k, v in sd.items()],
                parameters=int(sum(p.numel() for p in ref.parameters())),
                missing_keys=sorted(seen['r'].missing_keys), unexpected_keys=sorted(seen['r'].unexpected_keys),
                pretrain_config=PRETRAIN[0], pretrain_model=PRETRAIN[1])


def main():
    os.chdir(ROOT)
    R.setup()
    R.cpu_cuda_noop()
    pt, p2 = load_pt()
    if len(sys.argv) > 1 and sys.argv[1] == 'search':
        for seed in range(1, 40):
            _, m, dist = fixture(pt, p2, seed)
            print(seed, 'ok' if holds(m, dist) else '--', 'dist %.2e' % dist, ' '.join('%s %.2e' % kv for kv in m.items()),
                  flush=True)
        return
    for name, seed in SEEDS.items():
        out, m, dist = fixture(pt, p2, seed)
        assert holds(m, dist), (name, seed, m, dist)
        path = os.path.join(HERE, 'partseg_%s.npz' % name)
        np.savez_compressed(path, **out)
        print('wrote %s (%d bytes): seed %d, fp32 vs fp64 %.2e, margins %s'
              % (path, os.path.getsize(path), seed, dist, ' '.join('%s %.2e' % kv for kv in m.items())))
    doc = layout(pt)
    with open(os.path.join(HERE, 'partseg_layout.json'), 'w') as f:
        json.dump(doc, f, indent=1)
    print('%d state_dict entries, %d parameters, %d missing, %d unexpected'
          % (len(doc['state_dict']), doc['parameters'], len(doc['missing_keys']), len(doc['unexpected_keys'])))


if __name__ == '__main__':
    main()
