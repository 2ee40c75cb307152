"""Golden vectors for the two linear-SVM feature extractors PointNetv2_feat (models/PointCAE_pointnetv2.py) and
PointTransformerNoClassTokenSVMFeature (models/Point_MAE.py), from the LIVE reference.

Runs only where the reference tree exists (tests/golden/ref_import.py: the native ops replaced by the C oracle).  Each
model is built from the reference's finetune_modelnet_svm_classification.yaml with its NAME set, filled with
weights.fill_state(model, seed) -- non-trivial running estimates, so the weights are never stored -- and run in
evaluation mode on seeded B = 2, N = 1024 clouds twice: in fp32 as shipped, and with the geometry in fp32 and the dense
math in fp64 (the modules cast to double; gather / group stubs that keep the dtype, indices taken from fp32 copies of
the coordinates, which are fp32 values either way).  Stores inputs and expected outputs only.

    python tests/golden/make_svmfeat_fixtures.py            # writes the fixtures
    python tests/golden/make_svmfeat_fixtures.py search     # prints, per model, the seeds below 60 whose margins hold

  pointnetv2_svmfeat_{a,b}.npz    pts, feature32, feature64, dist, fps_idx0/1, ball_idx0/1
  transformer_svmfeat_{a,b}.npz   pts, feature32, feature64, dist, fps_idx, knn_idx
  svmfeat_layout.json             per model: state_dict keys and shapes, the parameter count, the missing / unexpected
                                  keys of the reference's own load_model_from_ckpt on this repository's pretraining
                                  checkpoint, the reference YAML's values and what the new config changes in them

The generator asserts what the tests rely on: no geometric decision hangs on rounding -- every ball-query |d^2 - r^2|
and every kNN k-th / (k+1)-th gap is at least MARGIN, every FPS winner leads its runner-up by at least MARGIN -- and
the reference's own fp32 feature lies at most FP32_DIST (max-abs over max-abs) from its fp64 feature.

One FPS pass cannot meet the absolute MARGIN: PointNet++'s first level keeps 512 of 1024 points, so late winners lead
a few hundred candidates whose squared distances to the chosen set lie within ~1e-4 of each other, and the least of the
1022 leads of a fixture was between 2e-9 and 1.9e-7 on every seed from 1 to 59 (`search` prints them).  What that pass
must satisfy instead is stated in the number format: each lead is at least FPS_ULPS = 16 units in the last place of the
winner's fp32 value -- both sides evaluate ((dx*dx + dy*dy) + dz*dz) and the running minimum in fp32 with every
operation rounded, eight roundings per value, so 16 ulps is twice what any other legitimate rounding of the same
expression could move.  Every other decision (the second level's FPS, both ball queries, the Transformer's FPS and kNN)
keeps the absolute MARGIN.
"""
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

CFG = 'cfgs/finetune_modelnet_svm_classification.yaml'
MARGIN = 1e-6
FPS_ULPS = 16.0                                       # PointNet++'s first FPS pass: see above
FP32_DIST = 1e-6
B, N = 2, 1024
# model -> (module, class, new config, pretraining config, pretraining model)
SPECS = {
    'pointnetv2': ('models.PointCAE_pointnetv2', 'PointNetv2_feat', 'finetune_modelnet_svm_pointnetv2.yaml',
                   'cfgs/pretrain_PointCAE_clean.yaml', 'Point_CAE_PointNetv2'),
    'transformer': ('models.Point_MAE', 'PointTransformerNoClassTokenSVMFeature', 'finetune_modelnet_svm_transformer.yaml',
                    'cfgs/pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml',
                    'PointCAE_transformer_fc_global_folding_local'),
}
SEEDS = {'pointnetv2': {'a': 36, 'b': 22}, 'transformer': {'a': 5, 'b': 21}}
SA_LEVELS = ((512, 0.2, 32), (128, 0.4, 64))          # models/pointnetv2_util.py:323-324
GROUP_SIZE = 32                                      # the YAML's group_size


def _yaml():
    import yaml
    return yaml.safe_load(open(os.path.join(R.REF, CFG)))


def build(kind, seed):
    import importlib
    from easydict import EasyDict
    if kind == 'pointnetv2':
        import pointnet2_utils as vendored
        vendored.GroupAll.ret_grouped_xyz = False     # attribute read at pointnet2_utils.py:421, never set (:386-389)
    module, cls = SPECS[kind][:2]
    cfg = EasyDict(dict(_yaml()['model'], NAME=cls))
    model = getattr(importlib.import_module(module), cls)(cfg)
    return weights.fill_state(model, seed).eval()


# ---- geometry in fp32, recorded; gather / group that keep the dtype ----------------------------------------------------
class Recorder:
    """Wraps the index-producing native ops of both import paths (pointnet2._ext of the vendored extension,
    pointnet2_ops.pointnet2_utils + knn_cuda of models/Point_MAE.py) so that they see fp32 copies of the coordinates
    and their results are recorded, and replaces the gathers by dtype-preserving framework ops."""

    def __init__(self):
        self.fps, self.ball, self.knn = [], [], []
        self._saved = []

    def _set(self, obj, name, value):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        from oracle import ops as O
        ext = sys.modules['pointnet2._ext']
        p2u = sys.modules['pointnet2_ops.pointnet2_utils']

        def fps(xyz, npoint):
            idx = torch.from_numpy(O.furthest_point_sample(xyz.detach().float().numpy(), npoint))
            self.fps.append(idx)
            return idx

        def ball(new_xyz, xyz, radius, nsample):
            idx = torch.from_numpy(O.ball_query(radius, nsample, xyz.detach().float().numpy(),
                                                new_xyz.detach().float().numpy()))
            self.ball.append(idx)
            return idx

        def gather(features, idx):                     # (B, C, N), (B, m) -> (B, C, m)
            return torch.gather(features, 2, idx.long().unsqueeze(1).expand(-1, features.shape[1], -1))

        def group(features, idx):                      # (B, C, N), (B, np, ns) -> (B, C, np, ns)
            b, c, _ = features.shape
            flat = idx.long().reshape(b, 1, -1).expand(-1, c, -1)
            return torch.gather(features, 2, flat).reshape(b, c, idx.shape[1], idx.shape[2])

        self._set(ext, 'furthest_point_sampling', fps)
        self._set(ext, 'ball_query', ball)
        self._set(ext, 'gather_points', gather)
        self._set(ext, 'group_points', group)
        self._set(p2u, 'furthest_point_sample', fps)
        self._set(p2u, 'gather_operation', gather)
        knn_mod = sys.modules['knn_cuda']
        rec = self

        class KNN(torch.nn.Module):
            def __init__(self, k, transpose_mode=False):
                super().__init__()
                self.k = k
                assert transpose_mode

            def forward(self, ref, query):
                d, i = O.knn(ref.detach().float().numpy(), query.detach().float().numpy(), self.k)
                rec.knn.append(torch.from_numpy(i))
                return torch.from_numpy(d), torch.from_numpy(i)
        self._set(knn_mod, 'KNN', KNN)
        self.KNN = KNN
        return self

    def __exit__(self, *exc):
        for obj, name, value in reversed(self._saved):
            setattr(obj, name, value)
        return False


def run(kind, model, pts, dtype):
    """The reference's forward in `dtype` with the geometry recorded -> (feature, recorder)."""
    with Recorder() as rec:
        if kind == 'transformer':                      # Group holds its KNN module from construction
            old = model.group_divider.knn
            model.group_divider.knn = rec.KNN(model.group_divider.group_size, transpose_mode=True)
        try:
            model.to(dtype)
            with torch.no_grad():
                f = model(torch.from_numpy(pts).to(dtype))
        finally:
            model.to(torch.float32)
            if kind == 'transformer':
                model.group_divider.knn = old
    return f.numpy(), rec


# ---- margins --------------------------------------------------------------------------------------------------------
def _sq(a, b):
    """((dx*dx + dy*dy) + dz*dz) in fp32, each operation rounded: the geometry kernels' squared distance."""
    d = (a - b).astype(np.float32)
    return ((d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)).astype(np.float32) \
        + (d[..., 2] * d[..., 2]).astype(np.float32)


def fps_margin(xyz, idx):
    """(the least lead of an FPS winner over its runner-up, the least lead in ulps of the winner's fp32 value), replaying
    the recorded order (points with |p|^2 <= 1e-3 are never selected: sampling_gpu.cu)."""
    worst, worst_ulps = np.inf, np.inf
    for b in range(xyz.shape[0]):
        p = xyz[b].astype(np.float32)
        ok = (p.astype(np.float64) ** 2).sum(-1) > 1e-3
        mind = np.full(p.shape[0], 1e10, np.float32)
        assert idx[b, 0] == 0
        for j in range(1, idx.shape[1]):
            mind = np.minimum(mind, _sq(p, p[idx[b, j - 1]]))
            cand = np.where(ok, mind, -1.0)
            order = np.argsort(-cand, kind='stable')
            assert order[0] == idx[b, j], (b, j)
            lead = float(cand[order[0]]) - float(cand[order[1]])
            worst = min(worst, lead)
            worst_ulps = min(worst_ulps, lead / float(np.spacing(np.float32(cand[order[0]]))))
    return worst, worst_ulps


def ball_margin(xyz, centres, radius):
    d2 = _sq(xyz[:, None, :, :], centres[:, :, None, :]).astype(np.float64)
    return float(np.abs(d2 - np.float64(np.float32(radius)) ** 2).min())


def knn_margin(xyz, centres, k):
    d2 = np.sort(_sq(xyz[:, None, :, :], centres[:, :, None, :]).astype(np.float64), axis=-1)
    return float((d2[..., k] - d2[..., k - 1]).min())


def margins(kind, pts, rec):
    out = {}
    if kind == 'pointnetv2':
        src = pts
        for lvl, (npoint, radius, _) in enumerate(SA_LEVELS):
            fi = rec.fps[lvl].numpy()
            ctr = np.take_along_axis(src, fi[..., None].astype(np.int64), axis=1)
            lead, ulps = fps_margin(src, fi)
            if lvl == 0:
                out['fps0_abs'], out['fps0_ulps'] = lead, ulps
            else:
                out['fps%d' % lvl] = lead
            out['ball%d' % lvl] = ball_margin(src, ctr, radius)
            src = ctr
    else:
        fi = rec.fps[0].numpy()
        ctr = np.take_along_axis(pts, fi[..., None].astype(np.int64), axis=1)
        out['fps'] = fps_margin(pts, fi)[0]
        out['knn'] = knn_margin(pts, ctr, GROUP_SIZE)
    return out


def fixture(kind, seed):
    """-> (arrays, margins, fp32-vs-fp64 distance) of one seed."""
    from point_dae_amd.synthetic import shapenet_like_clouds
    model = build(kind, seed)
    pts = shapenet_like_clouds(B, N, seed=seed)
    with torch.no_grad():
        direct = model(torch.from_numpy(pts)).numpy()              # the stock stubs: the shipped fp32 path
    f32, rec32 = run(kind, model, pts, torch.float32)
    assert np.array_equal(f32, direct), 'the recording stubs change the fp32 feature'
    f64, rec = run(kind, model, pts, torch.float64)
    for a, b in zip(rec32.fps + rec32.ball + rec32.knn, rec.fps + rec.ball + rec.knn):
        assert torch.equal(a, b), 'the fp64 run took other geometric decisions'
    dist = float(np.abs(f32.astype(np.float64) - f64).max() / np.abs(f64).max())
    out = {'pts': pts, 'feature32': f32, 'feature64': f64, 'dist': np.float64(dist), 'seed': np.int64(seed),
           'zero_fraction': np.float64((f64 == 0).mean())}
    if kind == 'pointnetv2':
        for lvl in range(2):
            out['fps_idx%d' % lvl] = rec.fps[lvl].numpy().astype(np.int32)
            out['ball_idx%d' % lvl] = rec.ball[lvl].numpy().astype(np.int32)
    else:
        out['fps_idx'] = rec.fps[0].numpy().astype(np.int32)
        out['knn_idx'] = rec.knn[0].numpy().astype(np.int64)
    return out, margins(kind, pts, rec), dist


def layout(kind):
    import importlib
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    module, cls, new_cfg, pre_path, pre_name = SPECS[kind]
    R.seed_all(0)
    ref = build(kind, 0)
    sd = ref.state_dict()
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, pre_path)).model
    pre_cfg.NAME = pre_name
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
        ref.load_model_from_ckpt(path)                 # the reference's own key surgery and load
    values = _yaml()
    values['model']['NAME'] = cls
    return dict(state_dict=[[k, list(v.shape)] for k, v in sd.items()],
                parameters=int(sum(p.numel() for p in ref.parameters())),
                missing_keys=sorted(seen['r'].missing_keys), unexpected_keys=sorted(seen['r'].unexpected_keys),
                pretrain_config=pre_path, pretrain_model=pre_name,
                configs={new_cfg: dict(reference=CFG, changes={'model.NAME': cls}, values=values)})


def margins_hold(m):
    return all(v >= (FPS_ULPS if k == 'fps0_ulps' else MARGIN) for k, v in m.items() if k != 'fps0_abs')


def holds(m, dist):
    return margins_hold(m) and dist <= FP32_DIST


def main():
    R.setup()
    R.cpu_cuda_noop()
    if len(sys.argv) > 1 and sys.argv[1] == 'search':
        for kind in SPECS:
            for seed in range(1, 60):
                _, m, dist = fixture(kind, seed)
                print(kind, seed, 'ok' if holds(m, dist) else '--', 'dist %.2e' % dist,
                      ' '.join('%s %.2e' % kv for kv in m.items()), flush=True)
        return
    doc = {}
    for kind in SPECS:
        for name, seed in SEEDS[kind].items():
            out, m, dist = fixture(kind, seed)
            assert margins_hold(m), (kind, name, seed, m)
            assert dist <= FP32_DIST, (kind, name, seed, dist)
            path = os.path.join(HERE, '%s_svmfeat_%s.npz' % (kind, name))
            np.savez_compressed(path, **out)
            print('wrote %s (%d bytes): seed %d, fp32 vs fp64 %.2e, zeros %.0f %%, margins %s'
                  % (path, os.path.getsize(path), seed, dist, 100 * out['zero_fraction'],
                     ' '.join('%s %.2e' % kv for kv in m.items())))
        doc[SPECS[kind][1]] = layout(kind)
        print('%s: %d state_dict entries, %d parameters, missing %r, %d unexpected'
              % (SPECS[kind][1], len(doc[SPECS[kind][1]]['state_dict']), doc[SPECS[kind][1]]['parameters'],
                 doc[SPECS[kind][1]]['missing_keys'], len(doc[SPECS[kind][1]]['unexpected_keys'])))
    with open(os.path.join(HERE, 'svmfeat_layout.json'), 'w') as f:
        json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
