"""Golden vectors for DGCNNPartSeg (point_dae_amd/dgcnn_partseg.py) from the LIVE reference's DGCNN segmentation model
(segmentation/models/dgcnn_partseg.py get_model on segmentation/models/dgcnn_util.py dgcnn_encoder_partseg).

Runs only where the reference tree exists (tests/golden/ref_import.py: ipdb and termcolor stubbed).  The model file does
`from models.dgcnn_util import ...` and `from logger import ...`, which must find the files of segmentation/, not the
top-level models/ package that ref_import registers, so `models` and `logger` are bound in sys.modules around the import
and restored afterwards.  get_model(50) is filled with weights.fill_state(model, seed) -- non-trivial running estimates,
so the weights are never stored -- and run in evaluation mode on seeded B = 2, N = 512 clouds in fp32 and in fp64, with
dgcnn_util.knn wrapped to record the three graphs, the distance expression's fp32 error and every row's k-th / (k+1)-th
gap.

    python tests/golden/make_dgcnn_partseg_fixtures.py            # writes the fixtures
    python tests/golden/make_dgcnn_partseg_fixtures.py search     # prints which seeds 1..12 hold the conditions

  dgcnn_partseg_{a,b}.npz     pts, cls, seed, graphs (3, 2, 512, 20) int16 (the fp64 run's, equal to the fp32 run's), per
                              layer pd_err (3,) = the largest |fp32 - fp64| of the reference's distance expression on the
                              layer's input and gap64 (3, 2, 512) = every row's fp64 gap between its k-th and (k+1)-th
                              neighbour, sub_idx (the seeded 256 points per cloud), logits64 on them, argmax64 and
                              margin64 (the fp64 full-range argmax and top-two gap of EVERY point), scale64, dist
  dgcnn_partseg_layout.json   state_dict keys and shapes, the parameter count, the missing / unexpected keys of the
                              reference's own load_model_from_ckpt on a state_dict with the names and shapes of the
                              reference's Point_CAE_DGCNN_PartSeg (tensors created here)

Asserted here, relied on by the tests: the fp32 and the fp64 run select the same neighbours (as a set: the max over them
does not see their order) on every row of all three layers;
the reference's fp32 logits lie at most FP32_DIST (max-abs over max-abs) from its fp64 ones; per layer at most 2 % of
the rows have gap64 < 8 pd_err (a row whose graph a rounding of the distance may change); at most 1 % of the points have
an fp64 top-two gap below 100 x the evaluation pin (1e-5) x the largest |logit|.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import as R  # noqa: E402
import weights  # noqa: E402

FP32_DIST = 1e-6
PIN = 1e-5
GAP_FACTOR = 8.0
B, N, K, SUB = 2, 512, 20, 256
SEEDS = {'a': 11, 'b': 12}
SEG_NAMES = ('models', 'models.dgcnn_util', 'models.dgcnn_partseg', 'logger')


def load_seg():
    """(segmentation/models/dgcnn_partseg.py, segmentation/models/dgcnn_util.py) with `models` and `logger` resolved
    inside segmentation/; sys.modules is restored."""
    seg = os.path.join(R.REF, 'segmentation')
    saved = {k: sys.modules.get(k) for k in SEG_NAMES}
    try:
        for k in SEG_NAMES:
            sys.modules.pop(k, None)
        pkg = types.ModuleType('models')
        pkg.__path__ = [os.path.join(seg, 'models')]
        sys.modules['models'] = pkg
        sys.path.insert(0, seg)
        try:
            model = importlib.import_module('models.dgcnn_partseg')
            util = importlib.import_module('models.dgcnn_util')
        finally:
            sys.path.remove(seg)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return model, util


class Recorder:
    """Stands in for dgcnn_util.knn: the reference's own selection, recorded, with the distance expression's fp32 error
    and the rows' k-th / (k+1)-th gaps where the run is in fp64."""

    def __init__(self, util):
        self.util, self.orig = util, util.knn
        self.graphs, self.pd_err, self.gap = [], [], []

    def __call__(self, x, k):
        idx = self.orig(x, k)
        self.graphs.append(idx.clone())                   # (get_graph_feature adds the cloud offsets in place)
        if x.dtype == torch.float64:
            pd64, pd32 = self.pd(x), self.pd(x.float()).double()
            self.pd_err.append(float((pd32 - pd64).abs().max()))
            top = pd64.topk(k + 1, dim=-1)[0] if x.shape[2] > k else None
            self.gap.append((top[..., k - 1] - top[..., k]) if top is not None else torch.full(idx.shape[:2], float('inf')))
        return idx

    @staticmethod
    def pd(x):
        inner = -2 * torch.matmul(x.transpose(2, 1), x)
        xx = torch.sum(x ** 2, dim=1, keepdim=True)
        return -xx - inner - xx.transpose(2, 1)

    def __enter__(self):
        self.util.knn = self
        return self

    def __exit__(self, *exc):
        self.util.knn = self.orig
        return False


def run(model, util, pts, cls, dtype):
    onehot = torch.zeros(len(cls), 16, dtype=dtype)
    onehot[torch.arange(len(cls)), torch.from_numpy(cls)] = 1
    with Recorder(util) as rec:
        try:
            model.to(dtype)
            with torch.no_grad():
                out = model(torch.from_numpy(pts).to(dtype).transpose(1, 2).contiguous(), onehot)
        finally:
            model.to(torch.float32)
    return out.numpy(), rec


def fixture(seg_model, util, seed):
    from point_dae_amd.synthetic import shapenet_like_clouds
    model = weights.fill_state(seg_model.get_model(50), seed).eval()
    pts = shapenet_like_clouds(B, N, seed=seed)
    cls = np.random.default_rng([seed, 7]).integers(0, 16, B).astype(np.int64)
    l32, rec32 = run(model, util, pts, cls, torch.float32)
    l64, rec = run(model, util, pts, cls, torch.float64)
    assert len(rec.graphs) == len(rec32.graphs) == 3
    # equal as SETS per row: the max over a row's neighbours does not see their order (two near-equal distances inside
    # the top k may swap places between fp32 and fp64)
    same = [bool(torch.equal(a.sort(-1)[0], b.sort(-1)[0])) for a, b in zip(rec32.graphs, rec.graphs)]
    graphs = torch.stack(rec.graphs).numpy()
    gap = torch.stack(rec.gap).numpy()
    pd_err = np.array(rec.pd_err, np.float64)
    close = [float((gap[l] < GAP_FACTOR * pd_err[l]).mean()) for l in range(3)]
    top2 = np.sort(l64, axis=-1)[..., -2:]
    margin64 = top2[..., 1] - top2[..., 0]
    scale = np.abs(l64).max()
    dist = float(np.abs(l32.astype(np.float64) - l64).max() / scale)
    m = dict(same=all(same), close=max(close), below=float((margin64 < 100 * PIN * scale).mean()), dist=dist)
    sub = np.stack([np.sort(np.random.default_rng([seed, 11, b]).choice(N, SUB, replace=False)) for b in range(B)])
    out = dict(pts=pts, cls=cls, seed=np.int64(seed), graphs=graphs.astype(np.int16), pd_err=pd_err, gap64=gap.astype(np.float64),
               sub_idx=sub.astype(np.int32), logits64=np.take_along_axis(l64, sub[..., None], axis=1),
               argmax64=l64.argmax(-1).astype(np.int32), margin64=margin64.astype(np.float32), scale64=np.float64(scale),
               dist=np.float64(dist))
    return out, m


def holds(m):
    return m['same'] and m['dist'] <= FP32_DIST and m['close'] <= 0.02 and m['below'] <= 0.01


def layout(seg_model):
    """The reference's state_dict layout, and what its own load_model_from_ckpt reports for a checkpoint that carries the
    names and shapes of the reference's Point_CAE_DGCNN_PartSeg (models/PointCAE_DGCNN_partseg.py)."""
    from easydict import EasyDict
    R.seed_all(0)
    ref = seg_model.get_model(50)
    sd = ref.state_dict()
    pre_mod = importlib.import_module('models.PointCAE_DGCNN_partseg')
    with contextlib.redirect_stdout(io.StringIO()):
        pre = pre_mod.Point_CAE_DGCNN_PartSeg(EasyDict(NAME='Point_CAE_DGCNN_PartSeg', corrupt_type=[], loss='cdl2'))
    pre_sd = {'module.' + k: torch.zeros(v.shape, dtype=v.dtype) for k, v in pre.state_dict().items()}
    seen = {}
    orig = ref.load_state_dict

    def capture(state, strict=True):
        seen['r'] = orig(state, strict=strict)
        return seen['r']
    ref.load_state_dict = capture
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'ckpt-last.pth')
        torch.save({'base_model': pre_sd}, path)
        with contextlib.redirect_stdout(io.StringIO()):          # (it prints the whole checkpoint's keys)
            ref.load_model_from_ckpt(path)                        # the reference's own key surgery and load
    return dict(state_dict=[[k, list(v.shape)] for k, v in sd.items()],
                parameters=int(sum(p.numel() for p in ref.parameters())),
                missing_keys=sorted(seen['r'].missing_keys), unexpected_keys=sorted(seen['r'].unexpected_keys),
                pretrain_model='Point_CAE_DGCNN_PartSeg',
                pretrain_state_dict=[[k, list(v.shape)] for k, v in pre.state_dict().items()])


def main():
    os.chdir(ROOT)
    R.setup()
    R.cpu_cuda_noop()
    seg_model, util = load_seg()
    if len(sys.argv) > 1 and sys.argv[1] == 'search':
        for seed in range(1, 13):
            _, m = fixture(seg_model, util, seed)
            print(seed, 'ok' if holds(m) else '--', ' '.join('%s %s' % (k, ('%.2e' % v) if isinstance(v, float) else v)
                                                              for k, v in m.items()), flush=True)
        return
    for name, seed in SEEDS.items():
        out, m = fixture(seg_model, util, seed)
        assert holds(m), (name, seed, m)
        path = os.path.join(HERE, 'dgcnn_partseg_%s.npz' % name)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 400 * 1024, os.path.getsize(path)
        print('wrote %s (%d bytes): seed %d, %s, pd_err %s' % (path, os.path.getsize(path), seed, m, out['pd_err']))
    doc = layout(seg_model)
    with open(os.path.join(HERE, 'dgcnn_partseg_layout.json'), 'w') as f:
        json.dump(doc, f, indent=1)
    print('%d state_dict entries, %d parameters, %d missing, %d unexpected'
          % (len(doc['state_dict']), doc['parameters'], len(doc['missing_keys']), len(doc['unexpected_keys'])))


if __name__ == '__main__':
    main()
