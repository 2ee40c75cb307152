"""Golden vectors for the PointNet++ classifier PointNetv2 (models/PointCAE_pointnetv2.py), from the LIVE reference.

Runs only where the reference tree exists (tests/golden/ref_import.py: the native ops replaced by the C oracle).  The
model is built from the reference's finetune_modelnet_transferring_features_PointNetv2.yaml, filled with
weights.fill_state(model, SEED) -- the weights are never stored -- its Dropout modules set to p = 0, and run on the
clouds of pointnetv2_svmfeat_a.npz (B = 2, N = 1024, the smallest batch the encoder's fixed 512 / 128 centres allow;
same seed, so the clouds and the FPS / ball-query indices that fixture records are this one's too and are not stored
again; make_svmfeat_fixtures.py asserted that none of those decisions hangs on rounding).  Geometry in fp32, dense math
in fp64 (make_svmfeat_fixtures.Recorder), as there:

  pointnetv2_cls_b2.npz     labels; eval_logits32 / eval_logits64 (evaluation mode, the shipped fp32 path and fp64);
                            train_logits64, loss64 (training mode: batch statistics everywhere), and of every parameter's
                            fp64 gradient 'grad/<name>/norm' (fp64) with '/full' (<= 1536 elements) or '/sample' (256
                            evenly spaced elements), rounded to fp32 for storage (6e-8 relative, far below every bound
                            the tests set); eval_dist / train_dist / loss_dist / grad_dist: the reference's own fp32 run
                            against its fp64 one (logits; logits, loss and the worst gradient tensor in training mode),
                            max-abs over max-abs
  pointnetv2_cls_layout.json  state_dict keys and shapes, the parameter count, the missing / unexpected keys of the
                            reference's own load_model_from_ckpt on this repository's Point_CAE_PointNetv2 checkpoint

A note on conditioning.  At B = 2 the head's two BatchNorm1d layers normalise over two rows: x_hat = +-(1 - 2 eps / d^2)
for a column whose two entries differ by d, so the training-mode logits depend on the encoder only through terms of
order eps / d^2 and every gradient behind the head is that small and that ill-conditioned in fp32.  The fixture records
what the reference computes; the kernels' own precision is pinned per op (tests/test_gpu_sa_train.py).

    python tests/golden/make_pointnetv2_cls_fixtures.py
"""
import copy
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
import make_svmfeat_fixtures as S  # noqa: E402

CFG = 'cfgs/finetune_modelnet_transferring_features_PointNetv2.yaml'
PRETRAIN_CFG, PRETRAIN_MODEL = 'cfgs/pretrain_PointCAE_clean.yaml', 'Point_CAE_PointNetv2'
GEOMETRY = 'pointnetv2_svmfeat_a.npz'
SEED = S.SEEDS['pointnetv2']['a']
FULL = 1536


def _yaml():
    import yaml
    return yaml.safe_load(open(os.path.join(R.REF, CFG)))


def build(seed):
    import importlib
    from easydict import EasyDict
    import pointnet2_utils as vendored
    vendored.GroupAll.ret_grouped_xyz = False         # attribute read at pointnet2_utils.py:421, never set (:386-389)
    M = importlib.import_module('models.PointCAE_pointnetv2')
    model = weights.fill_state(M.PointNetv2(EasyDict(_yaml()['model'])), seed)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _group_points_grad(grad_out, idx, N):
    """The backward of the vendored GroupingOperation in the gradient's own dtype (the stub of ref_import.py goes through
    the fp32 C oracle, which would round the gradient that sa2 hands to sa1): (B, C, np, ns), (B, np, ns) -> (B, C, N)."""
    b, c = grad_out.shape[:2]
    flat = idx.long().reshape(b, 1, -1).expand(-1, c, -1)
    return grad_out.new_zeros(b, c, N).scatter_add_(2, flat, grad_out.reshape(b, c, -1))


def _sample(t, n=256):
    flat = t.detach().reshape(-1)
    idx = np.linspace(0, flat.numel() - 1, min(n, flat.numel())).astype(np.int64)
    return flat[idx].numpy()


def fixture():
    from point_dae_amd.synthetic import shapenet_like_clouds
    geo = np.load(os.path.join(HERE, GEOMETRY))
    assert int(geo['seed']) == SEED
    pts = shapenet_like_clouds(S.B, S.N, seed=SEED)
    assert np.array_equal(pts, geo['pts'])
    model = build(SEED)
    assert model.smoothing is True
    labels = np.random.default_rng(SEED).integers(0, model.cls_dim, S.B).astype(np.int64)
    out = {'seed': np.int64(SEED), 'labels': labels}

    def check_geometry(rec):
        for lvl in range(2):
            assert np.array_equal(rec.fps[lvl].numpy().astype(np.int32), geo['fps_idx%d' % lvl]), lvl
            assert np.array_equal(rec.ball[lvl].numpy().astype(np.int32), geo['ball_idx%d' % lvl]), lvl

    # evaluation mode: the shipped fp32 path and fp64
    ev = copy.deepcopy(model).eval()
    with torch.no_grad():
        out['eval_logits32'] = ev(torch.from_numpy(pts)).numpy()
    with S.Recorder() as rec:
        ev.double()
        with torch.no_grad():
            out['eval_logits64'] = ev(torch.from_numpy(pts).double()).numpy()
    check_geometry(rec)
    out['eval_dist'] = np.float64(np.abs(out['eval_logits32'] - out['eval_logits64']).max() / np.abs(out['eval_logits64']).max())

    # training mode in fp32 as shipped: how far the reference's own fp32 logits lie from its fp64 ones
    tr32 = copy.deepcopy(model).train()
    logits32 = tr32(torch.from_numpy(pts))
    loss32, _ = tr32.get_loss_acc(logits32, torch.from_numpy(labels))
    loss32.backward()
    # training mode in fp64: logits, loss, every gradient
    tr = copy.deepcopy(model).train()
    with S.Recorder() as rec:
        rec._set(sys.modules['pointnet2._ext'], 'group_points_grad', _group_points_grad)
        tr.double()
        logits = tr(torch.from_numpy(pts).double())
        loss, _ = tr.get_loss_acc(logits, torch.from_numpy(labels))
        loss.backward()
    check_geometry(rec)
    out['train_logits64'] = logits.detach().numpy()
    out['loss64'] = np.float64(loss.item())
    out['train_dist'] = np.float64(np.abs(logits32.detach().numpy() - out['train_logits64']).max()
                                   / np.abs(out['train_logits64']).max())
    out['loss_dist'] = np.float64(abs(loss32.item() - loss.item()) / abs(loss.item()))
    grad_dist = 0.0
    g32 = {name: p.grad for name, p in tr32.named_parameters()}
    for name, p in tr.named_parameters():
        assert p.grad is not None, name
        # the reference's own fp32 error on the elements the fixture stores, in the tests' metric (max-abs over max-abs of
        # those elements); the analytically zero gradients are rounding noise on both sides and are left out
        pick = (lambda t: t) if p.grad.numel() <= FULL else (lambda t: torch.from_numpy(_sample(t)))
        if p.grad.norm().item() > 1e-9:
            own = float((pick(g32[name].double()) - pick(p.grad)).abs().max() / pick(p.grad).abs().max())
            print('  reference fp32 vs fp64  %-55s %.2e' % (name, own))
            grad_dist = max(grad_dist, own)
        key = 'grad/' + name
        out[key + '/norm'] = np.float64(p.grad.norm().item())
        if p.grad.numel() <= FULL:
            out[key + '/full'] = p.grad.numpy().astype(np.float32)
        else:
            out[key + '/sample'] = _sample(p.grad).astype(np.float32)
    out['grad_dist'] = np.float64(grad_dist)
    path = os.path.join(HERE, 'pointnetv2_cls_b2.npz')
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(HERE, GEOMETRY))
    print('wrote %s (%d bytes, limit %d): eval fp32 vs fp64 %.2e, train fp32 vs fp64 logits %.2e loss %.2e worst gradient '
          '%.2e, loss %.6f' % (path, os.path.getsize(path), limit, out['eval_dist'], out['train_dist'], out['loss_dist'],
                               out['grad_dist'], out['loss64']))
    assert os.path.getsize(path) <= limit
    return tr


def layout():
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    R.seed_all(0)
    ref = build(0)
    sd = ref.state_dict()
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, PRETRAIN_CFG)).model
    pre_cfg.NAME = PRETRAIN_MODEL
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
    doc = dict(state_dict=[[k, list(v.shape)] for k, v in sd.items()],
               parameters=int(sum(p.numel() for p in ref.parameters())),
               missing_keys=sorted(seen['r'].missing_keys), unexpected_keys=sorted(seen['r'].unexpected_keys),
               pretrain_config=PRETRAIN_CFG, pretrain_model=PRETRAIN_MODEL, reference_config=CFG, values=_yaml())
    with open(os.path.join(HERE, 'pointnetv2_cls_layout.json'), 'w') as f:
        json.dump(doc, f, indent=1)
    print('PointNetv2: %d state_dict entries, %d parameters, %d missing, %d unexpected'
          % (len(doc['state_dict']), doc['parameters'], len(doc['missing_keys']), len(doc['unexpected_keys'])))


if __name__ == '__main__':
    R.setup()
    R.cpu_cuda_noop()
    fixture()
    layout()
