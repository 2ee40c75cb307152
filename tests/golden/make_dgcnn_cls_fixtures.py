"""Generate the DGCNN classifier fixtures of tests/golden/ from the LIVE reference (models/PointCAE_DGCNN.py DGCNN).

Runs only in the dev container (needs the reference tree, imported read-only via ref_import.py with the native ops
replaced by the CPU oracle).  What is committed is data only:

  dgcnn_cls_layout.json  every state_dict key of the reference's DGCNN with its shape, and the missing / unexpected keys
                         its load_model_from_ckpt reports (load_state_dict(strict=False)) for a checkpoint of this
                         repository's Point_CAE_DGCNN_FCOnly
  dgcnn_cls_b4.npz       B=4, N=1024, train mode, smoothloss: inputs, labels, the injected dropout keep mask, the
                         encoder's feature, logits, the loss with smoothloss True and False (the same logits), acc,
                         sampled gradients of every parameter for the smoothed loss, the clip_grad_norm_ total norm, the
                         BatchNorm running statistics after the step, and eval-mode logits of the same clouds

The encoder's kNN graphs and max-pools are discrete, and at B=4 the head's training-mode BatchNorm magnifies what they
move: for most seeds the reference's own fp32 and fp64 runs differ by 1e-3 .. 5e-2 in the logits, because a decision
sits within fp32 rounding.  The seed is one where they agree (checked below), so the fixture measures arithmetic.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dgcnn_cls_fixtures.py
"""
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_import as R          # noqa: E402
from weights import fill_state  # noqa: E402

CFG = 'cfgs/finetune_modelnet_transferring_features_1k_smooth.yaml'
PRETRAIN_CFG = 'cfgs/pretrain_PointCAE_clean.yaml'


def _sample(t, n=256):
    flat = t.detach().reshape(-1)
    idx = np.linspace(0, flat.numel() - 1, min(n, flat.numel())).astype(np.int64)
    return flat[idx].numpy(), idx


def _ref_cfg():
    from easydict import EasyDict
    import yaml
    return EasyDict(yaml.safe_load(open(os.path.join(R.REF, CFG)))['model'])


class _InjectedDropout(torch.nn.Module):
    """nn.Dropout(p) with a given keep mask (the generator's draw instead of torch's bernoulli)."""

    def __init__(self, p, keep):
        super().__init__()
        self.p, self.keep = p, keep

    def forward(self, x):
        return x * self.keep.to(x.dtype) / (1 - self.p) if self.training else x


def layout():
    import models.PointCAE_DGCNN as M
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_dgcnn import Point_CAE_DGCNN_FCOnly
    R.seed_all(0)
    ref = M.DGCNN(_ref_cfg())
    keys = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, PRETRAIN_CFG)).model
    pre_cfg.NAME = 'Point_CAE_DGCNN_FCOnly'
    pre = Point_CAE_DGCNN_FCOnly(pre_cfg)
    seen = {}
    orig = ref.load_state_dict

    def capture(sd, strict=True):
        seen['r'] = orig(sd, strict=strict)
        return seen['r']
    ref.load_state_dict = capture
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'ckpt-last.pth')
        torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, path)
        ref.load_model_from_ckpt(path)                 # the reference's own key surgery and load
    out = dict(state_dict=keys, missing_keys=sorted(seen['r'].missing_keys),
               unexpected_keys=sorted(seen['r'].unexpected_keys), pretrain_config=PRETRAIN_CFG,
               pretrain_model='Point_CAE_DGCNN_FCOnly')
    with open(os.path.join(HERE, 'dgcnn_cls_layout.json'), 'w') as f:
        json.dump(out, f, indent=1)


def cls_fixture(name='dgcnn_cls_b4.npz', B=4, seed=12):
    import models.PointCAE_DGCNN as M
    from point_dae_amd.synthetic import shapenet_like_clouds
    R.seed_all(seed)
    ref = fill_state(M.DGCNN(_ref_cfg()), seed).train()
    assert ref.smoothing
    rng = np.random.default_rng(seed)
    pts = shapenet_like_clouds(B, 1024, seed=seed)
    labels = rng.integers(0, ref.cls_dim, B).astype(np.int64)
    keep = rng.random((B, 256)) >= 0.5
    ref.cls_head_finetune[6] = _InjectedDropout(0.5, torch.from_numpy(keep))
    # no discrete decision of the encoder within fp32 rounding: the fp64 run of the same model agrees
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        l64 = ref64(torch.from_numpy(pts).double())
    cap = {}
    ref.dgcnn_encoder.register_forward_hook(lambda m, i, o: cap.update(feature=o))
    logits = ref(torch.from_numpy(pts))
    cond = float((logits.detach().double() - l64).abs().max() / l64.abs().max())
    assert cond <= 1e-5, ('seed %d: the fp32 and fp64 logits differ by %.2e' % (seed, cond))
    loss, acc = ref.get_loss_acc(logits, torch.from_numpy(labels))
    ref.smoothing = False
    with torch.no_grad():
        loss_plain, _ = ref.get_loss_acc(logits, torch.from_numpy(labels))
    ref.smoothing = True
    loss.backward()
    out = dict(pts=pts, labels=labels, keep=keep, seed=np.int64(seed), feature=cap['feature'].detach().numpy(),
               logits=logits.detach().numpy(), fp64_logits_rel=np.float64(cond),
               loss=np.float32(loss.item()), loss_plain=np.float32(loss_plain.item()), acc=np.float32(acc.item()))
    for pname, p in ref.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        key = 'grad/' + pname
        out[key + '/norm'] = np.float64(g.double().norm().item())
        if g.numel() <= 1536:
            out[key + '/full'] = g.clone().numpy()          # (a copy: clip_grad_norm_ below scales .grad in place)
        else:
            out[key + '/sample'], _ = _sample(g)
    out['total_norm'] = np.float32(torch.nn.utils.clip_grad_norm_(ref.parameters(), 10).item())
    for bname, b in ref.named_buffers():          # BatchNorm running statistics after the step
        if b.dtype.is_floating_point:
            out['buf/' + bname] = b.numpy()
    ref.eval()
    with torch.no_grad():
        out['eval_logits'] = ref(torch.from_numpy(pts)).numpy()
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(name, 'fp32 vs fp64 logits %.2e' % cond, 'loss', loss.item(), 'plain', loss_plain.item(), 'acc', acc.item(),
          'size %.0f KB' % (os.path.getsize(os.path.join(HERE, name)) / 1024))


if __name__ == '__main__':
    R.setup()
    layout()
    cls_fixture()
