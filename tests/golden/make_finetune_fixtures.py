"""Generate the fine-tuning fixtures of tests/golden/ from the LIVE reference (models/Point_MAE.py PointTransformer).

Runs only in the dev container (needs the reference tree, imported read-only via ref_import.py with the native ops
replaced by the CPU oracle).  What is committed is data only:

  finetune_layout.json   every state_dict key of the reference's PointTransformer with its shape, and the missing /
                         unexpected keys its load_model_from_ckpt reports (load_state_dict(strict=False)) for a
                         pretraining checkpoint of this repository's PointCAE_transformer
  finetune_cls_b4.npz    B=4, N=1024, train mode, drop_path_rate 0: inputs, labels, the injected dropout keep masks,
                         logits, loss, acc, sampled gradients of every parameter, the clip_grad_norm_ total norm, the
                         BatchNorm running statistics after the step, eval-mode logits of the same clouds, and the
                         patch embedder's near-tie decisions of the training forward (near_ties)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_finetune_fixtures.py
"""
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

CFG = 'cfgs/finetune_modelnet_transferring_features.yaml'
PRETRAIN_CFG = 'cfgs/pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml'


def _sample(t, n=256):
    flat = t.detach().reshape(-1)
    idx = np.linspace(0, flat.numel() - 1, min(n, flat.numel())).astype(np.int64)
    return flat[idx].numpy(), idx


def _ref_cfg(overrides=()):
    from easydict import EasyDict
    import yaml
    cfg = EasyDict(yaml.safe_load(open(os.path.join(R.REF, CFG)))['model'])
    for k, v in overrides:
        cfg[k] = v
    return cfg


class _InjectedDropout(torch.nn.Module):
    """nn.Dropout(p) with a given keep mask (the generator's draw instead of torch's bernoulli)."""

    def __init__(self, p, keep):
        super().__init__()
        self.p, self.keep = p, keep

    def forward(self, x):
        return x * self.keep.to(x.dtype) / (1 - self.p) if self.training else x


def layout():
    import models.Point_MAE as M
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_transformer import PointCAE_transformer
    R.seed_all(0)
    ref = M.PointTransformer(_ref_cfg())
    keys = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, PRETRAIN_CFG)).model
    pre = PointCAE_transformer(pre_cfg)
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
               unexpected_keys=sorted(seen['r'].unexpected_keys), pretrain_config=PRETRAIN_CFG)
    with open(os.path.join(HERE, 'finetune_layout.json'), 'w') as f:
        json.dump(out, f, indent=1)


def near_ties(seen, rel=1e-5):
    """The patch embedder's decisions the reference took within `rel` of its channel's largest |value|: BatchNorm-ReLU
    inputs that close to zero (flat indices into (groups, C, n) and whether the ReLU passed them) and max-pools whose
    best two points are that close (flat indices into (groups, C) and the winner the reference's max took)."""
    out = {}
    for key in ('bn1', 'bn2'):
        v = seen[key]
        near = (v.abs() / v.abs().amax(dim=(0, 2), keepdim=True)).reshape(-1) <= rel
        idx = near.nonzero().reshape(-1)
        out['tie/%s/idx' % key], out['tie/%s/on' % key] = idx.numpy(), (v.reshape(-1)[idx] > 0).numpy()
    for key in ('f1', 'f2'):
        v = seen[key]
        top2 = v.topk(2, dim=2).values
        gap = (top2[..., 0] - top2[..., 1]) / v.abs().amax(dim=(0, 2)).clamp_min(1e-30).view(1, -1)
        idx = (gap.reshape(-1) <= rel).nonzero().reshape(-1)
        out['tie/%s/idx' % key], out['tie/%s/win' % key] = idx.numpy(), v.max(dim=2)[1].reshape(-1)[idx].numpy()
    return out


def cls_fixture(name='finetune_cls_b4.npz', B=4, seed=5):
    import models.Point_MAE as M
    from point_dae_amd.synthetic import shapenet_like_clouds
    overrides = (('drop_path_rate', 0.0),)
    R.seed_all(seed)
    ref = fill_state(M.PointTransformer(_ref_cfg(overrides)), seed).train()
    rng = np.random.default_rng(seed)
    pts = shapenet_like_clouds(B, 1024, seed=seed)
    labels = rng.integers(0, ref.cls_dim, B).astype(np.int64)
    keep1 = rng.random((B, 512)) >= 0.5
    keep2 = rng.random((B, 256)) >= 0.5
    head = ref.cls_head_finetune
    head[3] = _InjectedDropout(0.5, torch.from_numpy(keep1))
    head[7] = _InjectedDropout(0.5, torch.from_numpy(keep2))
    enc, seen = ref.encoder, {}
    hooks = [mod.register_forward_hook(lambda m, i, o, key=key: seen.update({key: o.detach().clone()}))
             for key, mod in (('bn1', enc.first_conv[1]), ('f1', enc.first_conv[3]), ('bn2', enc.second_conv[1]),
                              ('f2', enc.second_conv[3]))]
    logits = ref(torch.from_numpy(pts))
    for h in hooks:
        h.remove()
    loss, acc = ref.get_loss_acc(logits, torch.from_numpy(labels))
    loss.backward()
    out = dict(pts=pts, labels=labels, keep1=keep1, keep2=keep2, seed=np.int64(seed),
               overrides=np.array(repr(list(overrides))), logits=logits.detach().numpy(),
               loss=np.float32(loss.item()), acc=np.float32(acc.item()))
    out.update(near_ties(seen))
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


if __name__ == '__main__':
    R.setup()
    layout()
    cls_fixture()
