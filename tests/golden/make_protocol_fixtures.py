"""Generate the fixtures of the frozen-encoder protocols (optimizer.part only_new / diff_lr) from the LIVE reference.

Runs only in the dev container (needs the reference tree, imported read-only via ref_import.py with the native ops
replaced by the CPU oracle; tools/builder.py and tools/runner_finetune.py are imported in place for build_opti_sche and
set_bn_eval).  What is committed is data only:

  protocol_layout.json       the state_dict keys and shapes of the reference's PointTransformerLinearClassification and
                             the missing / unexpected keys of its load_model_from_ckpt for a pretraining checkpoint of
                             this repository; per model (PointTransformer, PointTransformerLinearClassification, DGCNN)
                             and part (only_new, diff_lr) the parameter names, lr and weight_decay of every group
                             build_opti_sche makes; per model the modules set_bn_eval puts in eval mode; the values of
                             the reference YAML the three new configs restate
  protocol_linear_b4.npz     B=4, N=1024, train() + set_bn_eval, drop_path_rate 0, PointTransformerLinearClassification
  protocol_nonlinear_b4.npz  the same for PointTransformer with injected dropout keeps (BN512 eval, BN256 training)
                             each: inputs, labels, logits, loss, acc, every parameter's gradient (full or sampled),
                             clip_grad_norm_'s total norm, the buffers after the step, the parameters (full or sampled)
                             after ONE clipped AdamW step over the reference's only_new groups, taken from the
                             moments of moments.fill_moments at step count moments.STEPS_BEFORE (a first step from
                             zero moments follows the sign of rounding noise wherever a gradient is analytically
                             zero), and the embedder's near-tie decisions (near_ties)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_protocol_fixtures.py
"""
import importlib
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
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_import as R          # noqa: E402
from make_finetune_fixtures import PRETRAIN_CFG, _InjectedDropout, _sample, near_ties  # noqa: E402
from moments import STEPS_BEFORE, fill_moments  # noqa: E402
from weights import fill_state  # noqa: E402

LINEAR_CFG = 'cfgs/finetune_modelnet_linear_classification.yaml'
DGCNN_CFG = 'cfgs/finetune_modelnet_non_linear_classification_officialmodelnet.yaml'
# the three new configs of this repository: the reference YAML each restates and what it changes in it (the reference
# ships the non-linear and diff_lr protocols for other data sets only; both are its ModelNet40 linear-classification /
# transferring-features settings with the model or the part exchanged)
NEW_CONFIGS = {
    'finetune_modelnet_linear_classification.yaml': (LINEAR_CFG, {}),
    'finetune_modelnet_non_linear_classification.yaml': (LINEAR_CFG, {'model.NAME': 'PointTransformer'}),
    'finetune_modelnet_transferring_features_diff_lr.yaml': ('cfgs/finetune_modelnet_transferring_features.yaml',
                                                             {'optimizer.part': 'diff_lr'}),
}


def near_tie_share(fx, B=4, G=64, n=32, widths=(('bn1', 128), ('bn2', 512), ('f1', 256), ('f2', 384))):
    """The share of the embedder's decisions (BatchNorm-ReLU signs and max-pool winners together) a fixture records
    as near-ties."""
    return (sum(len(fx['tie/%s/idx' % key]) for key, _ in widths)
            / sum(B * G * C * (n if key.startswith('bn') else 1) for key, C in widths))


def _yaml(path):
    import yaml
    return yaml.safe_load(open(os.path.join(R.REF, path)))


def _full_cfg(path, **model_overrides):
    from easydict import EasyDict
    cfg = EasyDict(_yaml(path))
    for k, v in model_overrides.items():
        cfg.model[k] = v
    return cfg


def load_reference_tools():
    R.setup()

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    sched = mod('timm.scheduler', CosineLRScheduler=lambda *a, **k: None)
    sys.modules['timm'].scheduler = sched
    mod('thop', profile=None, clever_format=None)
    mod('ptflops', get_model_complexity_info=None)
    mod('torchvision', transforms=mod('torchvision.transforms', Compose=lambda ts: ts))      # (not in this image)
    try:
        import sklearn.svm  # noqa: F401
    except ImportError:
        mod('sklearn', svm=mod('sklearn.svm', SVC=None))
    import models.Point_MAE as M
    import models.PointCAE_DGCNN as D
    sys.modules['models'].build_model_from_cfg = lambda cfg: getattr(D if cfg.NAME == 'DGCNN' else M, cfg.NAME)(cfg)
    sys.modules['datasets'].build_dataset_from_cfg = lambda *a, **k: None
    tools = types.ModuleType('tools')
    tools.__path__ = [os.path.join(R.REF, 'tools')]
    sys.modules['tools'] = tools
    builder = importlib.import_module('tools.builder')
    tools.builder = builder
    try:
        runner = importlib.import_module('tools.runner_finetune')
    except ImportError as e:                     # stub whatever third-party module the runner wants and this image lacks
        raise RuntimeError('tools/runner_finetune.py does not import here: %s' % e)
    return M, D, builder, runner


def _models(M, D):
    return {'PointTransformer': lambda **o: M.PointTransformer(_full_cfg(LINEAR_CFG, **o).model),
            'PointTransformerLinearClassification':
                lambda **o: M.PointTransformerLinearClassification(_full_cfg(LINEAR_CFG, **o).model),
            'DGCNN': lambda **o: D.DGCNN(_full_cfg(DGCNN_CFG, **o).model)}


def _groups(builder, net, cfg_path, part):
    cfg = _full_cfg(cfg_path)
    cfg.optimizer.part = part
    optimizer, _ = builder.build_opti_sche(torch.nn.DataParallel(net), cfg)
    name_of = {id(p): n for n, p in net.named_parameters()}
    return optimizer, [dict(names=[name_of[id(p)] for p in g['params']], lr=g['lr'], weight_decay=g['weight_decay'])
                       for g in optimizer.param_groups]


def layout(M, D, builder, runner):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_transformer import PointCAE_transformer
    R.seed_all(0)
    make = _models(M, D)
    ref = make['PointTransformerLinearClassification']()
    keys = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
    pre = PointCAE_transformer(cfg_from_yaml_file(os.path.join(ROOT, PRETRAIN_CFG)).model)
    seen = {}
    orig = ref.load_state_dict

    def capture(sd, strict=True):
        seen['r'] = orig(sd, strict=strict)
        return seen['r']
    ref.load_state_dict = capture
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'ckpt-last.pth')
        torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, path)
        ref.load_model_from_ckpt(path)
    out = dict(state_dict=keys, missing_keys=sorted(seen['r'].missing_keys),
               unexpected_keys=sorted(seen['r'].unexpected_keys), pretrain_config=PRETRAIN_CFG, groups={}, bn_eval={},
               configs={}, bn_train={})
    for name, ctor in make.items():
        cfg_path = DGCNN_CFG if name == 'DGCNN' else LINEAR_CFG
        out['groups'][name] = {part: _groups(builder, ctor(), cfg_path, part)[1] for part in ('only_new', 'diff_lr')}
        net = ctor().train()
        net.apply(runner.set_bn_eval)
        out['bn_eval'][name] = [n for n, m in net.named_modules()
                                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and not m.training]
        out['bn_train'][name] = [n for n, m in net.named_modules()
                                 if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training]
    for new, (src, changes) in NEW_CONFIGS.items():
        values = _yaml(src)
        for k, v in changes.items():
            node, parts = values, k.split('.')
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = v
        out['configs'][new] = dict(reference=src, changes=changes, values=values)
    with open(os.path.join(HERE, 'protocol_layout.json'), 'w') as f:
        json.dump(out, f, indent=1)


def _keep_or_sample(out, key, t):
    if t.numel() <= 1536:
        out[key + '/full'] = t.detach().clone().numpy()
    else:
        out[key + '/sample'], _ = _sample(t)


def step_fixture(M, D, builder, runner, model, name, B=4, seed=7):
    from point_dae_amd.synthetic import shapenet_like_clouds
    overrides = (('drop_path_rate', 0.0),)
    R.seed_all(seed)
    ref = fill_state(_models(M, D)[model](**dict(overrides)), seed).train()
    ref.apply(runner.set_bn_eval)
    rng = np.random.default_rng(seed)
    pts = shapenet_like_clouds(B, 1024, seed=seed)
    labels = rng.integers(0, ref.cls_dim, B).astype(np.int64)
    out = dict(pts=pts, labels=labels, seed=np.int64(seed), overrides=np.array(repr(list(overrides))))
    head = ref.cls_head_finetune
    if model == 'PointTransformer':
        keep1, keep2 = rng.random((B, 512)) >= 0.5, rng.random((B, 256)) >= 0.5
        head[3] = _InjectedDropout(0.5, torch.from_numpy(keep1)).train()
        head[7] = _InjectedDropout(0.5, torch.from_numpy(keep2)).train()
        out.update(keep1=keep1, keep2=keep2)
        assert not head[1].training and head[5].training
    enc, seen = ref.encoder, {}
    assert not enc.first_conv[1].training and not enc.second_conv[1].training
    hooks = [mod.register_forward_hook(lambda m, i, o, key=key: seen.update({key: o.detach().clone()}))
             for key, mod in (('bn1', enc.first_conv[1]), ('f1', enc.first_conv[3]), ('bn2', enc.second_conv[1]),
                              ('f2', enc.second_conv[3]))]
    before = {k: v.clone() for k, v in ref.state_dict().items()}
    logits = ref(torch.from_numpy(pts))
    for h in hooks:
        h.remove()
    loss, acc = ref.get_loss_acc(logits, torch.from_numpy(labels))
    loss.backward()
    out.update(logits=logits.detach().numpy(), loss=np.float32(loss.item()), acc=np.float32(acc.item()))
    ties = near_ties(seen)
    # the reference alone stays inside the share of decisions the existing fixture (finetune_cls_b4.npz) replays
    bound = near_tie_share(dict(np.load(os.path.join(HERE, 'finetune_cls_b4.npz'))))
    share = near_tie_share(ties)
    print(name, 'seed', seed, 'near-tie share', share, 'bound', bound)
    if share > bound:
        return False
    out.update(ties)
    for pname, p in ref.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out['grad/' + pname + '/norm'] = np.float64(g.double().norm().item())
        _keep_or_sample(out, 'grad/' + pname, g)
    optimizer, groups = _groups(builder, ref, LINEAR_CFG, 'only_new')
    out['total_norm'] = np.float32(torch.nn.utils.clip_grad_norm_(ref.parameters(), 10).item())
    trained = {n for g in groups for n in g['names']}
    for pname, p in ref.named_parameters():
        if pname in trained:
            m, v = fill_moments(pname, tuple(p.shape), seed)
            optimizer.state[p] = dict(step=torch.tensor(float(STEPS_BEFORE)), exp_avg=torch.from_numpy(m),
                                      exp_avg_sq=torch.from_numpy(v))
    optimizer.step()
    assert all(int(optimizer.state[p]['step']) == STEPS_BEFORE + 1 for g in optimizer.param_groups for p in g['params'])
    out['steps_before'] = np.int64(STEPS_BEFORE)
    for pname, p in ref.named_parameters():
        _keep_or_sample(out, 'param/' + pname, p)
        assert pname in trained or torch.equal(p, before[pname]), pname
    for bname, b in ref.named_buffers():
        if b.dtype.is_floating_point:
            out['buf/' + bname] = b.numpy()
    out['trained'] = np.array(json.dumps(sorted(trained)))
    np.savez_compressed(os.path.join(HERE, name), **out)
    return True


def first_seed_inside(tools, model, name, seeds=range(7, 27)):
    """The fixture at the first seed at which the reference's own near-tie shares stay inside the bound."""
    for seed in seeds:
        if step_fixture(*tools, model, name, seed=seed):
            return seed
    raise RuntimeError('%s: no seed in %r keeps the near-tie shares inside the bound' % (name, seeds))


if __name__ == '__main__':
    tools = load_reference_tools()
    layout(*tools)
    first_seed_inside(tools, 'PointTransformerLinearClassification', 'protocol_linear_b4.npz')
    first_seed_inside(tools, 'PointTransformer', 'protocol_nonlinear_b4.npz')
