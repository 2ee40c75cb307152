"""Generate the fixture of the linear-SVM evaluation protocol from the LIVE reference (models/PointCAE_DGCNN.py
DGCNN_feat, cfgs/finetune_modelnet_svm_classification.yaml).

Runs only in the dev container (needs the reference tree, imported read-only via ref_import.py with the native ops
replaced by the CPU oracle).  What is committed is data only:

  dgcnn_feat_layout.json  every state_dict key of the reference's DGCNN_feat with its shape; the missing / unexpected keys
                          its load_model_from_ckpt reports (load_state_dict(strict=False)) for a checkpoint of this
                          repository's Point_CAE_DGCNN_FCOnly; the values of the reference YAML that
                          cfgs/finetune_modelnet_svm_dgcnn.yaml restates, and what that file changes in them

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_svm_fixtures.py
"""
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_import as R          # noqa: E402

CFG = 'cfgs/finetune_modelnet_svm_classification.yaml'
PRETRAIN_CFG = 'cfgs/pretrain_PointCAE_clean.yaml'
NEW_CONFIG = 'finetune_modelnet_svm_dgcnn.yaml'
CHANGES = {'model.NAME': 'DGCNN_feat'}          # rerun.sh passes it as --model_name DGCNN_feat


def _yaml():
    import yaml
    return yaml.safe_load(open(os.path.join(R.REF, CFG)))


def layout():
    import models.PointCAE_DGCNN as M
    from easydict import EasyDict
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_dgcnn import Point_CAE_DGCNN_FCOnly
    R.seed_all(0)
    ref = M.DGCNN_feat(EasyDict(_yaml()['model']))
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
    values = _yaml()
    for k, v in CHANGES.items():
        node, parts = values, k.split('.')
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    out = dict(state_dict=keys, missing_keys=sorted(seen['r'].missing_keys),
               unexpected_keys=sorted(seen['r'].unexpected_keys), pretrain_config=PRETRAIN_CFG,
               pretrain_model='Point_CAE_DGCNN_FCOnly',
               configs={NEW_CONFIG: dict(reference=CFG, changes=CHANGES, values=values)})
    with open(os.path.join(HERE, 'dgcnn_feat_layout.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print('dgcnn_feat_layout.json: %d keys, missing %r, %d unexpected' % (len(keys), out['missing_keys'],
                                                                         len(out['unexpected_keys'])))


if __name__ == '__main__':
    R.setup()
    layout()
