"""The linear-SVM feature extractors PointNetv2_feat (point_dae_amd/point_cae_pointnetv2.py) and
PointTransformerNoClassTokenSVMFeature (point_dae_amd/point_transformer.py), the checks that need no GPU.

tests/golden/{pointnetv2,transformer}_svmfeat_{a,b}.npz and svmfeat_layout.json hold the LIVE reference's outputs
(make_svmfeat_fixtures.py): per model the fp32 feature as shipped, the feature of the same modules run in fp64 on the
same geometric decisions, those decisions, the state_dict layout, and what the reference's own load_model_from_ckpt
reports for a pretraining checkpoint of this repository.  (i) validates the yardstick of the GPU tests --
tests/svmfeat_restatement.py -- against them; the rest is the host side of the two models."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import svmfeat_restatement as R  # noqa: E402
import weights  # noqa: E402

# model -> (config, fixture prefix, {fixture: fill_state seed}, state_dict entries, parameters)
MODELS_UNDER_TEST = {
    'PointNetv2_feat': ('cfgs/finetune_modelnet_svm_pointnetv2.yaml', 'pointnetv2', {'a': 36, 'b': 22}, 54, 805184),
    'PointTransformerNoClassTokenSVMFeature': ('cfgs/finetune_modelnet_svm_transformer.yaml', 'transformer',
                                               {'a': 5, 'b': 21}, 156, 21825024),
}


def layout(name):
    with open(os.path.join(ROOT, 'tests', 'golden', 'svmfeat_layout.json')) as fh:
        return json.load(fh)[name]


def fixture(prefix, which):
    return np.load(os.path.join(ROOT, 'tests', 'golden', '%s_svmfeat_%s.npz' % (prefix, which)))


def build_model(name):
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401  (registers the models)
    return MODELS.build(cfg_from_yaml_file(os.path.join(ROOT, MODELS_UNDER_TEST[name][0])).model)


@pytest.mark.parametrize('which', ['a', 'b'])
def test_restatement_in_fp64_reproduces_the_live_reference(which):
    """(i) the fp64 restatement of the evaluation-mode set abstraction, fed the recorded FPS / ball-query indices, against
    the reference's fp64 feature: 1e-12 of the largest entry."""
    f = fixture('pointnetv2', which)
    assert int(f['seed']) == MODELS_UNDER_TEST['PointNetv2_feat'][2][which]
    model = weights.fill_state(build_model('PointNetv2_feat'), int(f['seed']))
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    got, _ = R.pointnetv2_feature(torch.from_numpy(f['pts']).double(), sd,
                                  [torch.from_numpy(f['fps_idx%d' % i]) for i in range(2)],
                                  [torch.from_numpy(f['ball_idx%d' % i]) for i in range(2)])
    want = f['feature64']
    err = np.abs(got.numpy() - want).max() / np.abs(want).max()
    print('%s: restatement fp64 vs reference fp64 %.2e; reference fp32 vs fp64 %.2e; %.0f %% of the outputs are 0'
          % (which, err, float(f['dist']), 100 * float(f['zero_fraction'])))
    assert want.shape == (2, 1024) and err <= 1e-12
    assert bool(((got.numpy() == 0) == (want == 0)).all())
    assert 1e-8 < float(f['dist']) <= 1e-6           # the stored fp32 feature is an fp32 evaluation of the same thing


@pytest.mark.parametrize('prefix', ['pointnetv2', 'transformer'])
def test_fixtures_carry_the_reference_fp32_distance(prefix):
    for which in ('a', 'b'):
        f = fixture(prefix, which)
        d = np.abs(f['feature32'].astype(np.float64) - f['feature64']).max() / np.abs(f['feature64']).max()
        assert d == float(f['dist']) and d <= 1e-6


@pytest.mark.parametrize('name', list(MODELS_UNDER_TEST))
def test_state_dict_layout_equals_the_reference(name):
    """(ii)"""
    _, _, _, entries, params = MODELS_UNDER_TEST[name]
    lay = layout(name)
    model = build_model(name)
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == lay['state_dict']
    assert len(sd) == entries
    assert sum(p.numel() for p in model.parameters()) == lay['parameters'] == params
    assert not any(k.startswith(('cls_head_finetune', 'cls_token', 'cls_pos')) for k in sd)


@pytest.mark.parametrize('name', list(MODELS_UNDER_TEST))
def test_pretraining_checkpoint_reports_the_recorded_keys(name, tmp_path):
    """(iii) a checkpoint of this repository's auto-encoder, saved as the pretraining runner saves it: the decoder keys
    unexpected, nothing missing -- exactly what the reference's own load_model_from_ckpt reports."""
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401
    lay = layout(name)
    pre_cfg = cfg_from_yaml_file(os.path.join(ROOT, lay['pretrain_config'])).model
    pre_cfg.NAME = lay['pretrain_model']
    pre = weights.fill_state(MODELS.build(pre_cfg), 3)
    path = str(tmp_path / 'ckpt-last.pth')
    torch.save({'base_model': {'module.' + k: v for k, v in pre.state_dict().items()}}, path)
    model = build_model(name)
    lines = []
    inc = model.load_model_from_ckpt(path, log=lines.append)
    assert sorted(inc.missing_keys) == lay['missing_keys'] == []
    assert sorted(inc.unexpected_keys) == lay['unexpected_keys'] and len(lay['unexpected_keys']) > 0
    src = {k[len('MAE_encoder.'):] if k.startswith('MAE_encoder.') else k: v for k, v in pre.state_dict().items()}
    for k, v in model.state_dict().items():
        assert torch.equal(v, src[k]), k
    text = '\n'.join(lines)
    assert 'unexpected_keys' in text and 'missing_keys' not in text
    lines = []
    assert build_model(name).load_model_from_ckpt(None, log=lines.append) is None and 'scratch' in lines[0]


@pytest.mark.parametrize('name', list(MODELS_UNDER_TEST))
def test_forward_refuses_the_cpu_and_training_mode(name):
    """(iv)"""
    model = build_model(name)
    pts = torch.rand(2, 1024, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        model.eval()(pts)
    with pytest.raises(NotImplementedError, match='evaluation mode only'):
        model.train()(pts)


# The four frozen feature extractors: config, the tail of the training-mode refusal (None: the model has none), and the
# state_dict keys in order, recorded before the classes were put on Classifier.forward_features.
FEATURE_MODELS = {
    'PointNetv2_feat': ('cfgs/finetune_modelnet_svm_pointnetv2.yaml',
                        'the forward-only encoder of the linear-SVM protocol; PointNet++ fine-tuning is not built'),
    'DGCNN_feat': ('cfgs/finetune_modelnet_svm_dgcnn.yaml', None),
    'PointTransformerNoClassTokenSVMFeature': (
        'cfgs/finetune_modelnet_svm_transformer.yaml',
        'the frozen feature extractor of the linear-SVM protocol; PointTransformerNoClassToken fine-tuning is not built'),
    'Point_M2AE_SVMFeature': (
        'cfgs/finetune_modelnet_svm_pointm2ae.yaml',
        'the forward-only encoder of the linear-SVM protocol; training of Point-M2AE and Point_M2AE_Finetune are not built'),
}
FEATURE_KEYS = {
    'PointNetv2_feat': """
        pointnetv2_encoder.sa1.mlps.0.layer0.conv.weight pointnetv2_encoder.sa1.mlps.0.layer0.bn.bn.weight
        pointnetv2_encoder.sa1.mlps.0.layer0.bn.bn.bias pointnetv2_encoder.sa1.mlps.0.layer0.bn.bn.running_mean
        pointnetv2_encoder.sa1.mlps.0.layer0.bn.bn.running_var
        pointnetv2_encoder.sa1.mlps.0.layer0.bn.bn.num_batches_tracked pointnetv2_encoder.sa1.mlps.0.layer1.conv.weight
        pointnetv2_encoder.sa1.mlps.0.layer1.bn.bn.weight pointnetv2_encoder.sa1.mlps.0.layer1.bn.bn.bias
        pointnetv2_encoder.sa1.mlps.0.layer1.bn.bn.running_mean pointnetv2_encoder.sa1.mlps.0.layer1.bn.bn.running_var
        pointnetv2_encoder.sa1.mlps.0.layer1.bn.bn.num_batches_tracked pointnetv2_encoder.sa1.mlps.0.layer2.conv.weight
        pointnetv2_encoder.sa1.mlps.0.layer2.bn.bn.weight pointnetv2_encoder.sa1.mlps.0.layer2.bn.bn.bias
        pointnetv2_encoder.sa1.mlps.0.layer2.bn.bn.running_mean pointnetv2_encoder.sa1.mlps.0.layer2.bn.bn.running_var
        pointnetv2_encoder.sa1.mlps.0.layer2.bn.bn.num_batches_tracked pointnetv2_encoder.sa2.mlps.0.layer0.conv.weight
        pointnetv2_encoder.sa2.mlps.0.layer0.bn.bn.weight pointnetv2_encoder.sa2.mlps.0.layer0.bn.bn.bias
        pointnetv2_encoder.sa2.mlps.0.layer0.bn.bn.running_mean pointnetv2_encoder.sa2.mlps.0.layer0.bn.bn.running_var
        pointnetv2_encoder.sa2.mlps.0.layer0.bn.bn.num_batches_tracked pointnetv2_encoder.sa2.mlps.0.layer1.conv.weight
        pointnetv2_encoder.sa2.mlps.0.layer1.bn.bn.weight pointnetv2_encoder.sa2.mlps.0.layer1.bn.bn.bias
        pointnetv2_encoder.sa2.mlps.0.layer1.bn.bn.running_mean pointnetv2_encoder.sa2.mlps.0.layer1.bn.bn.running_var
        pointnetv2_encoder.sa2.mlps.0.layer1.bn.bn.num_batches_tracked pointnetv2_encoder.sa2.mlps.0.layer2.conv.weight
        pointnetv2_encoder.sa2.mlps.0.layer2.bn.bn.weight pointnetv2_encoder.sa2.mlps.0.layer2.bn.bn.bias
        pointnetv2_encoder.sa2.mlps.0.layer2.bn.bn.running_mean pointnetv2_encoder.sa2.mlps.0.layer2.bn.bn.running_var
        pointnetv2_encoder.sa2.mlps.0.layer2.bn.bn.num_batches_tracked pointnetv2_encoder.sa3.mlps.0.layer0.conv.weight
        pointnetv2_encoder.sa3.mlps.0.layer0.bn.bn.weight pointnetv2_encoder.sa3.mlps.0.layer0.bn.bn.bias
        pointnetv2_encoder.sa3.mlps.0.layer0.bn.bn.running_mean pointnetv2_encoder.sa3.mlps.0.layer0.bn.bn.running_var
        pointnetv2_encoder.sa3.mlps.0.layer0.bn.bn.num_batches_tracked pointnetv2_encoder.sa3.mlps.0.layer1.conv.weight
        pointnetv2_encoder.sa3.mlps.0.layer1.bn.bn.weight pointnetv2_encoder.sa3.mlps.0.layer1.bn.bn.bias
        pointnetv2_encoder.sa3.mlps.0.layer1.bn.bn.running_mean pointnetv2_encoder.sa3.mlps.0.layer1.bn.bn.running_var
        pointnetv2_encoder.sa3.mlps.0.layer1.bn.bn.num_batches_tracked pointnetv2_encoder.sa3.mlps.0.layer2.conv.weight
        pointnetv2_encoder.sa3.mlps.0.layer2.bn.bn.weight pointnetv2_encoder.sa3.mlps.0.layer2.bn.bn.bias
        pointnetv2_encoder.sa3.mlps.0.layer2.bn.bn.running_mean pointnetv2_encoder.sa3.mlps.0.layer2.bn.bn.running_var
        pointnetv2_encoder.sa3.mlps.0.layer2.bn.bn.num_batches_tracked
        """,
    'DGCNN_feat': """
        dgcnn_encoder.bn1.weight dgcnn_encoder.bn1.bias dgcnn_encoder.bn1.running_mean dgcnn_encoder.bn1.running_var
        dgcnn_encoder.bn1.num_batches_tracked dgcnn_encoder.bn2.weight dgcnn_encoder.bn2.bias
        dgcnn_encoder.bn2.running_mean dgcnn_encoder.bn2.running_var dgcnn_encoder.bn2.num_batches_tracked
        dgcnn_encoder.bn3.weight dgcnn_encoder.bn3.bias dgcnn_encoder.bn3.running_mean dgcnn_encoder.bn3.running_var
        dgcnn_encoder.bn3.num_batches_tracked dgcnn_encoder.bn4.weight dgcnn_encoder.bn4.bias
        dgcnn_encoder.bn4.running_mean dgcnn_encoder.bn4.running_var dgcnn_encoder.bn4.num_batches_tracked
        dgcnn_encoder.bn5.weight dgcnn_encoder.bn5.bias dgcnn_encoder.bn5.running_mean dgcnn_encoder.bn5.running_var
        dgcnn_encoder.bn5.num_batches_tracked dgcnn_encoder.conv1.0.weight dgcnn_encoder.conv1.1.weight
        dgcnn_encoder.conv1.1.bias dgcnn_encoder.conv1.1.running_mean dgcnn_encoder.conv1.1.running_var
        dgcnn_encoder.conv1.1.num_batches_tracked dgcnn_encoder.conv2.0.weight dgcnn_encoder.conv2.1.weight
        dgcnn_encoder.conv2.1.bias dgcnn_encoder.conv2.1.running_mean dgcnn_encoder.conv2.1.running_var
        dgcnn_encoder.conv2.1.num_batches_tracked dgcnn_encoder.conv3.0.weight dgcnn_encoder.conv3.1.weight
        dgcnn_encoder.conv3.1.bias dgcnn_encoder.conv3.1.running_mean dgcnn_encoder.conv3.1.running_var
        dgcnn_encoder.conv3.1.num_batches_tracked dgcnn_encoder.conv4.0.weight dgcnn_encoder.conv4.1.weight
        dgcnn_encoder.conv4.1.bias dgcnn_encoder.conv4.1.running_mean dgcnn_encoder.conv4.1.running_var
        dgcnn_encoder.conv4.1.num_batches_tracked dgcnn_encoder.conv5.0.weight dgcnn_encoder.conv5.1.weight
        dgcnn_encoder.conv5.1.bias dgcnn_encoder.conv5.1.running_mean dgcnn_encoder.conv5.1.running_var
        dgcnn_encoder.conv5.1.num_batches_tracked
        """,
    'PointTransformerNoClassTokenSVMFeature': """
        encoder.first_conv.0.weight encoder.first_conv.0.bias encoder.first_conv.1.weight encoder.first_conv.1.bias
        encoder.first_conv.1.running_mean encoder.first_conv.1.running_var encoder.first_conv.1.num_batches_tracked
        encoder.first_conv.3.weight encoder.first_conv.3.bias encoder.second_conv.0.weight encoder.second_conv.0.bias
        encoder.second_conv.1.weight encoder.second_conv.1.bias encoder.second_conv.1.running_mean
        encoder.second_conv.1.running_var encoder.second_conv.1.num_batches_tracked encoder.second_conv.3.weight
        encoder.second_conv.3.bias pos_embed.0.weight pos_embed.0.bias pos_embed.2.weight pos_embed.2.bias
        blocks.blocks.0.norm1.weight blocks.blocks.0.norm1.bias blocks.blocks.0.norm2.weight blocks.blocks.0.norm2.bias
        blocks.blocks.0.mlp.fc1.weight blocks.blocks.0.mlp.fc1.bias blocks.blocks.0.mlp.fc2.weight
        blocks.blocks.0.mlp.fc2.bias blocks.blocks.0.attn.qkv.weight blocks.blocks.0.attn.proj.weight
        blocks.blocks.0.attn.proj.bias blocks.blocks.1.norm1.weight blocks.blocks.1.norm1.bias
        blocks.blocks.1.norm2.weight blocks.blocks.1.norm2.bias blocks.blocks.1.mlp.fc1.weight
        blocks.blocks.1.mlp.fc1.bias blocks.blocks.1.mlp.fc2.weight blocks.blocks.1.mlp.fc2.bias
        blocks.blocks.1.attn.qkv.weight blocks.blocks.1.attn.proj.weight blocks.blocks.1.attn.proj.bias
        blocks.blocks.2.norm1.weight blocks.blocks.2.norm1.bias blocks.blocks.2.norm2.weight blocks.blocks.2.norm2.bias
        blocks.blocks.2.mlp.fc1.weight blocks.blocks.2.mlp.fc1.bias blocks.blocks.2.mlp.fc2.weight
        blocks.blocks.2.mlp.fc2.bias blocks.blocks.2.attn.qkv.weight blocks.blocks.2.attn.proj.weight
        blocks.blocks.2.attn.proj.bias blocks.blocks.3.norm1.weight blocks.blocks.3.norm1.bias
        blocks.blocks.3.norm2.weight blocks.blocks.3.norm2.bias blocks.blocks.3.mlp.fc1.weight
        blocks.blocks.3.mlp.fc1.bias blocks.blocks.3.mlp.fc2.weight blocks.blocks.3.mlp.fc2.bias
        blocks.blocks.3.attn.qkv.weight blocks.blocks.3.attn.proj.weight blocks.blocks.3.attn.proj.bias
        blocks.blocks.4.norm1.weight blocks.blocks.4.norm1.bias blocks.blocks.4.norm2.weight blocks.blocks.4.norm2.bias
        blocks.blocks.4.mlp.fc1.weight blocks.blocks.4.mlp.fc1.bias blocks.blocks.4.mlp.fc2.weight
        blocks.blocks.4.mlp.fc2.bias blocks.blocks.4.attn.qkv.weight blocks.blocks.4.attn.proj.weight
        blocks.blocks.4.attn.proj.bias blocks.blocks.5.norm1.weight blocks.blocks.5.norm1.bias
        blocks.blocks.5.norm2.weight blocks.blocks.5.norm2.bias blocks.blocks.5.mlp.fc1.weight
        blocks.blocks.5.mlp.fc1.bias blocks.blocks.5.mlp.fc2.weight blocks.blocks.5.mlp.fc2.bias
        blocks.blocks.5.attn.qkv.weight blocks.blocks.5.attn.proj.weight blocks.blocks.5.attn.proj.bias
        blocks.blocks.6.norm1.weight blocks.blocks.6.norm1.bias blocks.blocks.6.norm2.weight blocks.blocks.6.norm2.bias
        blocks.blocks.6.mlp.fc1.weight blocks.blocks.6.mlp.fc1.bias blocks.blocks.6.mlp.fc2.weight
        blocks.blocks.6.mlp.fc2.bias blocks.blocks.6.attn.qkv.weight blocks.blocks.6.attn.proj.weight
        blocks.blocks.6.attn.proj.bias blocks.blocks.7.norm1.weight blocks.blocks.7.norm1.bias
        blocks.blocks.7.norm2.weight blocks.blocks.7.norm2.bias blocks.blocks.7.mlp.fc1.weight
        blocks.blocks.7.mlp.fc1.bias blocks.blocks.7.mlp.fc2.weight blocks.blocks.7.mlp.fc2.bias
        blocks.blocks.7.attn.qkv.weight blocks.blocks.7.attn.proj.weight blocks.blocks.7.attn.proj.bias
        blocks.blocks.8.norm1.weight blocks.blocks.8.norm1.bias blocks.blocks.8.norm2.weight blocks.blocks.8.norm2.bias
        blocks.blocks.8.mlp.fc1.weight blocks.blocks.8.mlp.fc1.bias blocks.blocks.8.mlp.fc2.weight
        blocks.blocks.8.mlp.fc2.bias blocks.blocks.8.attn.qkv.weight blocks.blocks.8.attn.proj.weight
        blocks.blocks.8.attn.proj.bias blocks.blocks.9.norm1.weight blocks.blocks.9.norm1.bias
        blocks.blocks.9.norm2.weight blocks.blocks.9.norm2.bias blocks.blocks.9.mlp.fc1.weight
        blocks.blocks.9.mlp.fc1.bias blocks.blocks.9.mlp.fc2.weight blocks.blocks.9.mlp.fc2.bias
        blocks.blocks.9.attn.qkv.weight blocks.blocks.9.attn.proj.weight blocks.blocks.9.attn.proj.bias
        blocks.blocks.10.norm1.weight blocks.blocks.10.norm1.bias blocks.blocks.10.norm2.weight
        blocks.blocks.10.norm2.bias blocks.blocks.10.mlp.fc1.weight blocks.blocks.10.mlp.fc1.bias
        blocks.blocks.10.mlp.fc2.weight blocks.blocks.10.mlp.fc2.bias blocks.blocks.10.attn.qkv.weight
        blocks.blocks.10.attn.proj.weight blocks.blocks.10.attn.proj.bias blocks.blocks.11.norm1.weight
        blocks.blocks.11.norm1.bias blocks.blocks.11.norm2.weight blocks.blocks.11.norm2.bias
        blocks.blocks.11.mlp.fc1.weight blocks.blocks.11.mlp.fc1.bias blocks.blocks.11.mlp.fc2.weight
        blocks.blocks.11.mlp.fc2.bias blocks.blocks.11.attn.qkv.weight blocks.blocks.11.attn.proj.weight
        blocks.blocks.11.attn.proj.bias norm.weight norm.bias
        """,
    'Point_M2AE_SVMFeature': """
        h_encoder.token_embed.0.first_conv.0.weight h_encoder.token_embed.0.first_conv.0.bias
        h_encoder.token_embed.0.first_conv.1.weight h_encoder.token_embed.0.first_conv.1.bias
        h_encoder.token_embed.0.first_conv.1.running_mean h_encoder.token_embed.0.first_conv.1.running_var
        h_encoder.token_embed.0.first_conv.1.num_batches_tracked h_encoder.token_embed.0.first_conv.3.weight
        h_encoder.token_embed.0.first_conv.3.bias h_encoder.token_embed.0.second_conv.0.weight
        h_encoder.token_embed.0.second_conv.0.bias h_encoder.token_embed.0.second_conv.1.weight
        h_encoder.token_embed.0.second_conv.1.bias h_encoder.token_embed.0.second_conv.1.running_mean
        h_encoder.token_embed.0.second_conv.1.running_var h_encoder.token_embed.0.second_conv.1.num_batches_tracked
        h_encoder.token_embed.0.second_conv.3.weight h_encoder.token_embed.0.second_conv.3.bias
        h_encoder.token_embed.1.first_conv.0.weight h_encoder.token_embed.1.first_conv.0.bias
        h_encoder.token_embed.1.first_conv.1.weight h_encoder.token_embed.1.first_conv.1.bias
        h_encoder.token_embed.1.first_conv.1.running_mean h_encoder.token_embed.1.first_conv.1.running_var
        h_encoder.token_embed.1.first_conv.1.num_batches_tracked h_encoder.token_embed.1.first_conv.3.weight
        h_encoder.token_embed.1.first_conv.3.bias h_encoder.token_embed.1.second_conv.0.weight
        h_encoder.token_embed.1.second_conv.0.bias h_encoder.token_embed.1.second_conv.1.weight
        h_encoder.token_embed.1.second_conv.1.bias h_encoder.token_embed.1.second_conv.1.running_mean
        h_encoder.token_embed.1.second_conv.1.running_var h_encoder.token_embed.1.second_conv.1.num_batches_tracked
        h_encoder.token_embed.1.second_conv.3.weight h_encoder.token_embed.1.second_conv.3.bias
        h_encoder.token_embed.2.first_conv.0.weight h_encoder.token_embed.2.first_conv.0.bias
        h_encoder.token_embed.2.first_conv.1.weight h_encoder.token_embed.2.first_conv.1.bias
        h_encoder.token_embed.2.first_conv.1.running_mean h_encoder.token_embed.2.first_conv.1.running_var
        h_encoder.token_embed.2.first_conv.1.num_batches_tracked h_encoder.token_embed.2.first_conv.3.weight
        h_encoder.token_embed.2.first_conv.3.bias h_encoder.token_embed.2.second_conv.0.weight
        h_encoder.token_embed.2.second_conv.0.bias h_encoder.token_embed.2.second_conv.1.weight
        h_encoder.token_embed.2.second_conv.1.bias h_encoder.token_embed.2.second_conv.1.running_mean
        h_encoder.token_embed.2.second_conv.1.running_var h_encoder.token_embed.2.second_conv.1.num_batches_tracked
        h_encoder.token_embed.2.second_conv.3.weight h_encoder.token_embed.2.second_conv.3.bias
        h_encoder.encoder_pos_embeds.0.0.weight h_encoder.encoder_pos_embeds.0.0.bias
        h_encoder.encoder_pos_embeds.0.2.weight h_encoder.encoder_pos_embeds.0.2.bias
        h_encoder.encoder_pos_embeds.1.0.weight h_encoder.encoder_pos_embeds.1.0.bias
        h_encoder.encoder_pos_embeds.1.2.weight h_encoder.encoder_pos_embeds.1.2.bias
        h_encoder.encoder_pos_embeds.2.0.weight h_encoder.encoder_pos_embeds.2.0.bias
        h_encoder.encoder_pos_embeds.2.2.weight h_encoder.encoder_pos_embeds.2.2.bias
        h_encoder.encoder_blocks.0.blocks.0.norm1.weight h_encoder.encoder_blocks.0.blocks.0.norm1.bias
        h_encoder.encoder_blocks.0.blocks.0.norm2.weight h_encoder.encoder_blocks.0.blocks.0.norm2.bias
        h_encoder.encoder_blocks.0.blocks.0.mlp.fc1.weight h_encoder.encoder_blocks.0.blocks.0.mlp.fc1.bias
        h_encoder.encoder_blocks.0.blocks.0.mlp.fc2.weight h_encoder.encoder_blocks.0.blocks.0.mlp.fc2.bias
        h_encoder.encoder_blocks.0.blocks.0.attn.qkv.weight h_encoder.encoder_blocks.0.blocks.0.attn.proj.weight
        h_encoder.encoder_blocks.0.blocks.0.attn.proj.bias h_encoder.encoder_blocks.0.blocks.1.norm1.weight
        h_encoder.encoder_blocks.0.blocks.1.norm1.bias h_encoder.encoder_blocks.0.blocks.1.norm2.weight
        h_encoder.encoder_blocks.0.blocks.1.norm2.bias h_encoder.encoder_blocks.0.blocks.1.mlp.fc1.weight
        h_encoder.encoder_blocks.0.blocks.1.mlp.fc1.bias h_encoder.encoder_blocks.0.blocks.1.mlp.fc2.weight
        h_encoder.encoder_blocks.0.blocks.1.mlp.fc2.bias h_encoder.encoder_blocks.0.blocks.1.attn.qkv.weight
        h_encoder.encoder_blocks.0.blocks.1.attn.proj.weight h_encoder.encoder_blocks.0.blocks.1.attn.proj.bias
        h_encoder.encoder_blocks.0.blocks.2.norm1.weight h_encoder.encoder_blocks.0.blocks.2.norm1.bias
        h_encoder.encoder_blocks.0.blocks.2.norm2.weight h_encoder.encoder_blocks.0.blocks.2.norm2.bias
        h_encoder.encoder_blocks.0.blocks.2.mlp.fc1.weight h_encoder.encoder_blocks.0.blocks.2.mlp.fc1.bias
        h_encoder.encoder_blocks.0.blocks.2.mlp.fc2.weight h_encoder.encoder_blocks.0.blocks.2.mlp.fc2.bias
        h_encoder.encoder_blocks.0.blocks.2.attn.qkv.weight h_encoder.encoder_blocks.0.blocks.2.attn.proj.weight
        h_encoder.encoder_blocks.0.blocks.2.attn.proj.bias h_encoder.encoder_blocks.0.blocks.3.norm1.weight
        h_encoder.encoder_blocks.0.blocks.3.norm1.bias h_encoder.encoder_blocks.0.blocks.3.norm2.weight
        h_encoder.encoder_blocks.0.blocks.3.norm2.bias h_encoder.encoder_blocks.0.blocks.3.mlp.fc1.weight
        h_encoder.encoder_blocks.0.blocks.3.mlp.fc1.bias h_encoder.encoder_blocks.0.blocks.3.mlp.fc2.weight
        h_encoder.encoder_blocks.0.blocks.3.mlp.fc2.bias h_encoder.encoder_blocks.0.blocks.3.attn.qkv.weight
        h_encoder.encoder_blocks.0.blocks.3.attn.proj.weight h_encoder.encoder_blocks.0.blocks.3.attn.proj.bias
        h_encoder.encoder_blocks.0.blocks.4.norm1.weight h_encoder.encoder_blocks.0.blocks.4.norm1.bias
        h_encoder.encoder_blocks.0.blocks.4.norm2.weight h_encoder.encoder_blocks.0.blocks.4.norm2.bias
        h_encoder.encoder_blocks.0.blocks.4.mlp.fc1.weight h_encoder.encoder_blocks.0.blocks.4.mlp.fc1.bias
        h_encoder.encoder_blocks.0.blocks.4.mlp.fc2.weight h_encoder.encoder_blocks.0.blocks.4.mlp.fc2.bias
        h_encoder.encoder_blocks.0.blocks.4.attn.qkv.weight h_encoder.encoder_blocks.0.blocks.4.attn.proj.weight
        h_encoder.encoder_blocks.0.blocks.4.attn.proj.bias h_encoder.encoder_blocks.1.blocks.0.norm1.weight
        h_encoder.encoder_blocks.1.blocks.0.norm1.bias h_encoder.encoder_blocks.1.blocks.0.norm2.weight
        h_encoder.encoder_blocks.1.blocks.0.norm2.bias h_encoder.encoder_blocks.1.blocks.0.mlp.fc1.weight
        h_encoder.encoder_blocks.1.blocks.0.mlp.fc1.bias h_encoder.encoder_blocks.1.blocks.0.mlp.fc2.weight
        h_encoder.encoder_blocks.1.blocks.0.mlp.fc2.bias h_encoder.encoder_blocks.1.blocks.0.attn.qkv.weight
        h_encoder.encoder_blocks.1.blocks.0.attn.proj.weight h_encoder.encoder_blocks.1.blocks.0.attn.proj.bias
        h_encoder.encoder_blocks.1.blocks.1.norm1.weight h_encoder.encoder_blocks.1.blocks.1.norm1.bias
        h_encoder.encoder_blocks.1.blocks.1.norm2.weight h_encoder.encoder_blocks.1.blocks.1.norm2.bias
        h_encoder.encoder_blocks.1.blocks.1.mlp.fc1.weight h_encoder.encoder_blocks.1.blocks.1.mlp.fc1.bias
        h_encoder.encoder_blocks.1.blocks.1.mlp.fc2.weight h_encoder.encoder_blocks.1.blocks.1.mlp.fc2.bias
        h_encoder.encoder_blocks.1.blocks.1.attn.qkv.weight h_encoder.encoder_blocks.1.blocks.1.attn.proj.weight
        h_encoder.encoder_blocks.1.blocks.1.attn.proj.bias h_encoder.encoder_blocks.1.blocks.2.norm1.weight
        h_encoder.encoder_blocks.1.blocks.2.norm1.bias h_encoder.encoder_blocks.1.blocks.2.norm2.weight
        h_encoder.encoder_blocks.1.blocks.2.norm2.bias h_encoder.encoder_blocks.1.blocks.2.mlp.fc1.weight
        h_encoder.encoder_blocks.1.blocks.2.mlp.fc1.bias h_encoder.encoder_blocks.1.blocks.2.mlp.fc2.weight
        h_encoder.encoder_blocks.1.blocks.2.mlp.fc2.bias h_encoder.encoder_blocks.1.blocks.2.attn.qkv.weight
        h_encoder.encoder_blocks.1.blocks.2.attn.proj.weight h_encoder.encoder_blocks.1.blocks.2.attn.proj.bias
        h_encoder.encoder_blocks.1.blocks.3.norm1.weight h_encoder.encoder_blocks.1.blocks.3.norm1.bias
        h_encoder.encoder_blocks.1.blocks.3.norm2.weight h_encoder.encoder_blocks.1.blocks.3.norm2.bias
        h_encoder.encoder_blocks.1.blocks.3.mlp.fc1.weight h_encoder.encoder_blocks.1.blocks.3.mlp.fc1.bias
        h_encoder.encoder_blocks.1.blocks.3.mlp.fc2.weight h_encoder.encoder_blocks.1.blocks.3.mlp.fc2.bias
        h_encoder.encoder_blocks.1.blocks.3.attn.qkv.weight h_encoder.encoder_blocks.1.blocks.3.attn.proj.weight
        h_encoder.encoder_blocks.1.blocks.3.attn.proj.bias h_encoder.encoder_blocks.1.blocks.4.norm1.weight
        h_encoder.encoder_blocks.1.blocks.4.norm1.bias h_encoder.encoder_blocks.1.blocks.4.norm2.weight
        h_encoder.encoder_blocks.1.blocks.4.norm2.bias h_encoder.encoder_blocks.1.blocks.4.mlp.fc1.weight
        h_encoder.encoder_blocks.1.blocks.4.mlp.fc1.bias h_encoder.encoder_blocks.1.blocks.4.mlp.fc2.weight
        h_encoder.encoder_blocks.1.blocks.4.mlp.fc2.bias h_encoder.encoder_blocks.1.blocks.4.attn.qkv.weight
        h_encoder.encoder_blocks.1.blocks.4.attn.proj.weight h_encoder.encoder_blocks.1.blocks.4.attn.proj.bias
        h_encoder.encoder_blocks.2.blocks.0.norm1.weight h_encoder.encoder_blocks.2.blocks.0.norm1.bias
        h_encoder.encoder_blocks.2.blocks.0.norm2.weight h_encoder.encoder_blocks.2.blocks.0.norm2.bias
        h_encoder.encoder_blocks.2.blocks.0.mlp.fc1.weight h_encoder.encoder_blocks.2.blocks.0.mlp.fc1.bias
        h_encoder.encoder_blocks.2.blocks.0.mlp.fc2.weight h_encoder.encoder_blocks.2.blocks.0.mlp.fc2.bias
        h_encoder.encoder_blocks.2.blocks.0.attn.qkv.weight h_encoder.encoder_blocks.2.blocks.0.attn.proj.weight
        h_encoder.encoder_blocks.2.blocks.0.attn.proj.bias h_encoder.encoder_blocks.2.blocks.1.norm1.weight
        h_encoder.encoder_blocks.2.blocks.1.norm1.bias h_encoder.encoder_blocks.2.blocks.1.norm2.weight
        h_encoder.encoder_blocks.2.blocks.1.norm2.bias h_encoder.encoder_blocks.2.blocks.1.mlp.fc1.weight
        h_encoder.encoder_blocks.2.blocks.1.mlp.fc1.bias h_encoder.encoder_blocks.2.blocks.1.mlp.fc2.weight
        h_encoder.encoder_blocks.2.blocks.1.mlp.fc2.bias h_encoder.encoder_blocks.2.blocks.1.attn.qkv.weight
        h_encoder.encoder_blocks.2.blocks.1.attn.proj.weight h_encoder.encoder_blocks.2.blocks.1.attn.proj.bias
        h_encoder.encoder_blocks.2.blocks.2.norm1.weight h_encoder.encoder_blocks.2.blocks.2.norm1.bias
        h_encoder.encoder_blocks.2.blocks.2.norm2.weight h_encoder.encoder_blocks.2.blocks.2.norm2.bias
        h_encoder.encoder_blocks.2.blocks.2.mlp.fc1.weight h_encoder.encoder_blocks.2.blocks.2.mlp.fc1.bias
        h_encoder.encoder_blocks.2.blocks.2.mlp.fc2.weight h_encoder.encoder_blocks.2.blocks.2.mlp.fc2.bias
        h_encoder.encoder_blocks.2.blocks.2.attn.qkv.weight h_encoder.encoder_blocks.2.blocks.2.attn.proj.weight
        h_encoder.encoder_blocks.2.blocks.2.attn.proj.bias h_encoder.encoder_blocks.2.blocks.3.norm1.weight
        h_encoder.encoder_blocks.2.blocks.3.norm1.bias h_encoder.encoder_blocks.2.blocks.3.norm2.weight
        h_encoder.encoder_blocks.2.blocks.3.norm2.bias h_encoder.encoder_blocks.2.blocks.3.mlp.fc1.weight
        h_encoder.encoder_blocks.2.blocks.3.mlp.fc1.bias h_encoder.encoder_blocks.2.blocks.3.mlp.fc2.weight
        h_encoder.encoder_blocks.2.blocks.3.mlp.fc2.bias h_encoder.encoder_blocks.2.blocks.3.attn.qkv.weight
        h_encoder.encoder_blocks.2.blocks.3.attn.proj.weight h_encoder.encoder_blocks.2.blocks.3.attn.proj.bias
        h_encoder.encoder_blocks.2.blocks.4.norm1.weight h_encoder.encoder_blocks.2.blocks.4.norm1.bias
        h_encoder.encoder_blocks.2.blocks.4.norm2.weight h_encoder.encoder_blocks.2.blocks.4.norm2.bias
        h_encoder.encoder_blocks.2.blocks.4.mlp.fc1.weight h_encoder.encoder_blocks.2.blocks.4.mlp.fc1.bias
        h_encoder.encoder_blocks.2.blocks.4.mlp.fc2.weight h_encoder.encoder_blocks.2.blocks.4.mlp.fc2.bias
        h_encoder.encoder_blocks.2.blocks.4.attn.qkv.weight h_encoder.encoder_blocks.2.blocks.4.attn.proj.weight
        h_encoder.encoder_blocks.2.blocks.4.attn.proj.bias h_encoder.encoder_norms.0.weight
        h_encoder.encoder_norms.0.bias h_encoder.encoder_norms.1.weight h_encoder.encoder_norms.1.bias
        h_encoder.encoder_norms.2.weight h_encoder.encoder_norms.2.bias
        """,
}


@pytest.mark.parametrize('name', list(FEATURE_MODELS))
def test_feature_guard_texts_and_state_dict_keys(name):
    """The guard in front of every feature extractor's trunk: the exact texts of the CPU-tensor error and of the
    training-mode refusal (DGCNN_feat has none: it answers a CPU tensor in training mode as in evaluation mode), and the
    state_dict keys, in order."""
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    from point_dae_amd import builder  # noqa: F401
    path, tail = FEATURE_MODELS[name]
    model = MODELS.build(cfg_from_yaml_file(os.path.join(ROOT, path)).model)
    assert list(model.state_dict().keys()) == FEATURE_KEYS[name].split()
    pts = torch.rand(2, 64, 3)
    cpu = name + ': points must be on the GPU (there is no CPU path)'
    with pytest.raises(RuntimeError) as err:
        model.eval()(pts)
    assert type(err.value) is RuntimeError and str(err.value) == cpu
    with pytest.raises(RuntimeError if tail is None else NotImplementedError) as err:
        model.train()(pts)
    assert str(err.value) == (cpu if tail is None else name + ': evaluation mode only -- ' + tail)
    assert type(err.value) is (RuntimeError if tail is None else NotImplementedError)


def test_the_encoder_switch_is_off_by_default_and_on_in_the_feature_model(monkeypatch):
    """(v) only PointNetv2_feat turns the fused evaluation path on; PDAE_SA_EVAL takes hip or layers."""
    from point_dae_amd import sa_eval_ops
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.point_cae_pointnetv2 import Point_CAE_PointNetv2, PointNetv2_encoder, PointnetSAModule
    enc = build_model('PointNetv2_feat').pointnetv2_encoder
    assert all(m.fused_eval for m in (enc.sa1, enc.sa2, enc.sa3))
    assert not any(m.fused_eval for m in PointNetv2_encoder().modules() if isinstance(m, PointnetSAModule))
    ae = Point_CAE_PointNetv2(cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'pretrain_PointCAE_clean.yaml')).model)
    assert not any(m.fused_eval for m in ae.modules() if isinstance(m, PointnetSAModule))
    monkeypatch.delenv('PDAE_SA_EVAL', raising=False)
    assert sa_eval_ops.mode() == 'hip'
    monkeypatch.setenv('PDAE_SA_EVAL', 'layers')
    assert sa_eval_ops.mode() == 'layers'
    monkeypatch.setenv('PDAE_SA_EVAL', 'eager')
    with pytest.raises(ValueError, match='PDAE_SA_EVAL'):
        sa_eval_ops.mode()


def test_loss_smoothing_follows_the_reference():
    """(vi) PointNetv2_feat.get_loss_acc smooths with eps 0.3 under smoothloss (PointCAE_pointnetv2.py:950-957); the
    Transformer's feature model has the plain cross-entropy (Point_MAE.py:1021-1025)."""
    from point_dae_amd.classifier import Classifier
    model = build_model('PointNetv2_feat')
    assert isinstance(model, Classifier) and model.smoothing and model.smooth_eps == 0.3
    model.smoothing = False
    assert model.smooth_eps is None
    tr = build_model('PointTransformerNoClassTokenSVMFeature')
    assert isinstance(tr, Classifier) and tr.smooth_eps is None and not tr.input_grad_supported
    assert tr.late_grad_prefixes == ()


@pytest.mark.parametrize('name', list(MODELS_UNDER_TEST))
def test_config_restates_the_reference_yaml(name, tmp_path, monkeypatch):
    """(vii) the new YAML carries the reference file's values with model.NAME set, and parses through the CLI."""
    from point_dae_amd import parser
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.registry import MODELS
    path = MODELS_UNDER_TEST[name][0]
    rec = layout(name)['configs'][os.path.basename(path)]
    assert rec['changes'] == {'model.NAME': name}
    cfg = cfg_from_yaml_file(os.path.join(ROOT, path))
    want = rec['values']
    assert dict(cfg.model) == want['model'] and cfg.model.NAME == name and name in MODELS
    for key in ('npoints', 'total_bs', 'step_per_update', 'max_epoch', 'grad_norm_clip'):
        assert cfg[key] == want[key], key
    assert (cfg.npoints, cfg.total_bs) == (1024, 32)
    assert cfg.optimizer.type == want['optimizer']['type'] and dict(cfg.optimizer.kwargs) == want['optimizer']['kwargs']
    assert cfg.optimizer.part == want['optimizer']['part']
    assert cfg.scheduler.type == want['scheduler']['type'] and dict(cfg.scheduler.kwargs) == want['scheduler']['kwargs']
    for split in ('train', 'val', 'test'):
        for k, v in want['dataset'][split]['others'].items():
            assert cfg.dataset[split].others[k] == v, (split, k)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    args = parser.get_args(['--config', os.path.join(ROOT, path), '--finetune_model', '--svm_classification'])
    assert args.svm_classification and args.model_name == 'none'
