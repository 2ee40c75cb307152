"""The saliency-map protocol (--vis_saliency), CPU side: the flags and their dispatch, the backend switch, the class
attribute that gates the protocol, and the grouping backward's formula against torch.autograd in fp64."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features.yaml')


def test_parser_accepts_vis_saliency(tmp_path, monkeypatch):
    from point_dae_amd import parser
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    args = parser.get_args(['--config', CFG])
    assert args.vis_saliency is False and args.saliency_score == 'logit'
    args = parser.get_args(['--config', CFG, '--vis_saliency', '--ckpts', 'x.pth', '--saliency_score', 'loss'])
    assert args.vis_saliency is True and args.saliency_score == 'loss'
    with pytest.raises(ValueError, match='ckpts'):
        parser.get_args(['--config', CFG, '--vis_saliency'])
    with pytest.raises(SystemExit):
        parser.get_args(['--config', CFG, '--vis_saliency', '--ckpts', 'x.pth', '--saliency_score', 'entropy'])


@pytest.mark.parametrize('flags,taken', [(['--vis_saliency', '--ckpts', 'x.pth'], 'vis_saliency_map'),
                                         (['--vis_saliency', '--ckpts', 'x.pth', '--finetune_model'], 'vis_saliency_map'),
                                         (['--test', '--vis_saliency', '--ckpts', 'x.pth'], 'test_net'),
                                         (['--scratch_model'], 'run_net')])
def test_main_dispatches_to_vis_saliency_map(tmp_path, monkeypatch, flags, taken):
    """main.py:94-103 of the reference: --test is looked at first, then --vis_saliency, then the fine-tuning runners."""
    from point_dae_amd import main, runner_finetune
    calls = []
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    for name in ('run_net', 'test_net', 'vis_saliency_map'):
        monkeypatch.setattr(runner_finetune, name, lambda args, config, name=name: calls.append(name))
    main.main(['--config', CFG, *flags])
    assert calls == [taken]


def test_main_refuses_the_distributed_launcher(tmp_path, monkeypatch):
    from point_dae_amd import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    with pytest.raises(NotImplementedError, match='one process'):
        main.main(['--config', CFG, '--vis_saliency', '--ckpts', 'x.pth', '--launcher', 'pytorch'])


def test_backend_selection(monkeypatch):
    from point_dae_amd import saliency_ops
    monkeypatch.delenv('PDAE_SALIENCY', raising=False)
    assert saliency_ops.backend() == 'hip'
    monkeypatch.setenv('PDAE_SALIENCY', 'torch')
    assert saliency_ops.backend() == 'torch'
    monkeypatch.setenv('PDAE_SALIENCY', 'eager')
    with pytest.raises(ValueError, match='PDAE_SALIENCY'):
        saliency_ops.backend()


def test_input_grad_supported_marks_the_transformer_family_only():
    from point_dae_amd.classifier import Classifier
    from point_dae_amd.dgcnn_cls import DGCNN
    from point_dae_amd.point_transformer import PointTransformer, PointTransformerLinearClassification
    assert Classifier.input_grad_supported is False and DGCNN.input_grad_supported is False
    assert PointTransformer.input_grad_supported is True
    assert PointTransformerLinearClassification.input_grad_supported is True


def test_input_gradients_refuses_an_unsupported_model_and_an_unknown_score():
    from point_dae_amd import saliency_ops

    class Plain(torch.nn.Module):
        input_grad_supported = False

    with pytest.raises(NotImplementedError, match='input_grad_supported'):
        saliency_ops.input_gradients(Plain(), torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match='score'):
        saliency_ops.input_gradients(Plain(), torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.int64), score='entropy')


def group_backward_reference(d_nbr, d_center, knn_idx, fps_idx, N):
    """d_xyz[b, n] = sum_{(g,j): knn_idx[b,g,j] = n} d_nbr[b,g,j] + sum_{g: fps_idx[b,g] = n} (d_center[b,g] - sum_j
    d_nbr[b,g,j]) by index_add, in the dtype of d_nbr (tests/test_gpu_saliency.py uses it in fp64)."""
    B, G, k, _ = d_nbr.shape
    out = torch.zeros(B, N, 3, dtype=d_nbr.dtype)
    for b in range(B):
        out[b].index_add_(0, knn_idx[b].reshape(-1).long(), d_nbr[b].reshape(G * k, 3))
        out[b].index_add_(0, fps_idx[b].long(), d_center[b] - d_nbr[b].sum(1))
    return out


def test_group_backward_formula_equals_autograd_in_fp64():
    """Random indices with forced duplicates: a centre that is its own first neighbour, a point that lies in three
    groups, a point in no group."""
    B, N, G, k = 2, 40, 5, 8
    g = torch.Generator().manual_seed(5)
    knn_idx = torch.randint(1, N, (B, G, k), generator=g)              # (point 0 of every cloud lies in no group)
    fps_idx = torch.stack([torch.randperm(N - 1, generator=g)[:G] + 1 for _ in range(B)]).to(torch.int32)
    knn_idx[:, :, 0] = fps_idx.long()                                   # every centre is its own first neighbour
    knn_idx[0, 0, 3] = knn_idx[0, 2, 5] = knn_idx[0, 4, 1] = 17         # one point in three groups
    xyz = torch.randn(B, N, 3, generator=g, dtype=torch.float64).requires_grad_()
    bi = torch.arange(B)[:, None]
    center = xyz[bi, fps_idx.long()]                                    # (B, G, 3)
    nbr = xyz[bi[:, :, None], knn_idx] - center[:, :, None]             # (B, G, k, 3)
    d_nbr = torch.randn(B, G, k, 3, generator=g, dtype=torch.float64)
    d_center = torch.randn(B, G, 3, generator=g, dtype=torch.float64)
    torch.autograd.backward([nbr, center], [d_nbr, d_center])
    got = group_backward_reference(d_nbr, d_center, knn_idx, fps_idx, N)
    assert torch.allclose(got, xyz.grad, rtol=1e-13, atol=1e-13)
    assert torch.equal(got[:, 0], torch.zeros(B, 3, dtype=torch.float64))
    assert got[0, 17].abs().sum() > 0
