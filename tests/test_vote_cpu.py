"""The voted evaluation without a GPU: the command line (--test, --vote, --vote_rounds), the order of the host draws against
a literal restatement of the reference's loop, and the host twin of pdae_vote_reduce."""
import numpy as np
import pytest


def _args(tmp_path, monkeypatch, *extra):
    from point_dae_amd import parser
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('LOCAL_RANK', '0')
    return parser.get_args(['--config', 'cfgs/x.yaml', *extra])


def test_parser_accepts_test_vote_and_vote_rounds(tmp_path, monkeypatch):
    args = _args(tmp_path, monkeypatch)
    assert args.test is False and args.vote is False and args.vote_rounds == 299
    args = _args(tmp_path, monkeypatch, '--test', '--ckpts', 'a.pth', '--vote_rounds', '2', '--exp_name', 'e')
    assert args.test is True and args.vote_rounds == 2 and args.ckpts == 'a.pth'
    assert args.exp_name == 'test_e'                        # utils/parser.py:127-128
    assert _args(tmp_path, monkeypatch, '--scratch_model', '--vote').vote is True


def test_parser_refuses_test_without_ckpts(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match='ckpts'):
        _args(tmp_path, monkeypatch, '--test')
    with pytest.raises(ValueError, match='resume'):
        _args(tmp_path, monkeypatch, '--test', '--ckpts', 'a.pth', '--resume')


def _reference_draws(B, point_all, npoints, times, scale_low=2. / 3., scale_high=3. / 2., translate_range=0.2):
    """tools/runner_finetune.py:861-866 with datasets/data_transforms.py:20-34 restated: per vote the subset draw, then per
    cloud three scale uniforms and three shift uniforms, each cast to fp32 as torch.from_numpy(...).float() does."""
    choice, scale, shift = [], [], []
    for kk in range(times):
        choice.append(np.random.choice(point_all, npoints, False))
        s, t = [], []
        for i in range(B):
            xyz1 = np.random.uniform(low=scale_low, high=scale_high, size=[3])
            xyz2 = np.random.uniform(low=-translate_range, high=translate_range, size=[3])
            s.append(xyz1.astype(np.float32))
            t.append(xyz2.astype(np.float32))
        scale.append(s)
        shift.append(t)
    return np.array(choice), np.array(scale), np.array(shift)


@pytest.mark.parametrize('B,point_all,npoints,times,seed', [(3, 40, 33, 4, 5), (1, 1200, 1024, 10, 0), (2, 16, 16, 1, 9)])
def test_draw_votes_makes_the_references_draws_in_its_order(B, point_all, npoints, times, seed):
    from point_dae_amd import vote_ops
    from point_dae_amd.data_transforms import PointcloudScaleAndTranslate
    np.random.seed(seed)
    want_choice, want_scale, want_shift = _reference_draws(B, point_all, npoints, times)
    want_next = np.random.random()
    np.random.seed(seed)
    choice, A, t = vote_ops.draw_votes(B, point_all, npoints, times, PointcloudScaleAndTranslate())
    assert np.random.random() == want_next                  # the generator is where the reference leaves it
    choice, A, t = choice.numpy(), A.numpy(), t.numpy()
    assert choice.dtype == np.int32 and choice.shape == (times, npoints)
    assert A.dtype == np.float32 and A.shape == (times, B, 3, 3) and t.dtype == np.float32 and t.shape == (times, B, 3)
    assert np.array_equal(choice, want_choice)
    assert np.array_equal(A[..., [0, 1, 2], [0, 1, 2]], want_scale)
    off = A.copy()
    off[..., [0, 1, 2], [0, 1, 2]] = 0
    assert not off.any()                                    # a diagonal map
    assert np.array_equal(t, want_shift)


def test_draw_votes_without_a_transform_draws_the_subsets_only():
    from point_dae_amd import vote_ops
    np.random.seed(3)
    want = [np.random.choice(24, 16, False) for _ in range(3)]
    want_next = np.random.random()
    np.random.seed(3)
    choice, A, t = vote_ops.draw_votes(2, 24, 16, 3, None)
    assert A is None and t is None and np.random.random() == want_next
    assert np.array_equal(choice.numpy(), np.array(want))


def test_reduce_host_ties_nan_and_one_vote():
    from point_dae_amd import vote_ops
    logits = np.array([[[1., 3., 3., 0.],                  # a tie: the lowest class
                        [0., np.nan, 5., 1.],               # a NaN: -1
                        [-2., -1., -3., -1.],
                        [0., -0., -1., -5.],                # +0 and -0 tie
                        [7., 1., 2., 3.]]], np.float32)
    mean, pred = vote_ops.reduce_host(logits)               # v = 1: the mean is the logits
    assert mean.dtype == np.float32 and np.array_equal(mean, logits[0], equal_nan=True)
    assert pred.dtype == np.int64 and pred.tolist() == [1, -1, 1, 0, 0]
    # a label outside 0 .. k-1 and the NaN row's -1 never count
    _, _, hits = vote_ops.reduce_host(logits, np.array([1, -1, 4, 0, 0]))
    assert hits == 3
    _, _, hits = vote_ops.reduce_host(logits, np.array([2, 2, -1, 1, 4]))
    assert hits == 0


def test_reduce_host_sums_in_vote_order_in_fp32():
    from point_dae_amd import vote_ops
    big = np.float32(2.0 ** 24)
    logits = np.array([[[big, 0.]], [[1., 0.]], [[-big, 0.]], [[1., 0.5]]], np.float32)      # ((big + 1) - big) + 1 = 1 in fp32
    mean, pred = vote_ops.reduce_host(logits)
    assert mean[0, 0] == np.float32(1.0) / np.float32(4.0) and mean[0, 1] == np.float32(0.125)
    assert pred.tolist() == [0]


def test_vote_point_all_is_the_voting_table():
    from point_dae_amd.runner_finetune import vote_point_all
    assert [vote_point_all(n, 10000) for n in (1024, 4096, 8192)] == [1200, 4800, 8192]
    assert vote_point_all(1024, 1100) == 1100
    with pytest.raises(NotImplementedError):
        vote_point_all(2048, 10000)


def test_backend_switch(monkeypatch):
    from point_dae_amd import vote_ops
    monkeypatch.delenv('PDAE_VOTE', raising=False)
    assert vote_ops.backend() == 'hip'
    monkeypatch.setenv('PDAE_VOTE', 'torch')
    assert vote_ops.backend() == 'torch'
    monkeypatch.setenv('PDAE_VOTE', 'eager')
    with pytest.raises(ValueError):
        vote_ops.backend()
