"""Entry point: `python -m point_dae_amd.main --config cfgs/X.yaml [--launcher pytorch]`
(main.py:16-111 of the reference): pretraining, or with --finetune_model / --scratch_model the
classification fine-tuning runner (--so3_rotation: its rotation-robustness protocol; --svm_classification: the linear-SVM
evaluation of the frozen encoder; --task_affinity: the linear probe whose test loss ranks corruptions; --vote: a ten-vote
validation behind a high plain one; --way/--shot/--fold: one fold of few-shot fine-tuning), or with --test --ckpts the
evaluation of a fine-tuned checkpoint: the plain accuracy, then --vote_rounds rounds of ten-vote evaluation; or with
--part_seg --test --ckpts the part-segmentation evaluation of a segmentation checkpoint on ShapeNetPart (the Transformer or,
with cfgs/segmentation_shapenetpart_dgcnn.yaml, the DGCNN); or with
--vis_saliency --ckpts its saliency maps: the gradient of the score with respect to every input point of the test set."""
import torch

from . import dist_utils, parser
from .config import get_config
from .misc import set_random_seed
from . import runner_finetune, runner_pretrain


def apply_fewshot_args(args, config):
    """main.py:85-91 of the reference: with --shot given, --way / --shot / --fold go into the train and the val dataset
    node (and into the test node where the config has one: the fine-tuning loop validates on it)."""
    if args.shot == -1:
        return config
    for subset in ('train', 'val', 'test'):
        node = config.dataset.get(subset)
        if node is None:
            continue
        node.others.shot, node.others.way, node.others.fold = args.shot, args.way, args.fold
    return config


def main(argv=None):
    args = parser.get_args(argv)
    fewshot = args.shot != -1
    if fewshot:
        # (the three lines utils/parse_test_res.py --few-shot reads from a redirected log, next to '[Validation] ... acc = ')
        print('args.way : %d' % args.way)
        print('args.shot : %d' % args.shot)
        print('args.fold : %d' % args.fold)
    if args.part_seg and args.launcher != 'none':
        raise NotImplementedError('--part_seg runs in one process: --launcher none')
    if args.part_seg and not args.test:
        raise NotImplementedError('part-segmentation training is not built')
    args.use_gpu = torch.cuda.is_available()
    if not args.use_gpu:
        raise RuntimeError('point_dae_amd needs an MI355X: there is no CPU path')
    if fewshot and args.launcher != 'none':
        # an episode is 50 to 200 clouds: one process, as the other small protocols
        raise ValueError('few-shot fine-tuning (--way/--shot/--fold) runs in one process: --launcher none')
    if args.svm_classification and args.launcher != 'none':
        # the reference runs this protocol in ONE process under DataParallel (rerun.sh); its distributed branch would fit
        # every rank's SVMs on that rank's shard of the features
        raise ValueError('--svm_classification runs in one process: --launcher none')
    if args.task_affinity and args.launcher != 'none':
        # (the same: every rank would train its probe on its own shard of the features)
        raise ValueError('--task_affinity runs in one process: --launcher none')
    if args.test and args.launcher != 'none':
        raise NotImplementedError('--test runs in one process: --launcher none')   # runner_finetune.py:697-699
    if args.vis_saliency and args.launcher != 'none':
        raise NotImplementedError('--vis_saliency runs in one process: --launcher none')
    if args.launcher == 'none':
        args.distributed = False
        args.world_size = 1
        torch.cuda.set_device(args.local_rank)
    else:
        args.distributed = True
        import os
        dist_utils.init_dist(args.launcher, backend=os.environ.get('PDAE_DIST_BACKEND', 'nccl'))
        _, args.world_size = dist_utils.get_dist_info()
    config = get_config(args)
    if args.model_name != 'none':
        config.model.NAME = args.model_name
    if args.total_bs != -1:
        config.total_bs = args.total_bs
    if args.max_epoch != -1:
        config.max_epoch = args.max_epoch
    finetune = args.finetune_model or args.scratch_model
    if not finetune and not args.test and not args.vis_saliency and len(config.model['corrupt_type']) == 0:   # main.py:51-55 (pretraining configs only)
        config.model['corrupt_type'] = config.dataset['train']['others']['corrupt_type']
    assert config.total_bs % args.world_size == 0
    config.dataset.train.others.bs = config.total_bs // args.world_size
    set_random_seed(args.seed + args.local_rank, deterministic=args.deterministic)   # main.py:78-81
    apply_fewshot_args(args, config)                                                 # main.py:85-91
    if args.part_seg:
        runner_finetune.part_seg_test(args, config)                        # segmentation/main.py:231-298
    elif args.test:
        runner_finetune.test_net(args, config)                             # main.py:94-95
    elif args.vis_saliency:
        runner_finetune.vis_saliency_map(args, config)                     # main.py:96-97
    elif finetune and args.svm_classification:
        runner_finetune.svm_classification(args, config)                   # main.py:102-103
    elif finetune and args.task_affinity:
        runner_finetune.task_affinity(args, config)                        # main.py:104-105
    elif finetune and args.so3_rotation:
        runner_finetune.run_net_rotation(args, config)                     # main.py:106-107
    elif finetune:
        runner_finetune.run_net(args, config)                              # main.py:96-103
    else:
        runner_pretrain.run_net(args, config)


if __name__ == '__main__':
    main()
