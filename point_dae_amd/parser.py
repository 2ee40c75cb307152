"""Command line of main.py: the flags of the reference's utils/parser.py:7-104
that matter on the pretraining and fine-tuning paths, same names and defaults."""
import argparse
import os
from pathlib import Path


def get_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--config', type=str, required=True, help='yaml config file')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none', help='job launcher')
    p.add_argument('--local_rank', type=int, default=0)
    p.add_argument('--num_workers', type=int, default=8)
    p.add_argument('--seed', type=int, default=0, help='random seed')
    p.add_argument('--deterministic', action='store_true')
    p.add_argument('--sync_bn', action='store_true', default=False, help='whether to use sync bn')
    p.add_argument('--exp_name', type=str, default='default', help='experiment name')
    p.add_argument('--root_folder', type=str, default='experiments')
    p.add_argument('--model_name', type=str, default='none', help='overrides model.NAME')
    p.add_argument('--start_ckpts', type=str, default=None, help='reload used ckpt path')
    p.add_argument('--ckpts', type=str, default=None)
    p.add_argument('--val_freq', type=int, default=1, help='test freq')
    p.add_argument('--vote', action='store_true', default=False, help='vote acc')
    p.add_argument('--resume', action='store_true', default=False)
    p.add_argument('--test', action='store_true', default=False, help='test mode for certain ckpt')
    p.add_argument('--vis_saliency', action='store_true', default=False,
                   help='saliency maps of a fine-tuned checkpoint: input-point gradients over the test set')
    p.add_argument('--saliency_score', choices=['logit', 'loss'], default='logit',
                   help='--vis_saliency: differentiate the label\'s logit (the reference) or the cloud\'s cross-entropy')
    p.add_argument('--total_bs', type=int, default=-1)
    p.add_argument('--finetune_model', action='store_true', default=False, help='finetune modelnet with pretrained weight')
    p.add_argument('--scratch_model', action='store_true', default=False, help='training modelnet from scratch')
    p.add_argument('--so3_rotation', action='store_true', default=False,
                   help='rotation-robustness fine-tuning: y-axis train rotation, ten-pass rotated validation')
    p.add_argument('--svm_classification', action='store_true', default=False,
                   help='linear-SVM evaluation of the frozen encoder: SVC(kernel=linear) for C = 1e-3 .. 1e2')
    p.add_argument('--task_affinity', action='store_true', default=False,
                   help='evaluate task affinity with pre-trained encoder.')
    p.add_argument('--part_seg', action='store_true', default=False,
                   help='part segmentation on ShapeNetPart; with --test --ckpts <segmentation checkpoint>: its evaluation')
    p.add_argument('--way', type=int, default=-1, help='few-shot fine-tuning: classes of the episode (5 or 10)')
    p.add_argument('--shot', type=int, default=-1, help='few-shot fine-tuning: training clouds per class (10 or 20)')
    p.add_argument('--fold', type=int, default=-1, help='few-shot fine-tuning: which of the ten episodes (0-9)')
    # synthetic-data controls (no dataset ships with this repo)
    p.add_argument('--max_epoch', type=int, default=-1, help='override config.max_epoch')
    p.add_argument('--steps_per_epoch', type=int, default=None,
                   help='batches per epoch; default for a listed .npy set: the reference\'s DataLoader length -- '
                        'floor(ceil(N / world) / bs) for the training subset (drop_last, tools/builder.py:21,28), ceil '
                        'otherwise; 50 for the synthetic set')
    p.add_argument('--vote_rounds', type=int, default=299,
                   help='--test: rounds of ten-vote evaluation (the reference hard-codes range(1, 300))')
    args = p.parse_args(argv)
    if args.test and args.resume:
        raise ValueError('--test and --resume cannot be both activate')
    if args.test and args.ckpts is None and not (args.part_seg and args.scratch_model):
        raise ValueError('ckpts shouldnt be None while test mode')
    if args.vis_saliency and args.ckpts is None:
        raise ValueError('ckpts shouldnt be None while vis_saliency mode')
    if args.vote_rounds < 0:
        raise ValueError('--vote_rounds must not be negative')
    if args.resume and args.start_ckpts is not None:
        raise ValueError('--resume and --start_ckpts cannot be both activate')
    given = [name for name in ('way', 'shot', 'fold') if getattr(args, name) != -1]
    if given and len(given) != 3:
        raise ValueError('few-shot fine-tuning needs --way, --shot and --fold together (given: %s)'
                         % ', '.join('--' + name for name in given))
    if args.finetune_model and args.scratch_model:
        raise ValueError('--finetune_model and --scratch_model cannot be both activate')
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    else:
        args.local_rank = int(os.environ['LOCAL_RANK'])
    if args.test:
        args.exp_name = 'test_' + args.exp_name
    stem = Path(args.config).stem + args.model_name
    args.experiment_path = os.path.join('./' + args.root_folder, stem, Path(args.config).parent.stem, args.exp_name)
    args.tfboard_path = os.path.join('./' + args.root_folder, stem, Path(args.config).parent.stem, 'TFBoard', args.exp_name)
    args.log_name = Path(args.config).stem
    if args.local_rank == 0:
        os.makedirs(args.experiment_path, exist_ok=True)
    return args
