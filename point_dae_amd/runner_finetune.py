"""Classification fine-tuning loop (tools/runner_finetune.py:81-318 of the reference).

Same control flow: FPS of every cloud to `point_all` points, a host np.random.choice of `npoints` of them, the gather;
forward, cross-entropy, backward; the gradient-norm clip (clip_grad_norm_ with `grad_norm_clip`) then AdamW; the
epoch-granular CosLR; validation on the test set with FPS to `npoints`, argmax accuracy, ckpt-best / ckpt-last.  The
clip coefficient stays on the device (finetune_ops.GradNormClip -> FlatAdamW grad_scale), and loss / accuracy are
accumulated on the device and read back once per log line, where the reference calls .item() twice per step.

run_net_rotation / validate_rotation (:322-564, main.py --so3_rotation) are the same loop with a train transform inside
the resample (data_transforms.resample_transformed: one launch into the graphed step's input) and ten validation passes.

svm_classification (:902-1049, main.py --svm_classification) trains nothing: one eval pass of the frozen encoder over the
train and the val loader, then the six linear SVMs of svm_ops on the features, which never leave the device.

task_affinity (:1052-1269, main.py --task_affinity) makes the same two passes, then trains the linear probe of
affinity_ops on the train features and reports its accuracy and mean cross-entropy on the test features.

test_net / test_vote / validate_vote (:686-748, :835-899, :568-632; main.py --test, --vote) evaluate a fine-tuned
checkpoint by voting: per test cloud ten subsets of its FPS order, each through test_transforms and the model, the mean of
the logits.  vote_pass runs one such pass on vote_ops (csrc/vote.hip); FPS is kept per test batch across passes, the hits
are counted on the device and test_net reads its rounds' counters once.

vis_saliency_map (:751-833, main.py --vis_saliency) differentiates a fine-tuned classifier's score with respect to its
input points over the test set, a batch at a time (saliency_ops), and saves the reference's (n, npoints, 6) tensor.

part_seg_test (segmentation/main.py:231-298, main.py --part_seg --test) evaluates a segmentation checkpoint on ShapeNetPart:
one evaluation pass of part_seg.PointTransformerPartSeg or dgcnn_partseg.DGCNNPartSeg (the config's model), the metric's
integer counts on the device (partseg_ops), one read-back, the reference's mIoU lines.

Few-shot fine-tuning (main.py --way/--shot/--fold, datasets.ModelNetFewShot) is run_net on one resident episode: the
train loader yields the draws of a batch (items, a fresh point shuffle per row) and fewshot_train_points makes the step's
input of them -- fewshot_ops (csrc/fewshot.hip): one launch --; the test loader's FPS-to-npoints point sets are taken once
per fold (fewshot_point_sets) and every later validation runs only the forward.

A ModelNet loader on the reference's processed files (datasets.ModelNet, `listed`) shuffles its items per epoch and redraws
every cloud's maps and point shuffle per access; under PDAE_MODELNET=hip its draws go through resident_train_points --
resident_ops (csrc/fewshot.hip, pdae_resident_batch): one launch into the step's input --, and a test loader that repeats
itself exactly keeps its point sets the way the few-shot one does.
"""
import time

import numpy as np
import torch

from . import builder, dist_utils
from . import datasets  # noqa: F401  (registers the synthetic ModelNet set)
from .data_parallel import FlatDataParallel
from .finetune_ops import GradNormClip
from .misc import fps
from .pointnet2_utils import furthest_point_sample, gather_operation
from .registry import DATASETS
from .svm_probe import Acc_Metric

POINT_ALL = {1024: 1200, 2048: 2400, 4096: 4800, 8192: 8192}      # runner_finetune.py:160-171
VOTE_POINT_ALL = {1024: 1200, 4096: 4800, 8192: 8192}             # runner_finetune.py:846-853 (voting: no 2048 row)


def set_bn_eval(m):
    """tools/runner_finetune.py:30-37, applied to every module after train() under optimizer.part only_new: a BatchNorm
    whose width is not 256 belongs to the pretrained model and runs on its running estimates (256 is the new head's
    BatchNorm, which keeps learning its own).  Dropout and DropPath stay live."""
    if 'BatchNorm' in type(m).__name__ and m.weight.size(0) != 256:
        m.eval()


def set_train_mode(model, part):
    """The mode of a training epoch: train(), then set_bn_eval under only_new (runner_finetune.py:141-146)."""
    model.train()
    if part == 'only_new':
        model.apply(set_bn_eval)
    return model


def subset_indices(npoints, point_all):
    """The host draw of runner_finetune.py:174: npoints of the point_all FPS indices, without replacement."""
    return np.random.choice(point_all, npoints, False)


def resample(points, npoints, choice=None, point_all=None):
    """FPS of each cloud to point_all points (default: the fine-tuning loop's oversampling POINT_ALL[npoints]), then the
    columns `choice` (default: a fresh host draw) of the FPS order, gathered -> (B, npoints, 3)
    (runner_finetune.py:158-176)."""
    if npoints not in POINT_ALL:
        raise NotImplementedError('npoints %d' % npoints)
    point_all = min(POINT_ALL[npoints] if point_all is None else point_all, points.shape[1])
    xyz = points[:, :, :3].contiguous()
    fps_idx = furthest_point_sample(xyz, point_all)
    if choice is None:
        choice = subset_indices(npoints, point_all)
    choice = torch.as_tensor(choice, dtype=torch.int64).to(points.device, non_blocking=True)
    idx = fps_idx.index_select(1, choice).contiguous()
    return gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()


def fewshot_train_points(train_loader, data, npoints, out=None):
    """The training batch of a few-shot episode from the loader's draws data = (item, perm, labels): FPS of every row's
    shuffled cloud to point_all points and the host draw of npoints of them (runner_finetune.py:158-176).
    PDAE_FEWSHOT=hip: fewshot_ops.fill_batch, one launch into `out` (a fresh buffer when None) -> out; torch:
    fewshot_ops.materialise + resample -> a new (B, npoints, 3) tensor.  Both take the same host draw."""
    from . import fewshot_ops
    if npoints not in POINT_ALL:
        raise NotImplementedError('npoints %d' % npoints)
    item, perm = data[0], data[1]
    set_ = train_loader.set
    point_all = min(POINT_ALL[npoints], set_.shape[1])
    choice = subset_indices(npoints, point_all)
    if fewshot_ops.backend() == 'torch':
        return resample(fewshot_ops.materialise(set_, item, perm), npoints, choice=choice)
    if out is None:
        out = torch.empty((item.shape[0], npoints, 3), dtype=torch.float32, device=set_.device)
    return fewshot_ops.fill_batch(set_, item, perm, choice, point_all, out)


def resident_train_points(train_loader, data, npoints, out):
    """The training batch of a resident ModelNet loader from its draws data = (item, perm, nmaps, maps, labels)
    (datasets.ModelNet.iter_draws): the maps, the shuffle, FPS to point_all points and the host draw of npoints of them,
    by one launch into `out` (resident_ops.fill_batch, csrc/fewshot.hip) -> out."""
    from . import resident_ops
    if npoints not in POINT_ALL:
        raise NotImplementedError('npoints %d' % npoints)
    item, perm, nmaps, maps = data[:4]
    set_ = train_loader.set
    point_all = min(POINT_ALL[npoints], set_.shape[1])
    choice = subset_indices(npoints, point_all)
    return resident_ops.fill_batch(set_, item, perm, nmaps, maps, choice, point_all, out)


def train_step(model, optimizer, clip, points, labels):
    """One optimisation step: forward, loss, backward, [gradient all-reduce], clip coefficient, AdamW.
    -> (loss, acc) device scalars."""
    base = model.module if isinstance(model, FlatDataParallel) else model
    ret = model(points)
    loss, acc = base.get_loss_acc(ret, labels)
    loss.backward()
    if isinstance(model, FlatDataParallel):
        model.finish()                                  # the norm is taken after the all-reduce, as DDP + clip do
    optimizer.step(grad_scale=clip() if clip is not None else None)
    model.zero_grad()
    return loss.detach(), acc.detach()


def fewshot_point_sets(test_loader, npoints):
    """The FPS-to-npoints point sets of a few-shot test loader, [(points (b, npoints, C), label (b,))] per batch: the test
    subset is never shuffled, so they are the same on every epoch of a fold and are taken once.  PDAE_FEWSHOT=hip:
    pdae_fewshot_batch with perm = slot = NULL; torch: misc.fps.  A listed ModelNet test loader without per-access
    augmentation (fps_cacheable) is kept the same way, under PDAE_MODELNET."""
    from . import fewshot_ops, resident_ops
    # (a listed ModelNet test loader keeps its point sets the same way, under PDAE_MODELNET)
    ops = fewshot_ops if getattr(test_loader, 'fewshot', False) else resident_ops
    sets = []
    for _, _, data in test_loader:
        points, label = data[0].cuda(), data[1].cuda()
        if ops.backend() == 'hip' and points.shape[2] == 3:
            points = ops.fps_points(points, npoints)
        else:
            _, points = fps(points, npoints)
        sets.append((points, label))
    return sets


def _predict(base_model, test_loader, config, args=None, point_sets=None):
    """One pass over the test loader: FPS to npoints, eval forward, argmax -> (pred, label) of every test cloud [of every
    rank].  point_sets: a list that keeps the FPS-to-npoints point sets of a loader that repeats itself exactly (a
    few-shot test loader): filled by the first pass (fewshot_point_sets), later passes run only the forward."""
    preds, labels = [], []
    if point_sets is not None and not point_sets:
        point_sets.extend(fewshot_point_sets(test_loader, config.npoints))
    for _, _, data in (test_loader if point_sets is None else ((None, None, d) for d in point_sets)):
        points, label = data[0].cuda(), data[1].cuda()
        if point_sets is None:
            _, points = fps(points, config.npoints)
        preds.append(base_model(points).argmax(-1).view(-1))
        labels.append(label.view(-1))
    pred, label = torch.cat(preds), torch.cat(labels)
    if args is not None and getattr(args, 'distributed', False):
        pred, label = dist_utils.gather_tensor(pred, args), dist_utils.gather_tensor(label, args)
    return pred, label


@torch.no_grad()
def validate(base_model, test_loader, epoch, config, args=None, log=print, point_sets=None):
    """runner_finetune.py:273-318: FPS to npoints, eval forward, argmax accuracy over the whole test set.  point_sets:
    _predict's list of kept point sets (few-shot: the test loader repeats itself exactly)."""
    base_model.eval()
    pred, label = _predict(base_model, test_loader, config, args, point_sets)
    acc = float((pred == label).sum().item()) / float(label.numel()) * 100.
    log('[Validation] EPOCH: %d  acc = %.4f' % (epoch, acc))
    return Acc_Metric(acc)


@torch.no_grad()
def validate_rotation(base_model, test_loader, epoch, config, args=None, log=print, passes=10):
    """runner_finetune.py:515-564: `passes` full passes over the test loader, whose 'rotate' / 'rotate_z' item draws a fresh
    rotation for every cloud on every pass; the accuracy of each pass (gathered per pass), then their fp32 mean."""
    base_model.eval()
    accs = []
    for _ in range(passes):
        pred, label = _predict(base_model, test_loader, config, args)
        accs.append((pred == label).sum() / float(label.size(0)) * 100.)
    acc = torch.Tensor([float(a) for a in accs]).mean()
    log('[Validation] EPOCH: %d  acc = %.4f' % (epoch, acc))
    return Acc_Metric(float(acc))


def vote_point_all(npoints, cloud_size):
    """runner_finetune.py:846-856: the voting table's FPS size for npoints, capped at the cloud's size."""
    if npoints not in VOTE_POINT_ALL:
        raise NotImplementedError('voting with npoints %d (the reference votes at 1024, 4096 and 8192)' % npoints)
    return min(VOTE_POINT_ALL[npoints], cloud_size)


def vote_pass(base_model, test_loader, config, times=10, fps_cache=None, correct=None):
    """One voted pass over the test loader (runner_finetune.py:843-880) on vote_ops: per batch FPS to point_all points
    -- taken from fps_cache[batch] when the list holds it, appended to the list otherwise: the test subset is not
    shuffled and FPS draws nothing, so a batch's FPS order is the same on every pass --, the host draws of the `times`
    votes (vote_ops.draw_votes), vote_ops.vote_batch.  correct: one int32 device counter that receives the hits (a fresh
    one by default).  Nothing is read back.  -> (pred (n,), label (n,), mean logits (n, K), correct)."""
    from . import vote_ops
    from .data_transforms import PointcloudScaleAndTranslate
    test_transforms = PointcloudScaleAndTranslate()                       # runner_finetune.py:53-59
    preds, labels, means = [], [], []
    for i, (_, _, data) in enumerate(test_loader):
        raw, label = data[0].cuda().contiguous(), data[1].cuda().view(-1).long()
        if correct is None:
            correct = torch.zeros(1, dtype=torch.int32, device=raw.device)
        B, P, C = raw.shape
        point_all = vote_point_all(config.npoints, P)
        if fps_cache is not None and i < len(fps_cache):
            fps_idx = fps_cache[i]
        else:
            fps_idx = furthest_point_sample(raw if C == 3 else raw[:, :, :3].contiguous(), point_all)
            if fps_cache is not None:
                fps_cache.append(fps_idx)
        draws = vote_ops.draw_votes(B, point_all, config.npoints, times, test_transforms, device=raw.device)
        pred, mean = vote_ops.vote_batch(base_model, raw, fps_idx, label, draws, correct)
        preds.append(pred)
        labels.append(label)
        means.append(mean)
    return torch.cat(preds), torch.cat(labels), torch.cat(means), correct


def fps_cacheable(test_loader):
    """Whether a loader yields the same clouds on every pass, so that a batch's FPS order may be kept: the ModelNet set
    with no augmentation but 'norm' (every other item draws per pass)."""
    aug = getattr(test_loader, 'aug_type', None)
    return aug is not None and all(item == 'norm' for item in aug)


def _percent(correct, total):
    """The reference's (pred == label).sum() / float(n) * 100. -- a division and a product of fp32 tensors."""
    return float(np.float32(correct) / np.float32(total) * np.float32(100.))


@torch.no_grad()
def test_vote(base_model, test_loader, config, args=None, times=10, fps_cache=None):
    """runner_finetune.py:835-899: the accuracy in percent of the mean logits of `times` votes per test cloud.
    fps_cache: a list of per-batch fps_idx tensors; the first pass fills it, later passes reuse it."""
    base_model.eval()
    pred, label, _, correct = vote_pass(base_model, test_loader, config, times, fps_cache)
    if args is not None and getattr(args, 'distributed', False):
        pred, label = dist_utils.gather_tensor(pred, args), dist_utils.gather_tensor(label, args)
        return _percent((pred == label).sum().item(), label.numel())
    return _percent(correct.item(), label.numel())


@torch.no_grad()
def validate_vote(base_model, test_loader, epoch, config, args=None, log=print, times=10, fps_cache=None):
    """runner_finetune.py:568-632: test_vote inside run_net (--vote), gathered across the ranks as validate is."""
    log('[VALIDATION_VOTE] epoch %d' % epoch)
    acc = test_vote(base_model, test_loader, config, args, times, fps_cache)
    log('[Validation_vote] EPOCH: %d  acc_vote = %.4f' % (epoch, acc))
    return Acc_Metric(acc)


@torch.no_grad()
def test_net(args, config, log=print):
    """runner_finetune.py:686-748 (main.py --test): the test loader, the model with builder.load_model(args.ckpts) in
    eval mode; '[TEST] acc' of the plain pass (FPS to npoints, argmax), then args.vote_rounds (the reference: 299) rounds
    of ten-vote evaluation and the best of them.  Under PDAE_VOTE=hip every round adds its hits to a device counter of
    its own, FPS runs once per batch for the whole test, and the host reads all counters once behind the last round --
    the rounds' lines are printed then; PDAE_VOTE=torch reads and prints round by round.  -> the best accuracy."""
    from . import vote_ops
    if getattr(args, 'distributed', False) or getattr(args, 'launcher', 'none') != 'none':
        raise NotImplementedError('--test runs in one process (the reference raises for --launcher pytorch too)')
    device = torch.device('cuda', torch.cuda.current_device())
    log('Tester start ... ')
    test_loader = _loader(config.dataset.test, device, args.seed, 0, 1, config.total_bs)
    _log_sources(log, None, test_loader)
    base_model = builder.model_builder(config.model)
    builder.load_model(base_model, args.ckpts)
    base_model = base_model.to(device).eval()
    pred, label = _predict(base_model, test_loader, config, args)
    total = label.numel()
    log('[TEST] acc = %.4f' % _percent((pred == label).sum().item(), total))
    log('[TEST_VOTE]')
    rounds = int(getattr(args, 'vote_rounds', 299))
    fused = vote_ops.backend() == 'hip'
    log('Vote backend: %s' % vote_ops.backend())
    fps_cache = [] if fused and fps_cacheable(test_loader) else None
    counters = torch.zeros(max(rounds, 1), dtype=torch.int32, device=device)
    accs = []
    for r in range(rounds):
        vote_pass(base_model, test_loader, config, 10, fps_cache, counters[r:r + 1])
        if not fused:
            accs.append(_percent(counters[r].item(), total))
            log('[TEST_VOTE_time %d]  acc = %.4f, best acc = %.4f' % (r + 1, accs[-1], max(accs)))
    acc = 0.
    if fused:
        for r, hits in enumerate(counters[:rounds].tolist()):           # the test's one read-back
            this_acc = _percent(hits, total)
            acc = max(acc, this_acc)
            log('[TEST_VOTE_time %d]  acc = %.4f, best acc = %.4f' % (r + 1, this_acc, acc))
    elif accs:
        acc = max(accs)
    log('[TEST_VOTE] acc = %.4f' % acc)
    return acc


@torch.no_grad()
def part_seg_test(args, config, log=print):
    """segmentation/main.py:231-298 of the reference (main.py --part_seg --test): one pass over the `test` split of
    ShapeNetPart with a segmentation checkpoint (model.load_segmentation_checkpoint(args.ckpts); --scratch_model in
    place of --ckpts: the initial weights) in evaluation mode; the model is the config's, PointTransformerPartSeg or
    DGCNNPartSeg (a model may name its own default backend: partseg_mode).  Every shape's prediction is the argmax over its own
    part range, taken from its first point's label; the metric's integer counts stay on the device
    (partseg_ops.Counts) and are read ONCE behind the last batch; the host forms accuracy, class_avg_accuracy, the
    per-category mIoU, class_avg_iou and inctance_avg_iou in float64 and prints the reference's lines.  -> the
    instance mIoU; the four metrics are left in args.part_seg_metrics."""
    from . import partseg_ops
    if getattr(args, 'distributed', False) or getattr(args, 'launcher', 'none') != 'none':
        raise NotImplementedError('--part_seg runs in one process: --launcher none')
    device = torch.device('cuda', torch.cuda.current_device())
    log('Tester start ... ')
    test_loader = _loader(config.dataset.test, device, args.seed, 0, 1, config.total_bs)
    log('ShapeNetPart test source: %s' % test_loader.source)
    base_model = builder.model_builder(config.model)
    if args.ckpts is not None:
        base_model.load_segmentation_checkpoint(args.ckpts, log=log)
    elif getattr(args, 'scratch_model', False):
        base_model.load_model_from_ckpt(None, log=log)
    else:
        raise ValueError('ckpts shouldnt be None while test mode')
    base_model = base_model.to(device).eval()
    log('Part-segmentation backend: %s' % getattr(base_model, 'partseg_mode', partseg_ops.mode)())
    counts = partseg_ops.Counts(test_loader.count, device)
    for _, _, (points, cls, seg) in test_loader:
        base_model(points, cls, seg=seg, counts=counts)
    m = partseg_ops.metrics(counts.read())                              # the test's one read-back
    for cat in sorted(m['category_iou']):
        log('eval mIoU of %s %f' % (cat + ' ' * (14 - len(cat)), m['category_iou'][cat]))
    log('test Accuracy: %f  Class avg mIOU: %f   Inctance avg mIOU: %f'
        % (m['accuracy'], m['class_avg_iou'], m['inctance_avg_iou']))
    args.part_seg_metrics = m
    return m['inctance_avg_iou']


def vis_saliency_map(args, config, log=print):
    """runner_finetune.py:751-833 (main.py --vis_saliency): the gradient of a fine-tuned classifier's score with respect
    to every input point, over the whole test set.  The test loader and the model as in test_net; every parameter frozen;
    per test batch -- the full total_bs, where the reference takes one cloud at a time because its `logits[0, label]`
    must be a scalar -- FPS to npoints and saliency_ops.input_gradients (one eval forward, one data-only backward);
    cat([points, grad], dim=2) of all batches, (n, npoints, 6) on the device, is saved ONCE to
    <experiment_path>/saliency.pt (the reference's tensor layout; its hard-coded path and debugger stop are not
    reproduced).  '[TEST] acc' comes from the same logits.  Must not run under no_grad.  -> the saved tensor."""
    import os
    from . import saliency_ops
    if getattr(args, 'distributed', False) or getattr(args, 'launcher', 'none') != 'none':
        raise NotImplementedError('--vis_saliency runs in one process: --launcher none')
    device = torch.device('cuda', torch.cuda.current_device())
    log('Saliency start ... ')
    test_loader = _loader(config.dataset.test, device, args.seed, 0, 1, config.total_bs)
    _log_sources(log, None, test_loader)
    base_model = builder.model_builder(config.model)
    if not getattr(base_model, 'input_grad_supported', False):
        raise NotImplementedError(
            '--vis_saliency: %s.input_grad_supported is False -- its backward carries no gradient down to the input '
            'points (the PointTransformer classifiers do)' % type(base_model).__name__)
    builder.load_model(base_model, args.ckpts)
    base_model = base_model.to(device).eval()
    for p in base_model.parameters():
        p.requires_grad_(False)
    score = getattr(args, 'saliency_score', 'logit')
    log('Saliency backend: %s, score: %s' % (saliency_ops.backend(), score))
    maps, preds, labels = [], [], []
    for _, _, data in test_loader:
        points, label = data[0].cuda(), data[1].cuda().view(-1).long()
        with torch.no_grad():
            _, points = fps(points, config.npoints)
        logits, grad = saliency_ops.input_gradients(base_model, points, label, score)
        maps.append(torch.cat([points[:, :, :3], grad], dim=2))
        preds.append(logits.argmax(-1).view(-1))
        labels.append(label)
    saliency = torch.cat(maps)
    pred, label = torch.cat(preds), torch.cat(labels)
    log('[TEST] acc = %.4f' % _percent((pred == label).sum().item(), label.numel()))
    path = os.path.join(args.experiment_path, 'saliency.pt')
    torch.save(saliency, path)
    log('Saliency map %s saved to %s' % (tuple(saliency.shape), path))
    return saliency


def _loader(node, device, seed, rank, world, bs, steps_per_epoch=None):
    c = dict(node._base_)
    c.update(dict(node.others))
    # ModelNetDataset yields N_POINTS points per cloud (the config's npoints is what the runner samples from them)
    c['npoints'] = int(c.get('N_POINTS', c.get('npoints', 1024)))
    c.update(device=device, seed=seed, rank=rank, world=world)
    if steps_per_epoch is not None:
        c.update(count=steps_per_epoch * bs)
    c.setdefault('bs', bs)
    return DATASETS.build(c)


def _log_sources(log, train_loader, test_loader):
    """One line per ModelNet loader saying where its clouds come from: the reference's processed file or the stand-in."""
    for name, loader in (('train', train_loader), ('test', test_loader)):
        if getattr(loader, 'source', None) is not None:
            log('ModelNet %s source: %s' % (name, loader.source))


def run_net(args, config, log=print, log_every=20):
    return _run(args, config, log, log_every)


def run_net_rotation(args, config, log=print, log_every=20):
    """runner_finetune.py:322-511 (--so3_rotation; z/z, z/SO(3) and SO(3)/SO(3) alike): run_net with train_transforms --
    data_transforms.PointcloudRotate, a y-axis rotation per cloud -- behind the resample, and validate_rotation."""
    from .data_transforms import PointcloudRotate
    return _run(args, config, log, log_every, train_transform=PointcloudRotate(), validate_fn=validate_rotation)


def _run(args, config, log, log_every, train_transform=None, validate_fn=validate):
    """The loop of run_net.  With a train_transform the batch is prepared by data_transforms.resample_transformed (the
    subset, the gather and the transform's map: one launch, straight into the graphed step's input buffer)."""
    rank, world = dist_utils.get_dist_info()
    device = torch.device('cuda', torch.cuda.current_device())
    from .graph_step import use_created_stream
    use_created_stream(device)
    bs = config.total_bs // world
    spe = getattr(args, 'steps_per_epoch', None)
    train_loader = _loader(config.dataset.train, device, args.seed + rank, rank, world, bs, spe)
    test_loader = _loader(config.dataset.test if config.dataset.get('test') is not None else config.dataset.val,
                          device, args.seed, rank, world, bs)

    base_model = builder.model_builder(config.model)
    part = config.optimizer.get('part', 'all')
    if part == 'only_new' and getattr(base_model, 'only_new_unsupported', None):
        raise NotImplementedError('runner_finetune: optimizer.part only_new with %s: %s'
                                  % (type(base_model).__name__, base_model.only_new_unsupported))
    start_epoch, best_metric = 0, 0.
    if args.resume:
        start_epoch, best_metric = builder.resume_model(base_model, args)
    elif args.ckpts is not None:
        base_model.load_model_from_ckpt(args.ckpts, log=log)           # runner_finetune.py:100-101
    else:
        base_model.load_model_from_ckpt(None, log=log)
    base_model = base_model.to(device)
    model = FlatDataParallel(base_model)
    optimizer, scheduler = builder.build_opti_sche(model, config)
    from .optim import FlatAdamW
    if not isinstance(optimizer, FlatAdamW):
        raise NotImplementedError('runner_finetune: the fused AdamW (optimizer.part: all, only_new, diff_lr) is the only '
                                  'optimiser that reads the device-side clip coefficient; part %r is not supported'
                                  % part)
    model.zero_grad()
    clip = GradNormClip(model.flat_grad, config.grad_norm_clip) if config.get('grad_norm_clip') is not None else None
    if int(config.get('step_per_update', 1)) != 1:
        raise NotImplementedError('runner_finetune: step_per_update > 1 (gradient accumulation) is not supported')
    best_metrics, metrics = Acc_Metric(best_metric), Acc_Metric(0.)
    # --vote: one voted validation behind a plain one that is high enough; the test batches' FPS orders are kept across them
    vote, best_metrics_vote = bool(getattr(args, 'vote', False)), Acc_Metric(0.)
    vote_fps = [] if vote and fps_cacheable(test_loader) else None
    # the step is replayed as a hipGraph (graph_step.GraphedClassifierStep)
    from .graph_step import GraphedClassifierStep
    if train_transform is not None:
        from .data_transforms import resample_transformed
    graphed = GraphedClassifierStep(model, optimizer, clip, bs, config.npoints)
    # few-shot (--way/--shot/--fold): the train loader yields (item, perm, labels) of the resident episode
    # (fewshot_train_points); the test loader's FPS-to-npoints point sets are taken once per fold
    fewshot = bool(getattr(train_loader, 'fewshot', False))
    if fewshot and train_transform is not None:
        raise NotImplementedError('runner_finetune: few-shot episodes with a train transform (--so3_rotation)')
    # a ModelNet loader on the reference's files (datasets.ModelNet, `listed`): the train loader's draws go through
    # resident_train_points under PDAE_MODELNET=hip; a test loader that repeats itself exactly keeps its point sets
    from . import resident_ops
    offered = bool(getattr(train_loader, 'resident', False)) and not fewshot and train_transform is None
    resident = offered and resident_ops.backend() == 'hip'
    keep_sets = getattr(test_loader, 'fewshot', False) or (getattr(test_loader, 'listed', False) and fps_cacheable(test_loader))
    if keep_sets and validate_fn is validate:
        import functools
        validate_fn = functools.partial(validate, point_sets=[])
    if rank == 0:
        log('step: hipGraph replay (GraphedClassifierStep)')
        _log_sources(log, train_loader, test_loader)
        if offered:
            log('ModelNet backend: %s' % resident_ops.backend())
        if fewshot:
            from . import fewshot_ops
            log('Few-shot backend: %s' % fewshot_ops.backend())
        if train_transform is not None:
            log('train transform: %s inside the resample; validation: %s' % (type(train_transform).__name__, validate_fn.__name__))

    for epoch in range(start_epoch, config.max_epoch + 1):
        # (the BatchNorm modes are the same every epoch, so the graph captured in the first one stays valid; the clip
        # coefficient is taken over the WHOLE flat gradient under every part, as clip_grad_norm_(parameters()) is)
        set_train_mode(model, part)
        if hasattr(train_loader, 'set_epoch'):
            train_loader.set_epoch(epoch)
        acc_sum = torch.zeros(2, device=device)
        t0, n = time.time(), 0
        for idx, (_, _, data) in enumerate(train_loader.iter_draws() if resident else train_loader):
            if resident:
                resident_train_points(train_loader, data, config.npoints, out=graphed.points)
                loss, acc = graphed.step_filled(data[4])
            elif fewshot:
                points = fewshot_train_points(train_loader, data, config.npoints, out=graphed.points)
                if points is graphed.points:                     # hip: the launch wrote the step's input
                    loss, acc = graphed.step_filled(data[2])
                else:                                            # torch: the reference's loop made a tensor of its own
                    loss, acc = graphed(points, data[2])
            elif train_transform is None:
                points = resample(data[0], config.npoints)
                loss, acc = graphed(points, data[1])             # (the train loader yields only full batches)
            else:
                resample_transformed(data[0], config.npoints, train_transform, out=graphed.points)
                loss, acc = graphed.step_filled(data[1])
            acc_sum += torch.stack([loss, acc])
            n += 1
            if (idx + 1) % log_every == 0 or idx + 1 == len(train_loader):
                vals = acc_sum.clone()
                if world > 1:
                    vals = dist_utils.reduce_tensor(vals, args)
                vals = (vals / n).tolist()                   # one host sync per log line
                if rank == 0:
                    log('[Epoch %d/%d][Batch %d/%d] %.1f clouds/s Loss = %.4f Acc = %.4f lr = %.6f' % (
                        epoch, config.max_epoch, idx + 1, len(train_loader), n * bs * world / (time.time() - t0),
                        vals[0], vals[1], optimizer.param_groups[0]['lr']))
        for item in (scheduler if isinstance(scheduler, list) else [scheduler]):
            if item is not None:
                item.step(epoch)
        if epoch % max(int(getattr(args, 'val_freq', 1)), 1) == 0:
            metrics = validate_fn(base_model, test_loader, epoch, config, args, log=log)
            better = metrics.better_than(best_metrics)
            if better:
                best_metrics = metrics
                builder.save_checkpoint(model, optimizer, epoch, metrics, best_metrics, 'ckpt-best', args)
            if vote and (metrics.acc > 92.1 or (better and metrics.acc > 91)):          # runner_finetune.py:254-262
                metrics_vote = validate_vote(base_model, test_loader, epoch, config, args, log=log, fps_cache=vote_fps)
                if metrics_vote.better_than(best_metrics_vote):
                    best_metrics_vote = metrics_vote
                    builder.save_checkpoint(model, optimizer, epoch, metrics, best_metrics_vote, 'ckpt-best_vote', args)
        builder.save_checkpoint(model, optimizer, epoch, metrics, best_metrics, 'ckpt-last', args)
    return model


@torch.no_grad()
def extract_svm_features(base_model, loader, npoints):
    """runner_finetune.py:955-987 / :1000-1031: per batch FPS to point_all = min(npoints, N) points -- no oversampling in
    this protocol --, the host draw np.random.choice(point_all, npoints, False) (a permutation of the FPS order), the
    gather, the eval forward -> (features (n, C), labels (n,)) on the device."""
    feats, labels = [], []
    for _, _, data in loader:
        points = resample(data[0].cuda(), npoints, point_all=npoints)
        feats.append(base_model(points).detach())
        labels.append(data[1].cuda().view(-1))
    return torch.cat(feats, 0), torch.cat(labels, 0)


def _frozen_features(args, config, log):
    """The part svm_classification and task_affinity share: one process, the train and val loaders, the model frozen in
    eval mode, extract_svm_features over both -> (train features, labels, test features, labels) on the device; the two
    feature shapes are logged as the reference prints them."""
    rank, world = dist_utils.get_dist_info()
    device = torch.device('cuda', torch.cuda.current_device())
    from .graph_step import use_created_stream
    use_created_stream(device)
    bs = config.total_bs // world
    train_loader = _loader(config.dataset.train, device, args.seed + rank, rank, world, bs,
                           getattr(args, 'steps_per_epoch', None))
    test_loader = _loader(config.dataset.val, device, args.seed, rank, world, bs)
    _log_sources(log, train_loader, test_loader)
    base_model = builder.model_builder(config.model)
    if getattr(args, 'resume', False):
        builder.resume_model(base_model, args)
    elif args.ckpts is not None:
        base_model.load_model_from_ckpt(args.ckpts, log=log)               # runner_finetune.py:921-922
    else:
        log('Training from scratch')                                       # (:924: the model keeps its constructor's init)
    base_model = base_model.to(device).eval()
    feats_train, labels_train = extract_svm_features(base_model, train_loader, config.npoints)
    log(str(tuple(feats_train.shape)))
    feats_test, labels_test = extract_svm_features(base_model, test_loader, config.npoints)
    log(str(tuple(feats_test.shape)))
    return feats_train, labels_train, feats_test, labels_test


def svm_classification(args, config, log=print):
    """runner_finetune.py:902-1049: the features of the train loader (its short last batch dropped), then of the val
    loader, from the frozen model in eval mode; SVC(C=c, kernel='linear') for c = 10**i, i in range(-3, 3) (svm_ops:
    the gfx950 solver, or PDAE_SVM=sklearn); the reference's lines -- the running best per c, then its
    '[Validation] EPOCH' line, whose epoch field is the last c -- -> Acc_Metric(best test accuracy, a fraction)."""
    from . import svm_ops
    feats_train, labels_train, feats_test, labels_test = _frozen_features(args, config, log)
    log('SVM backend: %s' % svm_ops.backend())
    max_acc, c = 0, None
    for c, acc in zip(svm_ops.SVM_CS, svm_ops.accuracies(feats_train, labels_train, feats_test, labels_test)):
        if max_acc < acc:
            max_acc = acc
        log('%s %s' % (c, max_acc))
    log('[Validation] EPOCH: %d  acc = %.4f' % (c, max_acc))
    return Acc_Metric(max_acc)


def task_affinity(args, config, log=print):
    """runner_finetune.py:1052-1269: the features of the train and the val loader from the frozen model, as for
    svm_classification; then the linear probe of affinity_ops (300 epochs of AdamW under the cosine schedule: one
    launch per step on csrc/affinity.hip, or PDAE_AFFINITY=torch) and the reference's line, which
    parse_test_res.py --taskaffinity reads -> (accuracy as a fraction, mean test cross-entropy)."""
    from . import affinity_ops
    feats_train, labels_train, feats_test, labels_test = _frozen_features(args, config, log)
    log('Affinity backend: %s' % affinity_ops.backend())
    acc, loss = affinity_ops.task_affinity_loss(feats_train, labels_train, feats_test, labels_test)
    log('[Validation] Acc: %.4f  loss = %.4f' % (acc, loss))
    return acc, loss
