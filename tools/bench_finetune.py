"""Times the classification fine-tuning step (point_transformer.PointTransformer on the ModelNet40 fine-tuning config,
B=32, N=1024, G=64; with --model DGCNN dgcnn_cls.DGCNN on cfgs/finetune_modelnet_dgcnn_smooth.yaml) and prints ONE
JSON line:

  graphed / eager   ms per optimisation step (forward, cross-entropy, backward, clip coefficient, AdamW) and clouds/s,
                    HIP events around `--steps` steps after `--warmup` untimed ones; the input batch is resampled in front
                    of the timed region (the loader's work is not part of the step)
  grad_norm_clip_us / adamw_step_gscale_us   one launch pair of each over the flat gradient / parameter buffers, HIP
                    events around `--reps` back-to-back calls
  kernels_per_step  device kernels of one eager step (torch.profiler), null where the profiler records none
  head_loss_us      (DGCNN only) the head and the smoothed loss, forward and backward, on the encoder's (B, 1024)
                    feature: HIP events around `--reps` eager calls (host-bound: ~30 launches); head_loss_kernels and
                    head_loss_kernel_us its device kernels and their summed device time, kernel_us_per_step that sum
                    for the whole eager step

  adamw_segments_all_us   (with --part) the ONE segmented launch over part all's two ranges, beside adamw_two_launch_us,
                    the two launches it generalises, on scratch copies of the flat buffers, `--reps` calls each,
                    three alternating rounds (min / max of the rounds: the run-to-run spread)

--part only_new | diff_lr times the frozen-encoder protocols (optimizer.part; only_new runs in train() + set_bn_eval);
--model PointTransformerLinearClassification is the linear protocol's model.

    timeout -k 10 300 python tools/bench_finetune.py [--model DGCNN] [--part only_new] [--steps 30 --warmup 10 --reps 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


CONFIGS = {'PointTransformer': 'finetune_modelnet_transferring_features.yaml', 'DGCNN': 'finetune_modelnet_dgcnn_smooth.yaml',
           'PointTransformerLinearClassification': 'finetune_modelnet_linear_classification.yaml'}


def _kernels(fn):
    """(device kernels fn() launches, their summed device time in us) from torch.profiler, and None or the error's type
    name; the counts are None where the profiler records no kernel."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type.name == 'CUDA']
        return (len(ev) or None, round(sum(e.time_range.elapsed_us() for e in ev), 1) if ev else None), None
    except Exception as e:                           # a profiler without a device tracer
        return (None, None), type(e).__name__


def _events_ms(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--model', choices=sorted(CONFIGS), default='PointTransformer')
    p.add_argument('--part', choices=['all', 'only_new', 'diff_lr'], default=None, help='optimizer.part (default: the config\'s)')
    a = p.parse_args(argv)
    import torch
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.finetune_ops import GradNormClip
    from point_dae_amd.graph_step import GraphedClassifierStep, use_created_stream
    from point_dae_amd.runner_finetune import resample, set_train_mode, train_step
    from point_dae_amd.synthetic import labelled_clouds

    config = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', CONFIGS[a.model]))
    if a.part is not None:
        config.optimizer.part = a.part
    part = config.optimizer.get('part', 'all')
    B, N = a.batch, config.npoints
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    use_created_stream(dev)
    x, y = labelled_clouds(B, 2048, seed=0, classes=3)
    pts = resample(torch.from_numpy(x).to(dev), N)
    labels = torch.from_numpy(y).to(dev)
    if a.model != 'DGCNN':
        out = dict(workload='finetune_modelnet', model=a.model, part=part, batch=B, npoints=N, num_group=config.model.num_group,
                   tokens=config.model.num_group + 1, depth=config.model.depth, steps=a.steps, warmup=a.warmup)
    else:
        out = dict(workload='finetune_modelnet_dgcnn', part=part, batch=B, npoints=N, smoothloss=bool(config.model.smoothloss),
                   steps=a.steps, warmup=a.warmup)

    def setup():
        torch.manual_seed(0)
        net = set_train_mode(builder.model_builder(config.model).to(dev), part)
        model = FlatDataParallel(net)
        opt, _ = builder.build_opti_sche(model, config)
        model.zero_grad()
        return model, opt, GradNormClip(model.flat_grad, config.grad_norm_clip)

    model, opt, clip = setup()
    for _ in range(a.warmup):
        train_step(model, opt, clip, pts, labels)
    ms = _events_ms(lambda: train_step(model, opt, clip, pts, labels), a.steps)
    out['eager'] = dict(ms_per_step=round(ms, 4), clouds_per_s=round(B / ms * 1e3, 1))
    (out['kernels_per_step'], kernel_us), err = _kernels(lambda: train_step(model, opt, clip, pts, labels))
    if err:
        out['kernels_per_step_error'] = err
    if a.model == 'DGCNN':
        out['kernel_us_per_step'] = kernel_us
    if a.model == 'DGCNN':
        net = model.module
        with torch.no_grad():
            feat = net.dgcnn_encoder.forward_rows(pts)
        feat.requires_grad_()

        def head_loss():
            loss, _ = net.get_loss_acc(net.head(feat), labels)
            loss.backward()
        for _ in range(a.warmup):
            head_loss()
        out['head_loss_us'] = round(_events_ms(head_loss, a.reps) * 1e3, 2)
        (out['head_loss_kernels'], out['head_loss_kernel_us']), _ = _kernels(head_loss)
        model.zero_grad()

    model, opt, clip = setup()
    step = GraphedClassifierStep(model, opt, clip, B, N)
    for _ in range(a.warmup):
        step(pts, labels)
    ms = _events_ms(lambda: step(pts, labels), a.steps)
    out['graphed'] = dict(ms_per_step=round(ms, 4), clouds_per_s=round(B / ms * 1e3, 1))

    coef = clip()
    out['flat_params'] = model.flat_grad.numel()
    out['grad_norm_clip_us'] = round(_events_ms(clip, a.reps) * 1e3, 2)
    out['grad_norm_clip_GBps'] = round(4.0 * model.flat_grad.numel() / (out['grad_norm_clip_us'] * 1e-6) / 1e9, 1)
    out['adamw_step_gscale_us'] = round(_events_ms(lambda: opt.step(grad_scale=coef), a.reps) * 1e3, 2)
    if a.part is not None:
        from point_dae_amd import _lib
        m = model
        bufs = [m.flat_param.clone(), m.flat_grad.clone(), torch.zeros_like(m.flat_param), torch.zeros_like(m.flat_param)]
        kw = config.optimizer.kwargs
        lr = float(kw.lr)
        ranges = [m.no_decay_range + (0.0,), m.decay_range + (float(kw.weight_decay),)]

        def two():
            for lo, hi, wd in ranges:
                _lib.call('pdae_adamw_step_gscale', bufs[0], hi - lo, *[t[lo:].data_ptr() for t in bufs], lr, 0.9, 0.999,
                          1e-8, wd, 1, coef.data_ptr())

        def one():
            _lib.adamw_step_segments(*bufs, [(lo, hi - lo, lr, wd) for lo, hi, wd in ranges], 0.9, 0.999, 1e-8, 1, coef)
        two(), one()
        rounds = [(_events_ms(two, a.reps) * 1e3, _events_ms(one, a.reps) * 1e3) for _ in range(3)]
        out['adamw_two_launch_us'] = [round(min(r[0] for r in rounds), 2), round(max(r[0] for r in rounds), 2)]
        out['adamw_segments_all_us'] = [round(min(r[1] for r in rounds), 2), round(max(r[1] for r in rounds), 2)]
        out['adamw_launches_per_step'] = 2 if part == 'all' else -(-sum(len(g['segments']) for g in opt.param_groups) // 8)
        if part != 'all':
            out['adamw_segments'] = sum(len(g['segments']) for g in opt.param_groups)
    out['device'] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
