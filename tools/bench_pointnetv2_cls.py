"""The graphed fine-tuning step of the PointNet++ classifier PointNetv2 (cfgs/finetune_modelnet_transferring_features_
PointNetv2.yaml: forward, smoothed loss, backward, clip coefficient as ONE hipGraph replay, then the fused AdamW) under both
settings of PDAE_SA_FIRST -- the figures of DESIGN.md §7:

    split     sa1 and sa2 run their first layer split by source point (csrc/sa_train.hip, sa_mlp.SplitFirstMLPMaxFunction)
    grouped   the grouped rows and sa_mlp.SharedMLPMaxFunction, the pretraining step's form

at B = 32 clouds of N = 1024 and of N = 2048 points, seeded weights and clouds.  The switch is read where the model is
built, so every setting runs in a process of its own: without --mode this program starts one child per setting, one after
the other, ROUNDS times alternately (grouped, split, grouped, split, ...), and never touches the GPU itself.  A child
captures the step, replays it WARM times, then times CALLS steps between two device events; the parent reports, per
shape and setting, (median, min, max) over the rounds in ms, the spread max - min, and the decision rule of DESIGN.md §7:
split is the default only if its median is lower than grouped's by more than grouped's spread.

    python tools/bench_pointnetv2_cls.py [ROUNDS]           # default 5 rounds
    python tools/bench_pointnetv2_cls.py --mode split       # one child: a JSON line with one figure per shape
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'cfgs', 'finetune_modelnet_transferring_features_PointNetv2.yaml')
B = 32
SHAPES = (1024, 2048)
WARM, CALLS = 20, 100
MODES = ('grouped', 'split')
CHILD_LIMIT = 240           # seconds


def child(mode):
    os.environ['PDAE_SA_FIRST'] = mode
    for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
        sys.path.insert(0, p)
    import torch
    import weights
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.finetune_ops import GradNormClip
    from point_dae_amd.graph_step import GraphedClassifierStep, use_created_stream
    from point_dae_amd.synthetic import labelled_clouds
    use_created_stream()
    config = cfg_from_yaml_file(CFG)
    out = {'mode': mode, 'B': B, 'calls': CALLS}
    for N in SHAPES:
        net = weights.fill_state(builder.model_builder(config.model), 7).cuda().train()
        assert net.sa_first == mode
        model = FlatDataParallel(net)
        opt, _ = builder.build_opti_sche(model, config)
        model.zero_grad()
        clip = GradNormClip(model.flat_grad, config.grad_norm_clip)
        step = GraphedClassifierStep(model, opt, clip, B, N)
        x, y = labelled_clouds(B, N, seed=3, classes=3)
        x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        for _ in range(WARM):
            loss, _ = step(x, y)
        torch.cuda.synchronize()
        assert step.graph is not None and bool(torch.isfinite(loss))
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(CALLS):
            loss, _ = step(x, y)
        end.record()
        end.synchronize()
        out['N%d_ms' % N] = start.elapsed_time(end) / CALLS
        out['N%d_loss' % N] = float(loss)
        del step, model, opt, net
    print(json.dumps(out), flush=True)


def main():
    if '--mode' in sys.argv:
        return child(sys.argv[sys.argv.index('--mode') + 1])
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    times = {(m, N): [] for m in MODES for N in SHAPES}
    for _ in range(rounds):
        for mode in MODES:
            cmd = ['timeout', '-k', '10', str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), '--mode', mode]
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0:              # nothing more is started behind a child that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode
            res = json.loads(r.stdout.strip().splitlines()[-1])
            for N in SHAPES:
                times[(mode, N)].append(res['N%d_ms' % N])
    for N in SHAPES:
        row = {'B': B, 'N': N, 'rounds': rounds, 'calls': CALLS}
        for mode in MODES:
            t = times[(mode, N)]
            row[mode + '_ms'] = (round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3))
            row[mode + '_spread_ms'] = round(max(t) - min(t), 3)
        gain = row['grouped_ms'][0] - row['split_ms'][0]
        row['split_gain_ms'] = round(gain, 3)
        row['split_is_default_by_the_rule'] = bool(gain > row['grouped_spread_ms'])
        print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main() or 0)
