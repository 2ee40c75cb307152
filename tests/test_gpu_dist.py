"""Multi-rank path on the GPU box: two processes (both on cuda:0 -- the box has one
GPU -- with the gloo backend, which carries CUDA tensors through the host) run the
hipGraph-replayed step + flat-gradient all-reduce + fused AdamW.  Checks what the
8-GPU RCCL run relies on: replicas start identical (broadcast), stay identical after
every update, and the loss goes down.  RCCL itself cannot be exercised with one GPU."""
import os
import socket

import pytest

import proc_util
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_env(rank, world, port):
    """Rendezvous of a spawned rank: loopback only (gloo otherwise resolves the box's hostname, which need not resolve),
    and a rank that is stuck dumps every thread's stack and exits instead of hanging the suite."""
    import faulthandler
    faulthandler.dump_traceback_later(240, exit=True)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK='0', GLOO_SOCKET_IFNAME='lo', HSA_ENABLE_IPC_MODE_LEGACY='0')


def _init(backend, rank, world):
    import datetime
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))


def _spawn(fn, args, nprocs, limit=180):
    """mp.spawn with a bounded join: ranks still alive after `limit` seconds are killed.  One re-run on such a
    time-out, with a warning -- a stuck rendezvous once stalled the whole suite for 19 minutes on one box and never
    again in ten loops; a failure of the ranks themselves (exception, wrong result) is never retried."""
    import time
    import warnings
    for attempt in (0, 1):
        ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
        deadline = time.monotonic() + limit
        timed_out = False
        while not ctx.join(timeout=5):
            if time.monotonic() > deadline:
                timed_out = True
                for proc in ctx.processes:
                    if proc.is_alive():
                        proc.kill()
                for proc in ctx.processes:
                    proc.join(10)
                break
        if not timed_out:
            return
        if attempt == 0:
            warnings.warn('%s: ranks still running after %d s, killed; running them once more' % (fn.__name__, limit))
            args = tuple(_free_port() if i == 1 else a for i, a in enumerate(args))     # a fresh rendezvous port
    raise AssertionError('%s: ranks still running after %d s, twice' % (fn.__name__, limit))


def _worker(rank, world, port, out, split=None, det=False, arith=None):
    _rank_env(rank, world, port)
    torch.cuda.set_device(0)
    _init('gloo', rank, world)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import sys
    sys.path.insert(0, root)
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.graph_step import GraphedTrainStep, use_created_stream
    use_created_stream()
    if det:
        from point_dae_amd import _lib
        _lib.set_deterministic(True)
        # Two PROCESSES time-sharing one GPU is this test's stand-in for two GPUs.  Round 4 ran this check on the
        # fp32-input kernels only: next to a process running the exact-split GEMMs a rank got wrong partial sums out of
        # embed.hip's conv1_backward_weight_kernel.  Root cause (round 5, tools/xproc_repro.hip): hipcc's SLP vectoriser
        # had packed that kernel's accumulations into v_pk_*_f32 with operand selects, which gfx950 computes wrongly in
        # lanes 16-31 while another wave of the CU runs bf16 MFMAs beside ds_read_b128 -- the library is built with
        # -fno-slp-vectorize now, and the check runs in BOTH arithmetics (`arith`).
        if arith is not None:
            _lib.set_gemm_arith(arith)
    from point_dae_amd.misc import set_random_seed
    from point_dae_amd.synthetic import shapenet_like_clouds
    config = cfg_from_yaml_file(os.path.join(
        root, 'cfgs', 'pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml'))
    config.model.transformer_config.depth = 2
    config.model.transformer_config.decoder_depth = 1
    set_random_seed(7 + rank)                       # different init per rank: broadcast must fix it
    net = builder.model_builder(config.model).cuda().train()
    model = FlatDataParallel(net)
    opt, _ = builder.build_opti_sche(model, config)
    B = 8
    x = torch.from_numpy(shapenet_like_clouds(B * 2, 1024, seed=10 + rank)).cuda().split(B)
    step = GraphedTrainStep(model, opt, config, B, 1024, warmup_eager=1, split=split)
    losses = []
    for i in range(6):
        losses.append(step(x[i % 2])[0].item())
    flat = [torch.empty_like(model.flat_param) for _ in range(world)]
    dist.all_gather(flat, model.flat_param)
    same = torch.equal(flat[0], flat[1])
    if rank == 0:
        # parameters by NAME: the flat layout is the same in both modes, but do not rely on it
        torch.save({'same': same, 'losses': losses, 'graphs': len(step.graphs), 'split': step.split,
                    'early_bytes': 4 * (model.early_range[1] - model.early_range[0]),
                    'late_bytes': 4 * sum(b - a for a, b in model.late_ranges),
                    'params': {n: p.detach().cpu().clone() for n, p in net.named_parameters()}}, out)
    dist.destroy_process_group()


def test_two_ranks_graphed_step_stay_in_sync(tmp_path):
    out = str(tmp_path / 'r.pt')
    _spawn(_worker, (2, _free_port(), out), 2)
    r = torch.load(out)
    assert r['same'], 'replicas diverged'
    assert r['graphs'] >= 1
    assert r['losses'][-1] < r['losses'][0], r['losses']


@pytest.mark.parametrize('arith', [1, 0], ids=['bf16x3', 'f32mfma'])
def test_two_ranks_split_step_overlapped_allreduce(tmp_path, arith):
    """The two-phase step (graph 1 = forward + Transformer backward, async all-reduce of the Transformer
    slice, graph 2 = embedder backward under it, then the embedder's two small slices): replicas stay
    bit-identical, and -- in deterministic mode -- every parameter after six updates equals the
    single-phase step's (one flat all-reduce after one graph) bit for bit, in the default exact-split
    arithmetic (arith 1) and on the fp32-input kernels (arith 0)."""
    res = {}
    for split in (True, False):
        out = str(tmp_path / ('r%d.pt' % split))
        _spawn(_worker, (2, _free_port(), out, split, True, arith), 2)
        res[split] = torch.load(out)
        assert res[split]['same'], 'replicas diverged (split=%s)' % split
        assert res[split]['split'] == split and res[split]['graphs'] >= 1
    assert res[True]['early_bytes'] > 10 * res[True]['late_bytes'] > 0   # depth 2+1 here; 58x at full depth
    assert res[True]['losses'] == res[False]['losses'], (res[True]['losses'], res[False]['losses'])
    for n, p in res[True]['params'].items():
        assert torch.equal(p, res[False]['params'][n]), n


@pytest.mark.parametrize('launcher', ['torchrun', 'self'])
def test_bench_two_ranks_code_path(launcher):
    """bench.py's N > 1 path end to end (launcher env, broadcast, graphed steps with the gradient
    all-reduce, rank-0-only roofline probe, max-over-ranks timing) with two gloo ranks sharing the GPU --
    RCCL needs one device per rank, so this checks the code path, not the collective's speed.
    'self': `python bench.py --gpus 2` with NO launcher must start the two ranks itself."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PDAE_BENCH_BACKEND='gloo', GLOO_SOCKET_IFNAME='lo')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    tail = [os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '2', '--batch', '8',
            '--probe-steps', '2', '--full']
    if launcher == 'torchrun':
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
               '--master-addr', '127.0.0.1', '--master-port', str(_free_port())] + tail
    else:
        cmd = [sys.executable] + tail
    r = proc_util.run(cmd, 600, env=env, cwd=root)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['config']['global_batch'] == 16 and d['scaling'] == 'weak'
    assert d['replicas_in_sync'] is True and d['config']['grad_allreduce'].startswith('Transformer slice')
    assert d['value'] > 0 and d['roofline'] is not None and 'cpu_baseline' not in d
    assert d['rccl_ranks'] == 0          # gloo ranks: not an RCCL measurement, and the line says so


def test_bench_refuses_more_ranks_than_gpus():
    """`--gpus 8` on a 1-GPU box must fail, not print an n_gpus=1 line (RCCL: one device per rank)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'PDAE_BENCH_BACKEND')}
    want = torch.cuda.device_count() + 1
    r = proc_util.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(want), '--steps', '1',
                       '--warmup', '0'], 300, env=env, cwd=root)
    assert r.returncode != 0 and '{"metric"' not in r.stdout, (r.returncode, r.stdout[-500:])


def _nccl_one_rank(rank, world, port, out):
    _rank_env(0, 1, port)
    torch.cuda.set_device(0)
    _init('nccl', 0, 1)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import sys
    sys.path.insert(0, root)
    from point_dae_amd import graph_step
    from point_dae_amd.data_parallel import FlatDataParallel
    from point_dae_amd.graph_step import use_created_stream
    use_created_stream()
    net = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.LayerNorm(64), torch.nn.Linear(64, 8)).cuda()
    model = FlatDataParallel(net)
    g = torch.Generator(device='cuda').manual_seed(0)
    model.flat_grad.copy_(torch.randn(model.flat_grad.shape, device='cuda', generator=g))
    want = model.flat_grad.clone()
    n = model.flat_grad.numel()
    # the slices of the split step: async all-reduce on RCCL's stream behind an event on the compute stream
    (w1, d1), (w2, d2) = graph_step._start_average(model, 0, n // 2), graph_step._start_average(model, n // 2, n)
    busy = torch.randn(1 << 20, device='cuda').sum()             # compute-stream work issued while RCCL runs
    for (a, b), (w, d) in (((0, n // 2), (w1, d1)), ((n // 2, n), (w2, d2))):
        w.wait()
        if d:
            model.flat_grad[a:b].div_(1)
    torch.cuda.synchronize()
    graph_step._average_gradients(model)                          # the single-phase path
    torch.cuda.synchronize()
    torch.save({'equal': torch.equal(model.flat_grad, want), 'avg_in_collective': not (d1 or d2),
                'backend': dist.get_backend(), 'busy': float(busy)}, out)
    dist.destroy_process_group()


def test_rccl_backend_runs_the_average_path(tmp_path):
    """The `nccl` backend of this torch build IS RCCL.  One rank (the box has one GPU) through the exact calls of the
    multi-GPU step -- graph_step._start_average on slices (async_op, ReduceOp.AVG) and _average_gradients: RCCL links,
    initialises a communicator, accepts AVG on fp32 views of the flat gradient buffer and returns it unchanged."""
    out = str(tmp_path / 'rccl.pt')
    _spawn(_nccl_one_rank, (1, _free_port(), out), 1)
    r = torch.load(out)
    assert r['backend'] == 'nccl'
    assert r['equal'], 'an average over one rank changed the gradients'
    assert r['avg_in_collective'], 'ReduceOp.AVG was rejected by this RCCL build: the step falls back to SUM + divide'


def _sync_bn_worker(rank, world, port, out):
    _rank_env(rank, world, port)
    torch.cuda.set_device(0)
    _init('gloo', rank, world)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import sys
    sys.path.insert(0, root)
    from point_dae_amd.graph_step import use_created_stream
    from point_dae_amd.point_cae_transformer import Encoder
    use_created_stream()
    torch.manual_seed(3)
    enc = Encoder(384).cuda().train()                              # same seed: same weights on both ranks
    for bn in (enc.first_conv[1], enc.second_conv[1]):
        torch.nn.init.uniform_(bn.weight, 0.5, 1.5), torch.nn.init.uniform_(bn.bias, -0.2, 0.2)
    g = torch.Generator().manual_seed(11)
    pts = (torch.randn(64, 32, 3, generator=g) * 0.2).cuda()        # 64 groups; rank r owns [32 r, 32 r + 32)
    groups = torch.arange(0, 32, 2, dtype=torch.int32, device='cuda')   # visible groups of a half (local ids)
    w = torch.randn(16, 384, generator=g).cuda()
    sync = torch.nn.SyncBatchNorm.convert_sync_batchnorm(Encoder(384).cuda().train())
    sync.load_state_dict(enc.state_dict())
    mine = pts[32 * rank:32 * rank + 32].reshape(1, 32, 32, 3)
    tok = sync(mine, groups=groups)
    (tok * w).sum().backward()
    grads = torch.cat([p.grad.reshape(-1) for p in sync.parameters()])
    dist.all_reduce(grads)                                          # the sum over the replicas (DDP would average)
    toks = [torch.empty_like(tok) for _ in range(world)]
    dist.all_gather(toks, tok.detach())
    if rank == 0:
        # one process, the whole batch: (b) the same layer-by-layer path with plain BatchNorm modules -- what SyncBN must
        # reproduce -- and (c) the FUSED embedder (per-"replica" statistics over all 64 groups)
        from point_dae_amd.patch_embed import patch_embed_layerwise
        allg = torch.cat([groups, groups + 32])
        names = [n for n, _ in enc.named_parameters()]
        plain = Encoder(384).cuda().train()
        plain.load_state_dict(enc.state_dict())
        lay = patch_embed_layerwise(pts, plain.first_conv, plain.second_conv, allg)
        (lay * torch.cat([w, w])).sum().backward()
        lay_g = [p.grad.reshape(-1).cpu() for p in plain.parameters()]
        ref = enc(pts.reshape(1, 64, 32, 3), groups=allg)
        (ref * torch.cat([w, w])).sum().backward()
        ref_g = [p.grad.reshape(-1).cpu() for p in enc.parameters()]
        sizes = [g.numel() for g in lay_g]
        torch.save({'tok': torch.cat(toks).cpu(), 'lay': lay.detach().cpu(), 'ref': ref.detach().cpu(),
                    'g': list(grads.cpu().split(sizes)), 'lay_g': lay_g, 'ref_g': ref_g, 'names': names,
                    'rm': sync.second_conv[1].running_mean.cpu(), 'lay_rm': plain.second_conv[1].running_mean.cpu(),
                    'ref_rm': enc.second_conv[1].running_mean.cpu(),
                    'rv': sync.first_conv[1].running_var.cpu(), 'lay_rv': plain.first_conv[1].running_var.cpu(),
                    'ref_rv': enc.first_conv[1].running_var.cpu()}, out)
    dist.destroy_process_group()


def test_two_ranks_sync_bn_statistics_span_the_replicas(tmp_path):
    """--sync_bn (runner_pretrain.py:81-83, collective C4): the converted embedder takes the layer-by-layer path
    (patch_embed.patch_embed_layerwise) whose SyncBatchNorm modules reduce the batch statistics over the ranks.
    Two ranks with half of the groups each reproduce ONE process running the fused embedder on all groups: tokens,
    running estimates and (summed over the ranks) every parameter gradient."""
    out = str(tmp_path / 'sbn.pt')
    _spawn(_sync_bn_worker, (2, _free_port(), out), 2)
    r = torch.load(out)

    gmax = max(g.abs().max().item() for g in r['lay_g'])

    dead = ('first_conv.0.bias', 'second_conv.0.bias')      # in front of a BatchNorm: the true gradient is exactly zero

    def worst(a, b):
        # error of a parameter's gradient against ITS max (floored at 1e-3 of the largest gradient)
        return max(((x - y).abs().max().item() / max(y.abs().max().item(), 1e-3 * gmax), n)
                   for x, y, n in zip(a, b, r['names']) if n not in dead)
    for x, y, n in zip(r['g'], r['lay_g'], r['names']):
        if n in dead:                                       # only rounding residue on either side
            assert x.abs().max().item() <= 1e-4 * gmax and y.abs().max().item() <= 1e-4 * gmax, n
    # SyncBN across two ranks == plain BatchNorm over the whole batch, same layer-by-layer code (tight)
    assert (r['tok'] - r['lay']).abs().max().item() <= 1e-5 * r['lay'].abs().max().item()
    assert torch.allclose(r['rm'], r['lay_rm'], rtol=1e-5, atol=1e-7) and torch.allclose(r['rv'], r['lay_rv'], rtol=1e-5, atol=1e-7)
    assert worst(r['g'], r['lay_g'])[0] <= 5e-4, worst(r['g'], r['lay_g'])      # (fp32 reassociation: measured 1.2e-4)
    # and the layer-by-layer path == the fused embedder (the two conv biases in front of a BatchNorm excepted: the fused
    # path returns exactly zero for them, the layer-wise one their rounding residue -- both ~0 against the others)
    assert (r['lay'] - r['ref']).abs().max().item() <= 2e-4 * r['ref'].abs().max().item()
    assert torch.allclose(r['lay_rm'], r['ref_rm'], rtol=1e-4, atol=1e-6) and torch.allclose(r['lay_rv'], r['ref_rv'], rtol=1e-4, atol=1e-6)
    scale = max(g.abs().max().item() for g in r['ref_g'])
    for a, b, n in zip(r['lay_g'], r['ref_g'], r['names']):
        if n in ('first_conv.0.bias', 'second_conv.0.bias'):
            assert a.abs().max().item() <= 1e-3 * scale and b.abs().max().item() == 0.0, n
        else:
            # (two implementations, 64 groups, random loss weights: a max-pool winner that 1 ulp of GEMM rounding
            # resolves the other way moves that channel's gradient to another row -- single elements of conv4's weight
            # gradient then differ by O(1) while everything else agrees to 1e-5; both paths are within 8e-3 of the CPU
            # oracle Encoder on such inputs, tools/lab/embed_paths.py.  Hence the L2 norm, which a handful of
            # re-routed elements cannot move.)
            rel = (a - b).double().norm().item() / max(b.double().norm().item(), 1e-3 * scale)
            assert rel <= 5e-2, (n, rel)
