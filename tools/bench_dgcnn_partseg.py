"""DGCNNPartSeg's evaluation forward at the protocol's shapes (cfgs/segmentation_shapenetpart_dgcnn.yaml): 16 clouds of
2048 points, seeded weights, eval mode -- the figures of DESIGN.md §7:

    block     ONE two-layer EdgeConv (conv3 + conv4 on x1 with its graph): the stacked-weight row GEMM +
              pdae_edge2_eval_forward (csrc/edge2_eval.hip) against the block as the reference writes it (the per-edge
              tensor by index gather, two conv + affine + LeakyReLU layers, amax) on kernels that predate it.  The graph
              and the stacked weight are made ahead of the window under both forms.
    encoder   DGCNNPartSeg.encode: three graphs, three EdgeConvs, conv6 and the pool, both forms
    forward   the whole forward (encoder + head) under PDAE_PARTSEG=hip against PDAE_PARTSEG=layers

The two forms of a pair are warmed up and then alternated ROUNDS times in one process; a figure is CALLS calls between two
device events, divided by CALLS, CALLS chosen so that a window lasts at least WINDOW_MS; (median, min, max) over the
rounds, in ms.  `spread` is max - min of the BASELINE's (the layers form's) rounds: a difference smaller than that is not
a difference, and `hip_is_faster` says whether the whole forward's medians differ by more than it.  The outputs of the two
forms are compared at the timed size first, on each form's own graphs and on one set of graphs.  One JSON object.

    python tools/bench_dgcnn_partseg.py [ROUNDS] [B]          # default 5 rounds at B = 16, N = 2048
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import weights  # noqa: E402
from point_dae_amd import _lib, builder  # noqa: E402,F401
from point_dae_amd import dgcnn_partseg as D  # noqa: E402
from point_dae_amd.config import cfg_from_yaml_file  # noqa: E402
from point_dae_amd.datasets import synthetic_part_shapes  # noqa: E402
from point_dae_amd.graph_step import use_created_stream  # noqa: E402
from point_dae_amd.registry import MODELS  # noqa: E402
from point_dae_amd.rows import bn_eval_affine, empty, rows_gemm  # noqa: E402

N = 2048
WINDOW_MS = 200.0


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def alternate(fns, rounds, warm=2):
    """-> per form (median, min, max) ms over `rounds` alternated windows, and the calls per window."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    calls = [max(1, int(WINDOW_MS / max(window(fn, 1), 1e-3)) + 1) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(rounds):
        for fn, c, acc in zip(fns, calls, times):
            acc.append(window(fn, c))
    return [(round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)) for t in times], calls


def under(mode, fn):
    def run():
        os.environ['PDAE_PARTSEG'] = mode
        return fn()
    return run


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def pair(out, name, hip, layers, rounds):
    (h, l), calls = alternate([hip, layers], rounds)
    out[name + '_hip_ms'], out[name + '_layers_ms'], out[name + '_calls'] = h, l, calls
    out[name + '_layers_spread_ms'] = round(l[2] - l[1], 3)
    out[name + '_speedup'] = round(l[0] / h[0], 2)
    return h, l


@torch.no_grad()
def bench(B, rounds, model):
    clouds, cls, _ = synthetic_part_shapes(B, N, seed=3)
    pts = torch.stack([torch.from_numpy(c[:N]) for c in clouds]).cuda()[:, :, :3].contiguous()
    cls = torch.from_numpy(cls).cuda()
    out = {'B': B, 'N': N, 'k': min(D.K_GRAPH, N), 'rounds': rounds, 'window_ms': WINDOW_MS}
    # ---- one fused block ------------------------------------------------------------------------------------------
    cap = {}
    under('hip', lambda: model(pts, cls, capture=cap))()
    enc = model.dgcnn_encoder
    x1, idx = cap['x1'].clone(), cap['graphs'][1].clone()
    s1, t1, _, _ = bn_eval_affine(enc.bn3)
    s2, t2, _, _ = bn_eval_affine(enc.bn4)
    stacked = empty((128, 64), x1)
    _lib.call('pdae_edge_weight_stack', x1, 64, 64, 64, _lib.ptr(enc.conv3[0].weight.contiguous()), _lib.ptr(stacked))
    w4 = enc.conv4[0].weight.reshape(64, 64).contiguous()
    cat = empty((B * N, 192), x1)

    def block_hip():
        return D.edge2_eval(rows_gemm(x1, stacked), idx, s1, t1, w4, s2, t2, out2=cat, col=64)

    def block_layers():
        return model._edgeconv_layers(x1, idx, 1, enc.conv3, enc.conv4, s1, t1, cat)
    out['block_hip_vs_layers_rel'] = rel(block_hip(), block_layers())
    out['block_edge_tensor_mb'] = round(B * N * out['k'] * 64 * 4 / 1e6, 1)
    pair(out, 'block', block_hip, block_layers, rounds)
    # ---- the encoder ----------------------------------------------------------------------------------------------
    a, b = model.encode(pts, True), model.encode(pts, False)
    out['encoder_hip_vs_layers_rel'] = (rel(a[0], b[0]), rel(a[1], b[1]))
    pair(out, 'encoder', lambda: model.encode(pts, True), lambda: model.encode(pts, False), rounds)
    # ---- the whole forward ----------------------------------------------------------------------------------------
    hip, layers = under('hip', lambda: model(pts, cls)), under('layers', lambda: model(pts, cls))
    out['forward_hip_vs_layers_rel'] = rel(hip(), layers())
    # each form selects its graphs on its own features: a row whose k-th and (k+1)-th neighbour lie within the rounding of
    # the distance may pick the other one, and the logits follow.  With ONE set of graphs the two forms are compared as
    # arithmetic: the hip run's graphs injected into both.
    ch, cl = {}, {}
    a = under('hip', lambda: model(pts, cls, capture=ch))()
    under('layers', lambda: model(pts, cls, capture=cl))()
    same = [(ch['graphs'][l].sort(-1)[0] == cl['graphs'][l].sort(-1)[0]).all(-1).double().mean().item() for l in range(3)]
    out['graph_rows_equal_share'] = [round(v, 5) for v in same]
    b = under('layers', lambda: model(pts, cls, graphs=ch['graphs']))()
    out['forward_hip_vs_layers_rel_same_graphs'] = rel(a, b)
    h, l = pair(out, 'forward', hip, layers, rounds)
    out['clouds_per_s_hip'] = round(B / (h[0] * 1e-3), 1)
    out['clouds_per_s_layers'] = round(B / (l[0] * 1e-3), 1)
    out['hip_is_faster'] = bool(l[0] - h[0] > out['forward_layers_spread_ms'])
    print(json.dumps(out), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    use_created_stream()
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'segmentation_shapenetpart_dgcnn.yaml')).model
    model = weights.fill_state(MODELS.build(cfg), 7).cuda().eval()
    bench(B, rounds, model)


if __name__ == '__main__':
    main()
