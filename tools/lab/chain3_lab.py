"""LAB (round 6, VERDICT r5 item 1, stage gate): a GEMM -> GEMM seam inside ONE persistent launch (band-local counters,
tools/lab/chain3_lab.hip) against the same two products as two launches, at the encoder MLP pair's size.
    bash tools/lab/build_chain3_lab.sh && gpurun -- python tools/lab/chain3_lab.py
Prints: bit-equality of both results, time per pair from graph replays (HIP events), and the in-kernel timeline of the
chained launch (s_memrealtime stamps per block and unit): when the fc2 units start, how long they wait, what the seam costs."""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from point_dae_amd import _lib  # noqa: E402
from point_dae_amd.rows import rows_gemm  # noqa: E402
from point_dae_amd.graph_step import use_created_stream  # noqa: E402

lab = ctypes.CDLL(os.path.join(ROOT, 'tools', 'lab', 'libchain3_lab.so'))
vp, i32 = ctypes.c_void_p, ctypes.c_int
lab.lab_chain3.argtypes = [i32] * 5 + [vp] * 8 + [i32, i32, vp]
lab.lab_two_launches.argtypes = [i32] * 5 + [vp] * 5 + [vp]
MAXU = 4


def stream():
    return torch.cuda.current_stream().cuda_stream


def graph_ms(fn, per_graph=20, replays=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        for _ in range(per_graph):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / replays / per_graph * 1e3      # us per pair


def main():
    use_created_stream()
    torch.manual_seed(0)
    N1, K1, N2, S = 1536, 384, 384, 3
    blocks = 256
    for T in (23, 13, 32):
        M = 128 * T
        X = torch.randn(M, K1, device='cuda')
        W1 = torch.randn(N1, K1, device='cuda') * K1 ** -0.5
        W2 = torch.randn(N2, N1, device='cuda') * N1 ** -0.5
        H0, Y0 = torch.empty(M, N1, device='cuda'), torch.empty(S, M, N2, device='cuda')
        H1, Y1 = torch.full((M, N1), float('nan'), device='cuda'), torch.full((S, M, N2), float('nan'), device='cuda')
        bands = (M + 127) // 128
        cnt = torch.zeros(bands * S, dtype=torch.int32, device='cuda')
        sync = torch.zeros(4, dtype=torch.int32, device='cuda')
        stamps = torch.zeros(blocks * MAXU * 4, dtype=torch.int64, device='cuda')

        def two():
            rc = lab.lab_two_launches(M, N1, K1, N2, S, X.data_ptr(), W1.data_ptr(), H0.data_ptr(), W2.data_ptr(), Y0.data_ptr(), stream())
            assert rc == 0, rc

        def chain(waits=1):
            rc = lab.lab_chain3(M, N1, K1, N2, S, X.data_ptr(), W1.data_ptr(), H1.data_ptr(), W2.data_ptr(), Y1.data_ptr(),
                                cnt.data_ptr(), sync.data_ptr(), stamps.data_ptr(), waits, blocks, stream())
            assert rc == 0, rc

        def shipped():      # what the step launches today: the planned tile shapes (128 x 192 for fc1, slabs for fc2)
            h = rows_gemm(X, W1)
            cfg, splits, sb = _lib.rows_gemm_plan(M, N2, N1, False, 8)
            y = torch.empty(max(splits, 1), M, N2, device='cuda')
            _lib.call('pdae_rows_gemm', h, M, N2, N1, _lib.ptr(h), _lib.ptr(W2), 0, None, 0, None, _lib.ptr(y), cfg, splits, sb)
            return y
        two()
        chain()
        torch.cuda.synchronize()
        ok_h, ok_y = torch.equal(H0, H1), torch.equal(Y0, Y1)
        ref = (X.double() @ W1.double().t()) @ W2.double().t()
        err = (Y1.sum(0).double() - ref).abs().max().item() / ref.abs().max().item()
        # 200 chained launches back to back, results re-checked: a stale read shows up under load, not on the first launch
        bad = 0
        for _ in range(200):
            Y1.fill_(float('nan'))
            chain()
            bad += int(not torch.equal(Y0, Y1))
        t_two, t_chain, t_ship = graph_ms(two), graph_ms(chain), graph_ms(shipped)
        t_free = graph_ms(lambda: chain(0))
        chain()
        torch.cuda.synchronize()
        print(f'M = {M} (T_vis {T}): H equal {ok_h}, Y equal {ok_y}, 200 repeats differing {bad}, give-ups {int(sync[2])}, err vs fp64 {err:.1e}')
        print(f'   two launches (128x128 tiles both) {t_two:6.1f} us | shipped plan (two launches) {t_ship:6.1f} us | ONE launch, chained '
              f'{t_chain:6.1f} us | one launch without the waits (wrong results: what is left is packing) {t_free:6.1f} us')
        # timeline of the last chained launch (100 MHz ticks -> us, relative to the earliest block start)
        st = stamps.view(blocks, MAXU, 4).cpu().double()
        t0 = st[:, 0, 0].min()
        n1 = (M // 128) * (N1 // 128)
        rows = []
        for b in range(blocks):
            for k in range(MAXU):
                if st[b, k, 2] > 0:
                    rows.append((int(st[b, k, 3]), (st[b, k, 0] - t0) / 100, (st[b, k, 1] - t0) / 100, (st[b, k, 2] - t0) / 100))
        f1 = [r for r in rows if r[0] < n1]
        f2 = [r for r in rows if r[0] >= n1]
        if f1 and f2:
            import statistics as stt
            print('   timeline (us from the first block\'s start): fc1 tiles end %.1f .. %.1f (median %.1f); fc2 units: start %.1f .. %.1f, '
                  'wait for the dependency median %.2f max %.2f, body median %.1f, launch ends %.1f' % (
                      min(r[3] for r in f1), max(r[3] for r in f1), stt.median(r[3] for r in f1),
                      min(r[1] for r in f2), max(r[1] for r in f2), stt.median(r[2] - r[1] for r in f2), max(r[2] - r[1] for r in f2),
                      stt.median(r[3] - r[2] for r in f2), max(r[3] for r in rows)))
            # the seam as a unit sees it: time from the LAST of its four producers' publish to its own first instruction behind the wait
            pub = {r[0]: r[3] for r in f1}
            seam = []
            for r in f2:
                v = r[0] - n1
                bs = v // (N2 // 128)
                s_, band = bs % S, bs // S
                prod = [pub.get(band * (N1 // 128) + j) for j in range(4 * s_, 4 * s_ + 4)]
                if all(p is not None for p in prod) and r[1] <= max(prod):        # it really waited
                    seam.append(r[2] - max(prod))
            if seam:
                print('   hand-off latency (last producer published -> consumer past its acquire), units that waited: n %d median %.2f us max %.2f us'
                      % (len(seam), stt.median(seam), max(seam)))


if __name__ == '__main__':
    main()


# ---------------------------------------------------------------------------------------------
# The four heavy phases of an encoder block's forward (qkv -> proj -> fc1 -> fc2) as ONE table-driven persistent launch
# (chain4_kernel) against four launches; unit orders: phase-major, band-group wavefronts, band-major.
def unit_table(T, S, order, G=8):
    import numpy as np
    B = T                                        # bands of 128 rows
    c0 = lambda b: b
    c1 = lambda b: B + b
    c2 = lambda b, s: 2 * B + b * S + s
    per_phase = {0: [], 1: [], 2: [], 3: []}
    for b in range(B):
        for j in range(9):
            per_phase[0].append((b, (0, b * 9 + j, 0, -1, 0, c0(b) if j < 3 else -1)))
        for j in range(3):
            per_phase[1].append((b, (1, b * 3 + j, 0, c0(b), 3, c1(b))))
        for j in range(12):
            per_phase[2].append((b, (2, b * 12 + j, 0, c1(b), 3, c2(b, j // 4))))
        for s in range(S):
            for j in range(3):
                per_phase[3].append((b, (3, b * 3 + j, s, c2(b, s), 4, -1)))
    units = []
    if order == 'phase':
        for ph in range(4):
            units += [u for _, u in per_phase[ph]]
    elif order == 'band':
        for b in range(B):
            for ph in range(4):
                units += [u for bb, u in per_phase[ph] if bb == b]
    else:                                         # wavefront over groups of G bands: (group g, phase p) in slot g + p
        ngroups = (B + G - 1) // G
        for slot in range(ngroups + 3):
            for ph in (3, 2, 1, 0):               # later phases first: they are on the critical path
                g = slot - ph
                if 0 <= g < ngroups:
                    units += [u for bb, u in per_phase[ph] if bb // G == g]
    return torch.tensor(np.array(units, dtype=np.int32)), 2 * B + B * S


def main4():
    use_created_stream()
    torch.manual_seed(1)
    S, blocks, MAXU4 = 3, 256, 6
    lab.lab_chain4.argtypes = [i32, i32] + [vp] * 10 + [i32] + [vp] * 3 + [i32, i32, vp]
    lab.lab_four_launches.argtypes = [i32, i32] + [vp] * 9 + [vp]
    for T in (23, 13, 32):
        M = 128 * T
        X = torch.randn(M, 384, device='cuda')
        Wq, Wp = torch.randn(1152, 384, device='cuda') * 384 ** -0.5, torch.randn(384, 384, device='cuda') * 384 ** -0.5
        W1, W2 = torch.randn(1536, 384, device='cuda') * 384 ** -0.5, torch.randn(384, 1536, device='cuda') * 1536 ** -0.5
        def bufs(fill):
            mk = lambda *s: torch.full(s, fill, device='cuda')
            return mk(M, 1152), mk(M, 384), mk(M, 1536), mk(S, M, 384)
        Q0, P0, H0, Y0 = bufs(0.0)
        Q1, P1, H1, Y1 = bufs(float('nan'))
        sync = torch.zeros(4, dtype=torch.int32, device='cuda')
        stamps = torch.zeros(blocks * MAXU4 * 4, dtype=torch.int64, device='cuda')

        def four():
            rc = lab.lab_four_launches(M, S, X.data_ptr(), Wq.data_ptr(), Q0.data_ptr(), Wp.data_ptr(), P0.data_ptr(), W1.data_ptr(),
                                       H0.data_ptr(), W2.data_ptr(), Y0.data_ptr(), stream())
            assert rc == 0, rc

        def shipped():
            q = rows_gemm(X, Wq)
            outs = []
            for a, w in ((q[:, :384].contiguous() if False else q, Wp),):
                pass
            # proj reads the q third: the library's entry takes a contiguous operand, so the shipped comparison uses a
            # (M, 384) operand of its own (same shape, same work)
            cfg, sp, sb = _lib.rows_gemm_plan(M, 384, 384, False, 8)
            p_ = torch.empty(max(sp, 1), M, 384, device='cuda')
            _lib.call('pdae_rows_gemm', X, M, 384, 384, _lib.ptr(X), _lib.ptr(Wp), 0, None, 0, None, _lib.ptr(p_), cfg, sp, sb)
            h = rows_gemm(p_[0], W1)
            cfg, sp, sb = _lib.rows_gemm_plan(M, 384, 1536, False, 8)
            y = torch.empty(max(sp, 1), M, 384, device='cuda')
            _lib.call('pdae_rows_gemm', h, M, 384, 1536, _lib.ptr(h), _lib.ptr(W2), 0, None, 0, None, _lib.ptr(y), cfg, sp, sb)
            return y
        four()
        torch.cuda.synchronize()
        t_four, t_ship = graph_ms(four), graph_ms(shipped)
        print(f'M = {M} (T_vis {T}): four launches (128x128 tiles) {t_four:6.1f} us | shipped plans (four launches) {t_ship:6.1f} us')
        for order, G in (('phase', 0), ('wave', 8), ('wave', 4), ('band', 0)):
            table, ncnt = unit_table(T, S, order, G)
            table = table.cuda().contiguous()
            cnt = torch.zeros(ncnt, dtype=torch.int32, device='cuda')
            sync.zero_()

            def chain(waits=1):
                rc = lab.lab_chain4(M, S, X.data_ptr(), Wq.data_ptr(), Q1.data_ptr(), Wp.data_ptr(), P1.data_ptr(), W1.data_ptr(),
                                    H1.data_ptr(), W2.data_ptr(), Y1.data_ptr(), table.data_ptr(), table.shape[0], cnt.data_ptr(),
                                    sync.data_ptr(), stamps.data_ptr(), waits, blocks, stream())
                assert rc == 0, rc
            bad = 0
            for _ in range(50):
                Y1.fill_(float('nan'))
                chain()
                bad += int(not (torch.equal(Y0, Y1) and torch.equal(H0, H1) and torch.equal(P0, P1) and torch.equal(Q0, Q1)))
            t_chain = graph_ms(chain)
            chain()
            torch.cuda.synchronize()
            st = stamps.view(blocks, MAXU4, 4).cpu().double()
            t0 = st[:, 0, 0].min()
            waits = [(st[b, k, 1] - st[b, k, 0]).item() / 100 for b in range(blocks) for k in range(MAXU4) if st[b, k, 2] > 0]
            end = max((st[b, k, 2] - t0).item() / 100 for b in range(blocks) for k in range(MAXU4) if st[b, k, 2] > 0)
            import statistics as stt
            print(f'   ONE launch, order {order:5s}{("/" + str(G)) if G else "  "}: {t_chain:6.1f} us  ({table.shape[0]} units; 50 repeats differing {bad}, '
                  f'give-ups {int(sync[2])}; in-kernel: launch ends {end:5.1f} us, waiting per unit mean {stt.mean(waits):.2f} max {max(waits):.1f} us, '
                  f'sum of waits per block {sum(waits) / blocks:.1f} us)')


if __name__ == '__main__' and os.environ.get('CHAIN4', '1') == '1':
    main4()
