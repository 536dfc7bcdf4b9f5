"""Cost of the Wilcoxon rank-sum integers (dcahip_ranksum, Engine.rank_sums) at the product's shapes: 68 579 cells with
512, 4 096 and 20 000 genes, and 1 000 000 x 2 048; 16 groups, every group against the rest.  Per shape:

  (a) dcahip_ranksum alone on a gene-major buffer of positive, heavy-tailed values (expf of a normal draw, as a denoised
      mean looks), and the bytes it has to move: per labelled cell 4 (histogram read) + 12 per sort pass that RUNS (read and
      write of a 4-byte key and a 2-byte code; the passes are counted from the data: a byte that is the same in all keys of a
      row is skipped) + 12 (the two scans), so `bound_ms` = bytes / `--stream-tb` (6.0 TB/s, a streaming read on this chip);
  (b) the same numbers composed from torch.sort(stable=True) on the same buffer plus torch scans (cummax / cummin /
      scatter_add), in blocks of genes that keep its int64 temporaries under ~1 GB -- the baseline on the device.  The two
      ALTERNATE in one process; the first block's results are compared for equality;
  (c) Engine.rank_sums end to end (forward pass over all cells, transpose, the kernel) on device-synthesised counts, as
      bench.py makes them, zinb-conddisp 64-32-64;
  (d) ROUGH: scipy.stats.rankdata on the host on a slice of the genes, scaled to all of them and divided by 16 threads'
      worth of genes.

Device events on the stream, one warm-up per shape, the median of `--rounds` (5).
  python tools/bench_ranksum.py [--shapes 68579x512,68579x4096,68579x20000,1000000x2048] [--groups 16] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dca_amd import prep, synth                                 # noqa: E402
from dca_amd.network import AE_types                            # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _order(codes, K):
    lab = np.flatnonzero(codes >= 0)
    order = lab[np.argsort(codes[lab], kind='stable')].astype(np.int32)
    counts = np.bincount(codes[lab], minlength=K)
    return order, np.r_[0, np.cumsum(counts)].astype(np.int32)


def _passes(buf, n, odev, block=256):
    """Sort passes the kernel runs per row, summed over the rows: the bytes of the key image that differ inside a row (at
    least one: a constant row is copied once)."""
    total = 0
    for g0 in range(0, buf.shape[0], block):
        u = buf[g0:g0 + block, :n].index_select(1, odev.long()).view(torch.int32)
        u = torch.where(u == -2 ** 31, torch.zeros_like(u), u)
        key = torch.where(u < 0, ~u, u | -2 ** 31)
        per_row = torch.zeros(key.shape[0], dtype=torch.int64, device=buf.device)
        for p in range(4):
            byte = (key >> (8 * p)) & 255
            per_row += (byte.max(dim=1).values != byte.min(dim=1).values).long()
        total += int(per_row.clamp(min=1).sum())
    return total


def _torch_ranks(buf, n, odev, code0, K, block):
    """rank2 and tie of every row, rest mode, from torch.sort and torch scans."""
    g, m = buf.shape[0], odev.numel()
    r2 = torch.zeros(g, K, dtype=torch.int64, device=buf.device)
    tie = torch.zeros(g, dtype=torch.int64, device=buf.device)
    pos = torch.arange(m, device=buf.device)
    for g0 in range(0, g, block):
        x = buf[g0:g0 + block, :n].index_select(1, odev.long())
        v, idx = torch.sort(x, dim=1, stable=True)
        c = code0[idx]
        head = torch.ones_like(v, dtype=torch.bool)
        head[:, 1:] = v[:, 1:] != v[:, :-1]
        tail = torch.ones_like(head)
        tail[:, :-1] = head[:, 1:]
        a = torch.cummax(torch.where(head, pos, -1), dim=1).values
        b = torch.cummin(torch.where(tail, pos + 1, m + 1).flip(1), dim=1).values.flip(1)
        r2[g0:g0 + block].scatter_add_(1, c, a + b + 1)
        t = torch.where(head, b - a, 0)
        tie[g0:g0 + block] = (t * t * t - t).sum(dim=1)
    return r2, tie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=str, default='68579x512,68579x4096,68579x20000,1000000x2048')
    ap.add_argument('--groups', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--stream-tb', type=float, default=6.0)
    ap.add_argument('--host-genes', type=int, default=8)
    ap.add_argument('--no-engine', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'ranksum_bench.json'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    K = args.groups
    ops = HipOps()
    res = {'device': torch.cuda.get_device_name(0), 'groups': K, 'rounds': args.rounds, 'mode': 'every group against the rest',
           'stream_TB_per_s_assumed': args.stream_tb, 'shapes': {}}
    for shape in args.shapes.split(','):
        n, G = (int(v) for v in shape.split('x'))
        codes = np.random.default_rng(0).integers(0, K, size=n).astype(np.int32)
        codes[::50] = -1                                            # a fiftieth of the cells in no group
        order, gstart = _order(codes, K)
        m = int(order.size)
        odev, gdev = torch.as_tensor(order).to(dev), torch.as_tensor(gstart).to(dev)
        code0 = torch.as_tensor(np.repeat(np.arange(K), np.diff(gstart))).to(dev)
        ldn = (n + 3) // 4 * 4
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        buf = torch.empty(G, ldn, dtype=torch.float32, device=dev)
        for g0 in range(0, G, 1024):
            buf[g0:g0 + 1024].normal_(0.0, 1.5, generator=gen).exp_()
        rank2 = torch.zeros(K, G, dtype=torch.int64, device=dev)
        tie = torch.zeros(K, G, dtype=torch.int64, device=dev)
        ws = torch.empty(ops.ranksum_workspace_bytes(G, n), dtype=torch.uint8, device=dev)
        block = max(1, min(G, (1 << 30) // (8 * m)))

        def kernel():
            ops.ranksum(buf, ldn, G, n, odev, m, gdev, K, -1, rank2, tie, G, ws)

        def composed():
            return _torch_ranks(buf, n, odev, code0, K, block)
        _timed(kernel)
        _, (t2, tt) = _timed(composed)
        same = bool(torch.equal(t2.t(), rank2)) and bool(torch.equal(tt, tie[0]))
        tk, tc = [], []
        for _ in range(args.rounds):
            tk.append(_timed(kernel)[0])
            tc.append(_timed(composed)[0])
        passes = _passes(buf, n, odev)
        nbytes = m * (16 * G + 12 * passes)
        entry = {'cells': n, 'genes': G, 'labelled_cells': m, 'kernel_ms': round(_median(tk), 3),
                 'kernel_rounds_ms': [round(t, 3) for t in tk], 'sort_passes_per_gene': round(passes / G, 3),
                 'bytes_moved': nbytes, 'bound_ms': round(nbytes / (args.stream_tb * 1e12) * 1e3, 3),
                 'kernel_TB_per_s': round(nbytes / (_median(tk) * 1e-3) / 1e12, 3),
                 'workspace_bytes': int(ws.numel()), 'torch_sort_composition_ms': round(_median(tc), 3),
                 'torch_rounds_ms': [round(t, 3) for t in tc], 'torch_gene_block': block,
                 'torch_over_kernel': round(_median(tc) / _median(tk), 3), 'results_equal': same}
        # a row of equal values costs what any row costs: the same shape, every value 1.5 (512 genes at most)
        gc = min(G, 512)
        const = torch.full((gc, ldn), 1.5, dtype=torch.float32, device=dev)

        def kernel_const():
            ops.ranksum(const, ldn, gc, n, odev, m, gdev, K, -1, rank2, tie, G, ws)

        def kernel_part():
            ops.ranksum(buf, ldn, gc, n, odev, m, gdev, K, -1, rank2, tie, G, ws)
        _timed(kernel_const)
        entry['all_equal_rows_ms'] = {'genes': gc, 'all_equal': round(_median([_timed(kernel_const)[0] for _ in range(args.rounds)]), 3),
                                      'continuous': round(_median([_timed(kernel_part)[0] for _ in range(args.rounds)]), 3)}
        del const
        # (d) the host, rough
        hg = min(args.host_genes, G)
        from scipy.stats import rankdata
        xh = buf[:hg, :n].cpu().numpy()[:, order]
        t0 = time.perf_counter()
        rankdata(xh, axis=1)
        th = time.perf_counter() - t0
        entry['host_rankdata_rough'] = {'genes_measured': hg, 'seconds_measured': round(th, 4), 'scaled': True,
                                        'scaled_16_threads_s': round(th / hg * G / 16, 2),
                                        'note': 'scipy.stats.rankdata alone on %d genes, times %d / %d, divided by 16: rough'
                                                % (hg, G, hg)}
        del buf, ws, t2, tt
        torch.cuda.empty_cache()
        # (c) end to end
        if not args.no_engine:
            Y = synth.generate_counts(n, G, device=dev)
            cnt = prep.cell_counts(ops, Y, n, G)
            sf = cnt / cnt.median()
            X, norm = prep.transform(ops, Y, n, G, sf, True, True, None, return_norm=True)
            net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
            net.build()
            eng = net.engine
            eng.attach_device_data(X, Y, sf, norm=norm)
            eng.reserve(4096)

            def e2e():
                return eng.rank_sums(codes, K, no_sf=True, log1p=True, chunk=4096)
            _, r = _timed(e2e)
            assert bool((r['rank2'].sum(dim=0) == m * (m + 1)).all())
            te = [_timed(e2e)[0] for _ in range(args.rounds)]
            entry['engine_rank_sums_ms'] = round(_median(te), 3)
            entry['engine_rounds_ms'] = [round(t, 3) for t in te]
            del eng, net, X, Y, r
            torch.cuda.empty_cache()
        res['shapes'][shape] = entry
        print(shape, json.dumps(entry), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
