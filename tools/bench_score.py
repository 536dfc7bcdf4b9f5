"""Cost of scoring a fitted model (Engine.score: per-cell and per-gene NLL on the GPU) on BASELINE configs[2]'s shape --
68 579 x 20 000, zinb-conddisp 64-32-64, device-synthesised counts as bench.py makes them.  Three figures:

  (a) Engine.score over all cells;
  (b) Engine.eval_loss_sum over the same rows on the same engine, in the same chunks -- the validation pass, "about one
      forward pass" (its call and its kernels predate score);
  (c) what a user did for the same numbers before: predict(return_info=True) to the host, then the element-wise ZINB
      likelihood with numpy / scipy and its two sums.  Run on a slice of the cells and SCALED to all of them (the output
      says so): the full pass moves three cells x genes fp32 matrices (16 GB) through the host.

(a) and (b): device events on the stream around the call, one warm-up, then the two alternate; the median of the rounds.
  python tools/bench_score.py [--cells 68579] [--genes 20000] [--rounds 5] [--chunk 1024,4096] [--slice 4096] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dca_amd import prep, synth                                 # noqa: E402
from dca_amd._anndata import MiniAnnData                        # noqa: E402
from dca_amd.network import AE_types                            # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402
from oracle import zinb_np as Z                                 # noqa: E402


def _timed(fn):
    """Milliseconds of fn's work on the current stream, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=68579)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--chunk', type=str, default='1024,4096', help='rows per chunk (1024: what a fit leaves reserved)')
    ap.add_argument('--slice', type=int, default=4096, help='cells of the host-side route (c)')
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda')
    n, G = args.cells, args.genes
    ops = HipOps()
    Y = synth.generate_counts(n, G, device=dev)
    counts = prep.cell_counts(ops, Y, n, G)
    sf = counts / counts.median()
    X, norm = prep.transform(ops, Y, n, G, sf, True, True, None, return_norm=True)
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
    net.build()
    eng = net.engine
    eng.attach_device_data(X, Y, sf, norm=norm)
    res = {'workload': 'BASELINE configs[2] shape: %d x %d, zinb-conddisp 64-32-64, batch norm, synthetic counts' % (n, G),
           'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'score_ms': {}, 'eval_loss_sum_ms': {},
           'score_over_eval_loss_sum': {}, 'rounds_ms': {}}
    scale = 1.0 / (float(n) * G)
    for chunk in (int(c) for c in args.chunk.split(',')):
        eng.reserve(chunk)

        def score():
            return eng.score(chunk=chunk)

        def val():
            eng.acc.zero_()
            eng.eval_loss_sum(0, n, scale, chunk)
            return eng.acc[1]
        _, s0 = _timed(score)                                   # warm-up of every shape (the ragged last chunk included)
        _, v0 = _timed(val)
        total, v = float(s0['cell'].sum().item()) * scale, float(v0.item())
        assert abs(total - v) <= 1e-5 * abs(v), (total, v)      # the two passes add up the same likelihood
        ts, tv = [], []
        for _ in range(args.rounds):
            ts.append(_timed(score)[0])
            tv.append(_timed(val)[0])
        key = 'chunk%d' % chunk
        ms, mv = sorted(ts)[len(ts) // 2], sorted(tv)[len(tv) // 2]
        res['score_ms'][key], res['eval_loss_sum_ms'][key] = round(ms, 3), round(mv, 3)
        res['score_over_eval_loss_sum'][key] = round(ms / mv, 3)
        res['rounds_ms'][key] = {'score': [round(t, 3) for t in ts], 'eval_loss_sum': [round(t, 3) for t in tv]}
        res['mean_nll'] = total
    # (c) the host route on a slice, through the public predict()
    m = min(args.slice, n)
    ad = MiniAnnData(X[:m, :G].cpu().numpy(), obs=pd.DataFrame({'size_factors': sf[:m].cpu().numpy()},
                                                                 index=pd.RangeIndex(m).astype(str)))
    y_host = Y[:m, :G].cpu().numpy()
    host = []
    for _ in range(2):                                          # the first pass locks the staging pages
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.predict(ad, mode='denoise', return_info=True, copy=True)
        t1 = time.perf_counter()
        el = Z.zinb_nll(y_host, out.X, out.obsm['X_dca_dispersion'], out.obsm['X_dca_dropout'], 0.0)
        cell, gene = el.sum(axis=1, dtype=np.float64), el.sum(axis=0, dtype=np.float64)
        t2 = time.perf_counter()
        host.append((t1 - t0, t2 - t1))
    res['host_route'] = {'cells_measured': m, 'predict_s': round(host[-1][0], 3), 'likelihood_s': round(host[-1][1], 3),
                         'scaled_to_cells': n, 'scaled': True,
                         'scaled_total_s': round((host[-1][0] + host[-1][1]) * n / m, 2),
                         'note': 'measured on %d cells and multiplied by %d / %d; numpy fp32 arrays as predict() returns '
                                 'them, scipy gammaln' % (m, n, m)}
    res['host_route']['mean_nll_slice'] = float(cell.sum() / (m * G))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
