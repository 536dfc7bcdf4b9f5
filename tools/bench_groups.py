"""Cost of the per-group moments of the denoised expression (Engine.group_moments -> dcahip_group_moments) on BASELINE
configs[2]'s shape -- 68 579 x 20 000, zinb-conddisp 64-32-64, device-synthesised counts as bench.py makes them, 16 groups.
Four figures:

  (a) Engine.group_moments over all cells;
  (b) Engine.score over the same rows on the same engine, in the same chunks -- the yardstick: the same forward pass per
      chunk, then a kernel that reads up to three planes and the targets where (a) reads one plane;
  (c) dcahip_group_moments alone on one chunk's plane: time per call and plane bytes (B x G x 4) / time, next to the
      6.0 - 6.3 TB/s a streaming read reaches on this chip; the calls rotate over copies of the plane that together exceed
      the Infinity Cache several times, so each reads its plane from HBM;
  (d) what a user did for the same numbers before: predict() to the host, then numpy mean and variance per group.  Run on
      a slice of the cells and SCALED to all of them (the output says so).

(a) and (b): device events on the stream around the call, one warm-up, then the two alternate; the median of the rounds.
(c): events around `--reps` back-to-back calls, divided; the median of the rounds.
  python tools/bench_groups.py [--cells 68579] [--genes 20000] [--groups 16] [--rounds 5] [--chunk 1024,4096] [--out FILE]"""
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


def _timed(fn):
    """Milliseconds of fn's work on the current stream, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=68579)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--groups', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20, help='back-to-back kernel calls per timed window of (c)')
    ap.add_argument('--chunk', type=str, default='1024,4096', help='rows per chunk (1024: what a fit leaves reserved)')
    ap.add_argument('--slice', type=int, default=4096, help='cells of the host-side route (d)')
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda')
    n, G, K = args.cells, args.genes, args.groups
    ops = HipOps()
    Y = synth.generate_counts(n, G, device=dev)
    counts = prep.cell_counts(ops, Y, n, G)
    sf = counts / counts.median()
    X, norm = prep.transform(ops, Y, n, G, sf, True, True, None, return_norm=True)
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
    net.build()
    eng = net.engine
    eng.attach_device_data(X, Y, sf, norm=norm)
    codes = np.random.default_rng(0).integers(0, K, size=n).astype(np.int32)
    codes[::50] = -1                                            # a fiftieth of the cells in no group
    codes_dev = torch.as_tensor(codes).to(dev)
    res = {'workload': 'BASELINE configs[2] shape: %d x %d, zinb-conddisp 64-32-64, batch norm, synthetic counts, %d groups'
                       % (n, G, K),
           'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'group_moments_ms': {}, 'score_ms': {},
           'group_moments_over_score': {}, 'rounds_ms': {}, 'kernel': {}}
    for chunk in (int(c) for c in args.chunk.split(',')):
        eng.reserve(chunk)

        def moments():
            return eng.group_moments(codes, K, no_sf=True, log1p=True, chunk=chunk)

        def score():
            return eng.score(chunk=chunk)
        _, m0 = _timed(moments)                                 # warm-up of every shape (the ragged last chunk included)
        _timed(score)
        assert int(m0['count'].sum().item()) == int((codes >= 0).sum()) and bool(torch.isfinite(m0['sum']).all())
        tm, ts = [], []
        for _ in range(args.rounds):
            tm.append(_timed(moments)[0])
            ts.append(_timed(score)[0])
        key = 'chunk%d' % chunk
        res['group_moments_ms'][key], res['score_ms'][key] = round(_median(tm), 3), round(_median(ts), 3)
        res['group_moments_over_score'][key] = round(_median(tm) / _median(ts), 3)
        res['rounds_ms'][key] = {'group_moments': [round(t, 3) for t in tm], 'score': [round(t, 3) for t in ts]}
        # (c) the kernel alone on the pre-activation plane of the first chunk
        b = min(chunk, n)
        o = eng._range_rows(0, b)
        eng._heads_forward(b, eng._hidden_forward(b, ('range', o), False))
        # copies of the plane buffer to rotate over: between two reads of a plane more than the 256 MiB of the Infinity Cache
        # is read from the others, so every call streams its plane from HBM
        plane_bytes = b * G * 4
        copies = [eng.A] + [eng.A.clone() for _ in range(max(2, -(-600_000_000 // plane_bytes)))]
        planes = [eng._plane(A, 'mean') for A in copies]
        f64 = dict(dtype=torch.float64, device=dev)
        s1, s2 = torch.zeros(K, G, **f64), torch.zeros(K, G, **f64)
        ws = torch.zeros(ops.group_moments_workspace_doubles(b, G, K), **f64)
        for name, flags in (('log1p_no_sf', 48), ('denoised', 0)):
            def kernel():
                for r in range(args.reps):
                    ops.group_moments(planes[r % len(planes)], eng.lay.ldA, eng.sf[o:], codes_dev, b, G, K, flags, s1, s2, G, ws)
            _timed(kernel)
            tk = [_timed(kernel)[0] / args.reps for _ in range(args.rounds)]
            ms = _median(tk)
            res['kernel']['%s_%s' % (key, name)] = {
                'rows': b, 'ms': round(ms, 4), 'plane_bytes': plane_bytes, 'planes_rotated': len(planes),
                'plane_TB_per_s': round(plane_bytes / (ms * 1e-3) / 1e12, 3),
                'rounds_ms': [round(t, 4) for t in tk]}
        del copies, planes
    res['streaming_read_TB_per_s_reference'] = '6.0-6.3'
    # (d) the host route on a slice, through the public predict()
    m = min(args.slice, n)
    ad = MiniAnnData(X[:m, :G].cpu().numpy(), obs=pd.DataFrame({'size_factors': sf[:m].cpu().numpy()},
                                                                 index=pd.RangeIndex(m).astype(str)))
    host = []
    for _ in range(2):                                          # the first pass locks the staging pages
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.predict(ad, mode='denoise', copy=True)
        t1 = time.perf_counter()
        x = np.log1p(np.asarray(out.X, np.float64) / ad.obs['size_factors'].values[:, None])
        mean = np.stack([x[codes[:m] == k].mean(axis=0) for k in range(K)])
        var = np.stack([x[codes[:m] == k].var(axis=0, ddof=1) for k in range(K)])
        t2 = time.perf_counter()
        host.append((t1 - t0, t2 - t1))
    res['host_route'] = {'cells_measured': m, 'predict_s': round(host[-1][0], 3), 'numpy_s': round(host[-1][1], 3),
                         'scaled_to_cells': n, 'scaled': True,
                         'scaled_total_s': round((host[-1][0] + host[-1][1]) * n / m, 2),
                         'note': 'measured on %d cells and multiplied by %d / %d; predict() to the host, log1p and per-group '
                                 'mean / variance in numpy float64' % (m, n, m)}
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
