"""Cost of the gene cross-products behind the gene-gene correlation of the denoised expression (Engine.gene_gram ->
dcahip_gram).  Two parts:

  (1) the kernel alone on one chunk: 4 096 rows of a 20 000-column fp32 plane (uniform random values), G = 512, 2 048 and
      8 192 genes gathered from it (a random subset, in the plane's column order as `dca --genecorr` passes it, and once more
      shuffled), against the composition a user could write today in the same process:
          D = X[:, cols].double() - shift;  torch.mm(D.T, D);  D.sum(0)
      Both add up the same numbers; their results are compared before they are timed.  Reported per shape: milliseconds of
      both, the ratio baseline / kernel (>= 1: the kernel is no slower), and the kernel's fp64 rate on the G (G + 1) B
      operations of the triangle it computes, as a fraction of the 78.6 TFLOP/s fp64 figure of the spec sheet (a datasheet
      value; nothing in this project has measured the chip's fp64 peak).
  (2) end to end on BASELINE configs[2]'s shape (68 579 x 20 000, zinb-conddisp 64-32-64, device-synthesised counts as
      bench.py makes them): Engine.gene_gram with 2 048 genes over all cells, next to Engine.group_moments (16 groups) over
      the same rows on the same engine in the same chunks (informational: the forward pass is shared), and next to the host
      route, predict() + np.corrcoef, run on a slice of the cells and SCALED to all of them (the output says so; rough).

Device events on the stream around windows of back-to-back calls (as many as fill about a tenth of a second), the two
sides alternating, the median of `--rounds` windows, every shape warmed up first.
  python tools/bench_genecorr.py [--rows 4096] [--plane 20000] [--genes 512,2048,8192] [--rounds 5] [--out FILE]"""
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

SPEC_FP64_TFLOPS = 78.6


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


def kernel_part(ops, args, dev):
    B, W = args.rows, args.plane
    f64 = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    X = torch.rand(B, W, device=dev, generator=gen) * 1.5 + 0.5
    out = {}
    for G in (int(g) for g in args.genes.split(',')):
        for order in ('sorted', 'shuffled'):
            rng = np.random.default_rng(G)
            pick = rng.permutation(W)[:G]
            pick = np.sort(pick) if order == 'sorted' else pick
            cols32 = torch.as_tensor(pick.astype(np.int32)).to(dev)
            cols64 = cols32.long()
            shift = X[:1024].index_select(1, cols64).double().mean(dim=0)
            nws = ops.gram_workspace_doubles(B, G)
            ws = torch.zeros(nws, **f64) if nws else None
            cross, dsum = torch.zeros(G, G, **f64), torch.zeros(G, **f64)

            def ours():
                ops.gram(X, W, cols32, None, shift, B, G, cross, G, dsum, ws)

            def base():
                D = X[:, cols64].double() - shift
                return torch.mm(D.T, D), D.sum(0)
            ours()
            ref_c, ref_d = base()
            torch.cuda.synchronize()
            scale = float(ref_c.diagonal().max())
            err = float((cross - ref_c).abs().max()) / scale
            assert err < 1e-12 and torch.equal(cross, cross.T), (G, order, err)      # the same sums before any is timed
            assert float((dsum - ref_d).abs().max()) < 1e-9
            t1 = max(_timed(ours)[0], _timed(base)[0], 1e-3)
            reps = int(min(200, max(3, np.ceil(100.0 / t1))))

            def window(fn):
                def run():
                    for _ in range(reps):
                        fn()
                return run
            _timed(window(ours))
            _timed(window(base))
            to, tb = [], []
            for _ in range(args.rounds):
                to.append(_timed(window(ours))[0] / reps)
                tb.append(_timed(window(base))[0] / reps)
            mo, mb = _median(to), _median(tb)
            flops = float(G) * (G + 1) * B
            out['G%d_%s' % (G, order)] = {
                'rows': B, 'genes': G, 'plane_columns': W, 'cols_order': order, 'calls_per_window': reps,
                'kernel_ms': round(mo, 4), 'baseline_ms': round(mb, 4), 'baseline_over_kernel': round(mb / mo, 3),
                'kernel_fp64_TFLOPs': round(flops / (mo * 1e-3) / 1e12, 2),
                'fraction_of_spec_fp64': round(flops / (mo * 1e-3) / 1e12 / SPEC_FP64_TFLOPS, 3),
                'max_rel_difference': err,
                'rounds_ms': {'kernel': [round(t, 4) for t in to], 'baseline': [round(t, 4) for t in tb]}}
            del cross, ref_c
    return out


def end_to_end_part(ops, args, dev):
    n, G, g, K, chunk = args.cells, args.plane, args.e2e_genes, 16, args.chunk
    Y = synth.generate_counts(n, G, device=dev)
    counts = prep.cell_counts(ops, Y, n, G)
    sf = counts / counts.median()
    X, norm = prep.transform(ops, Y, n, G, sf, True, True, None, return_norm=True)
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
    net.build()
    eng = net.engine
    eng.attach_device_data(X, Y, sf, norm=norm)
    eng.reserve(chunk)
    cols = np.sort(np.random.default_rng(1).permutation(G)[:g])
    codes = np.random.default_rng(0).integers(0, K, size=n).astype(np.int32)

    def gram():
        return eng.gene_gram(cols, no_sf=True, log1p=True, chunk=chunk)

    def moments():
        return eng.group_moments(codes, K, no_sf=True, log1p=True, chunk=chunk)
    _, r0 = _timed(gram)                                        # warm-up of every shape (the ragged last chunk included)
    _timed(moments)
    assert r0['count'] == n and bool(torch.isfinite(r0['cross']).all()) and torch.equal(r0['cross'], r0['cross'].T)
    tg, tm = [], []
    for _ in range(args.rounds):
        tg.append(_timed(gram)[0])
        tm.append(_timed(moments)[0])
    res = {'cells': n, 'plane_columns': G, 'genes': g, 'chunk': chunk, 'gene_gram_ms': round(_median(tg), 2),
           'group_moments_ms': round(_median(tm), 2), 'gene_gram_over_group_moments': round(_median(tg) / _median(tm), 2),
           'rounds_ms': {'gene_gram': [round(t, 2) for t in tg], 'group_moments': [round(t, 2) for t in tm]}}
    # the host route on a slice, through the public predict()
    m = min(args.slice, n)
    ad = MiniAnnData(X[:m, :G].cpu().numpy(), obs=pd.DataFrame({'size_factors': sf[:m].cpu().numpy()},
                                                                 index=pd.RangeIndex(m).astype(str)))
    host = []
    for _ in range(2):                                          # the first pass locks the staging pages
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.predict(ad, mode='denoise', copy=True)
        t1 = time.perf_counter()
        x = np.log1p(np.asarray(out.X, np.float64)[:, cols] / ad.obs['size_factors'].values[:, None])
        r = np.corrcoef(x, rowvar=False)
        t2 = time.perf_counter()
        host.append((t1 - t0, t2 - t1))
    assert r.shape == (g, g)
    res['host_route'] = {'cells_measured': m, 'predict_s': round(host[-1][0], 3), 'corrcoef_s': round(host[-1][1], 3),
                         'scaled_to_cells': n, 'scaled': True,
                         'scaled_total_s': round((host[-1][0] + host[-1][1]) * n / m, 2),
                         'note': 'rough: measured on %d cells and multiplied by %d / %d; predict() to the host, log1p and '
                                 'np.corrcoef of the %d genes in float64' % (m, n, m, g)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--plane', type=int, default=20000)
    ap.add_argument('--genes', type=str, default='512,2048,8192')
    ap.add_argument('--cells', type=int, default=68579)
    ap.add_argument('--e2e-genes', type=int, default=2048)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--slice', type=int, default=4096, help='cells of the host-side route')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-end-to-end', action='store_true')
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda')
    ops = HipOps()
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'spec_fp64_TFLOPs': SPEC_FP64_TFLOPS, 'spec_note': 'datasheet figure, not measured in this project',
           'kernel': kernel_part(ops, args, dev)}
    if not args.skip_end_to_end:
        res['end_to_end'] = end_to_end_part(ops, args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
