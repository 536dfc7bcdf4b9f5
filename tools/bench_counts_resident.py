"""Counts-resident mode on one MI355X ("Counts-resident mode").

  python tools/bench_counts_resident.py --out profiles/counts_resident_bench.json
      1. ms/step at C3 (68 579 x 20 000, zinb-conddisp 64-32-64, B = 4096) in four forms: the default dense path, dense
         without the byte store, counts mode, counts mode gathering a byte tile (EngineConfig.counts_compact) -- the full
         training steps of the epoch replayed from hipGraphs, the forms INTERLEAVED over --rounds rounds (every round
         times every form once; the result holds every round, the median and the spread (max - min) / median);
      2. dcahip_csr_gather and the byte tile's gather (+ its per-step table) alone (graph replays, event-timed) against
         the HBM store bound of what they write;
      3. 20 steps on a matrix that cannot be dense-resident (default 1 500 000 x 30 000, 2 000 non-zeros per cell,
         synthesised on the device as CSR): ms/step and the peak device memory (--big-compact: with the byte tile).
  python tools/bench_counts_resident.py --gather-only [--compact]   (the gather's replays alone: for rocprofv3
                                                                     --kernel-trace --stats)
  python tools/bench_counts_resident.py --subset K --out profiles/counts_subset_bench.json
      dcahip_csr_gather_cols for K shuffled output genes beside dcahip_csr_gather at the same shape, in one process, the two
      interleaved over --rounds rounds (graph replays, event-timed): ms per call, the spread, their ratio.
  --forms a,b: only these forms (a run of an older checkout beside this one: --forms counts).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dca_amd import prep, synth                       # noqa: E402
from dca_amd.engine import Engine                     # noqa: E402
from dca_amd.ops import HipOps                        # noqa: E402
from dca_amd.train import _StepRunner                 # noqa: E402

STORE_TBPS = 6.1          # plain-store HBM rate of MI355X_MICROARCH (6.0-6.2 TB/s)


def dense_to_csr(Y, G, chunk=8192):
    """A resident dense count matrix -> CsrCounts (device, row chunks)."""
    n = Y.shape[0]
    dev = Y.device
    lens = torch.zeros(n, dtype=torch.int64, device=dev)
    for s in range(0, n, chunk):
        lens[s:s + chunk] = (Y[s:s + chunk, :G] != 0).sum(dim=1)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    nnz = int(indptr[-1].item())
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    values = torch.empty(nnz, dtype=torch.float32, device=dev)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        blk = Y[s:e, :G]
        rc = torch.nonzero(blk)                       # row-major order: sorted columns within each row
        a, b = int(indptr[s].item()), int(indptr[e].item())
        indices[a:b] = rc[:, 1].to(torch.int32)
        values[a:b] = blk[rc[:, 0], rc[:, 1]]
    return prep.CsrCounts(indptr, indices, values, n, G)


def synth_csr(n, G, per_row, dev, chunk=1 << 15):
    """n x G counts with per_row non-zeros in every row (one column per stride of G // per_row, hashed), values 1 .. 8."""
    stride = G // per_row
    indptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * per_row
    nnz = n * per_row
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    values = torch.empty(nnz, dtype=torch.float32, device=dev)
    k = torch.arange(per_row, dtype=torch.int64, device=dev)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        r = torch.arange(s, e, dtype=torch.int64, device=dev)[:, None]
        h = (r * 2654435761 + k * 40503 + 12345) % 1000003
        indices[s * per_row:e * per_row] = (k * stride + h % stride).to(torch.int32).reshape(-1)
        values[s * per_row:e * per_row] = (1 + (h // 7) % 8).to(torch.float32).reshape(-1)
    return prep.CsrCounts(indptr, indices, values, n, G)


def csr_normalisation(ops, csr):
    counts = prep.csr_cell_counts(ops, csr)
    sf = counts / counts.median()
    return sf, prep.csr_norm(ops, csr, sf, True, True)


def prepare_steps(eng, n_train, B):
    """Reserves, shuffles and captures: the runner whose replays timed_steps times."""
    dev = eng.dev
    steps = n_train // B
    eng.reserve(B)
    eng.perm = torch.randperm(n_train, device=dev).to(torch.int32)
    eng.hist = torch.zeros(steps + 1, dtype=torch.float32, device=dev)
    eng.clip = 5.0
    eng.set_lr(1e-3)
    runner = _StepRunner(eng, True)
    eng.cursor.zero_()
    runner.run(B, B, [B], B, steps)                   # eager first step + captures
    torch.cuda.synchronize()
    return runner, steps


def time_steps(eng, n_train, B, epochs):
    """ms per full training step: the full steps of `epochs` epochs replayed from hipGraphs (8 steps per launch)."""
    runner, steps = prepare_steps(eng, n_train, B)
    return timed_steps(eng, runner, B, steps, epochs)


def timed_steps(eng, runner, B, steps, epochs):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(epochs):
        eng.cursor.zero_()
        runner.run(B, B, [B], B, steps)
    t1.record()
    torch.cuda.synchronize()
    loss = float(eng.hist[:steps].mean().item())
    return t0.elapsed_time(t1) / (epochs * steps), loss


def gather_replays(ops, eng, B, reps, step=False):
    """csr_gather of B perm rows (step: what a training step gathers -- the byte tile and its table with counts_compact),
    replayed from a graph: ms per gather."""
    gather = eng._gather_step if step else eng._gather
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    eng.cursor.zero_()
    gather(B)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(10):
                gather(B)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (reps * 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=68579)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--big-cells', type=int, default=1500000)
    ap.add_argument('--big-genes', type=int, default=30000)
    ap.add_argument('--big-per-row', type=int, default=2000)
    ap.add_argument('--big-steps', type=int, default=20)
    ap.add_argument('--gather-only', action='store_true')
    ap.add_argument('--skip-big', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--forms', type=str, default='dense,dense_no_byte_store,counts,counts_compact')
    ap.add_argument('--compact', action='store_true', help='--gather-only: the byte tile\'s gather')
    ap.add_argument('--big-compact', action='store_true')
    ap.add_argument('--subset', type=int, default=0,
                    help='time csr_gather_cols for this many shuffled output genes beside csr_gather, interleaved; nothing else')
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda')
    ops = HipOps()
    n, G, B = args.cells, args.genes, args.batch
    n_train = int(n * 0.9)
    res = dict(cells=n, genes=G, batch=B, device=torch.cuda.get_device_name())

    Y = synth.generate_counts(n, G, device=dev)
    cc = prep.cell_counts(ops, Y, n, G)
    sf = cc / cc.median()
    X, norm = prep.transform(ops, Y, n, G, sf, True, True, return_norm=True)
    csr = dense_to_csr(Y, G)
    res['nnz'] = csr.nnz
    res['csr_gb'] = csr.nbytes / 1e9
    res['dense_estimate_gb'] = prep.dense_bytes(n, G) / 1e9

    if args.subset:
        import numpy as np
        K = args.subset
        cols = np.random.default_rng(0).permutation(G)[:K]
        engs = {}
        for form, k, oc in (('csr_gather', G, None), ('csr_gather_cols', K, cols)):
            eng = Engine('zinb-conddisp', G, k, (64, 32, 64), True, 0.0, ops=ops)
            eng.attach_counts(csr, sf, norm, compact=False, out_cols=oc)
            eng.reserve(B)
            eng.perm = torch.randperm(n_train, device=dev).to(torch.int32)
            engs[form] = eng
        rounds = {form: [] for form in engs}
        for _ in range(args.rounds):                  # interleaved: every round times both entries once
            for form, eng in engs.items():
                rounds[form].append(round(gather_replays(ops, eng, B, 50), 4))
        for form, ms in rounds.items():
            med = sorted(ms)[len(ms) // 2]
            eng = engs[form]
            res[form] = dict(ms=med, rounds=ms, spread=round((max(ms) - min(ms)) / med, 4),
                             tile_mb=(B * (eng.ldx + eng.ldy) * 4 + B * 4) / 1e6)
        res['subset'] = K
        res['cols_over_gather'] = round(res['csr_gather_cols']['ms'] / res['csr_gather']['ms'], 3)
        res['gather_status'] = [int(e.gather_status.item()) for e in engs.values()]
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(res, f, indent=1)
        return

    if args.gather_only:
        eng = Engine('zinb-conddisp', G, G, (64, 32, 64), True, 0.0, ops=ops)
        eng.attach_counts(csr, sf, norm, compact=args.compact)
        eng.reserve(B)
        eng.perm = torch.randperm(n_train, device=dev).to(torch.int32)
        print('gather %.4f ms' % gather_replays(ops, eng, B, 50, step=args.compact))
        return

    engs, runners = {}, {}
    for form in args.forms.split(','):
        eng = Engine('zinb-conddisp', G, G, (64, 32, 64), True, 0.0, ops=ops)
        eng.init_params(0)
        if form == 'dense':
            eng.attach_device_data(X, Y, sf, norm=norm)
        elif form == 'dense_no_byte_store':
            eng.attach_device_data(X, Y, sf, norm=norm, compact=False)
        else:
            eng.attach_counts(csr, sf, norm, compact=(form == 'counts_compact'))
        engs[form] = eng
        runners[form] = prepare_steps(eng, n_train, B)
    rounds = {form: [] for form in engs}
    loss = {}
    for _ in range(args.rounds):                      # interleaved: every round times every form once
        for form, eng in engs.items():
            ms, loss[form] = timed_steps(eng, runners[form][0], B, runners[form][1], args.epochs)
            rounds[form].append(round(ms, 4))
    forms = {}
    for form, ms in rounds.items():
        med = sorted(ms)[len(ms) // 2]
        forms[form] = dict(ms_per_step=med, rounds=ms, spread=round((max(ms) - min(ms)) / med, 4), mean_loss=loss[form])
        print(form, forms[form], flush=True)
    if 'counts' in engs:
        eng = engs['counts']
        gms = gather_replays(ops, eng, B, 50)
        tile_bytes = B * (eng.ldx + eng.ldy) * 4 + B * 4
        res['csr_gather'] = dict(ms=round(gms, 4), tile_mb=tile_bytes / 1e6,
                                 store_bound_ms=round(tile_bytes / (STORE_TBPS * 1e12) * 1e3, 4),
                                 fraction_of_store_bound=round(tile_bytes / (STORE_TBPS * 1e12) * 1e3 / gms, 3))
    if 'counts_compact' in engs:
        eng = engs['counts_compact']
        gms = gather_replays(ops, eng, B, 50, step=True)
        tile_bytes = B * (eng.cc.ldc + 8) + (B * 1024 if eng.cc_in is not None else 0)
        res['csr_gather_compact'] = dict(ms=round(gms, 4), tile_mb=tile_bytes / 1e6,
                                         store_bound_ms=round(tile_bytes / (STORE_TBPS * 1e12) * 1e3, 4),
                                         fraction_of_store_bound=round(tile_bytes / (STORE_TBPS * 1e12) * 1e3 / gms, 3))
    del engs, runners, eng
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    res['c3'] = forms
    for form in ('counts', 'counts_compact'):
        if form in forms and 'dense' in forms:
            res[form + '_over_dense'] = round(forms[form]['ms_per_step'] / forms['dense']['ms_per_step'], 3)
    del X, Y, csr
    torch.cuda.empty_cache()

    if not args.skip_big:
        bn, bG, per = args.big_cells, args.big_genes, args.big_per_row
        torch.cuda.reset_peak_memory_stats()
        t = time.perf_counter()
        big = synth_csr(bn, bG, per, dev)
        bsf, bnorm = csr_normalisation(ops, big)
        torch.cuda.synchronize()
        setup = time.perf_counter() - t
        eng = Engine('zinb-conddisp', bG, bG, (64, 32, 64), True, 0.0, ops=ops)
        eng.init_params(0)
        eng.attach_counts(big, bsf, bnorm, compact=args.big_compact)
        steps = args.big_steps
        ms, loss = time_steps(eng, min(int(bn * 0.9), steps * B), B, 1)
        _, total = torch.cuda.mem_get_info()
        res['beyond_dense'] = dict(counts_compact=bool(args.big_compact), cells=bn, genes=bG, nnz=big.nnz, csr_gb=round(big.nbytes / 1e9, 2),
                                   dense_estimate_gb=round(prep.dense_bytes(bn, bG) / 1e9, 1), steps=steps,
                                   ms_per_step=round(ms, 4), mean_loss=loss, setup_s=round(setup, 1),
                                   peak_gb=round(torch.cuda.max_memory_allocated() / 1e9, 2),
                                   device_gb=round(total / 1e9, 1))
        print('beyond dense', res['beyond_dense'], flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
