"""Cost of the molecular cross-validation split (K-SPLIT, dcahip_csr_thin) on BASELINE configs[2]'s shape -- 68 579 x 20 000,
device-synthesised counts as bench.py makes them, held as CSR.  Three figures:

  (a) the device split of the RESIDENT CSR (HipOps.csr_thin: draw + count, two prefix sums, the stores, the parts cut to size);
  (b) the same from a host scipy CSR: prep.upload_csr + (a) -- what mcv.split_counts does before it copies the parts back;
  (c) what a user does today on the host: np.random.default_rng().binomial(values, f) on the CSR values, the two parts as
      scipy matrices, eliminate_zeros() on both.

(a): device events on the stream around the call; (b), (c): wall clock (host work is part of them), the device idle before and
after.  One warm-up, then the median of the rounds.
  python tools/bench_split.py [--cells 68579] [--genes 20000] [--fraction 0.8] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dca_amd import mcv, prep, synth                            # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402


def _host_csr(Y, n, G, chunk=4096):
    """The device count matrix as a host scipy CSR (float32), row chunks at a time."""
    ptr, idx, val = [np.zeros(1, np.int64)], [], []
    base = 0
    for s in range(0, n, chunk):
        t = Y[s:s + chunk, :G]
        m = t != 0
        per = m.sum(dim=1).cpu().numpy().astype(np.int64)
        idx.append(m.nonzero()[:, 1].to(torch.int32).cpu().numpy())
        val.append(t[m].cpu().numpy())
        ptr.append(base + np.cumsum(per))
        base += int(per.sum())
    return sp.csr_matrix((np.concatenate(val), np.concatenate(idx), np.concatenate(ptr)), shape=(n, G))


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=68579)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--fraction', type=float, default=0.8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda')
    n, G, f = args.cells, args.genes, args.fraction
    thr = mcv.threshold_of(f)
    ops = HipOps()
    Y = synth.generate_counts(n, G, device=dev)
    X = _host_csr(Y, n, G)
    del Y
    torch.cuda.empty_cache()
    csr = prep.upload_csr(X, dev, ops)
    res = {'workload': 'BASELINE configs[2] shape: %d x %d synthetic counts as CSR, fraction %g' % (n, G, f),
           'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'nnz': int(csr.nnz),
           'molecules': int(X.data.sum(dtype=np.float64))}

    def thin():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        parts = ops.csr_thin(csr, None, thr, 0)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), parts

    def upload_thin():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = ops.csr_thin(prep.upload_csr(X, dev, ops), None, thr, 0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, parts

    _, (A, B) = thin()                                          # warm-up
    total = float(A.values.sum(dtype=torch.float64).item()) + float(B.values.sum(dtype=torch.float64).item())
    assert total == res['molecules'], (total, res['molecules'])
    res['fit_nnz'], res['held_nnz'] = int(A.nnz), int(B.nnz)
    res['fit_molecule_fraction'] = float(A.values.sum(dtype=torch.float64).item()) / total
    del A, B
    ts = [thin()[0] for _ in range(args.rounds)]
    res['device_split_ms'] = round(_median(ts), 3)
    upload_thin()
    tu = [upload_thin()[0] for _ in range(args.rounds)]
    res['upload_and_device_split_ms'] = round(_median(tu), 3)
    res['rounds_ms'] = {'device_split': [round(t, 3) for t in ts], 'upload_and_device_split': [round(t, 3) for t in tu]}

    def host():
        t0 = time.perf_counter()
        a = np.random.default_rng().binomial(X.data.astype(np.int64), f).astype(np.float32)
        fit = sp.csr_matrix((a, X.indices.copy(), X.indptr.copy()), shape=X.shape)
        held = sp.csr_matrix((X.data - a, X.indices.copy(), X.indptr.copy()), shape=X.shape)
        fit.eliminate_zeros()
        held.eliminate_zeros()
        return (time.perf_counter() - t0) * 1e3
    host()
    th = [host() for _ in range(max(1, min(args.rounds, 3)))]
    res['host_binomial_ms'] = round(_median(th), 3)
    res['rounds_ms']['host_binomial'] = [round(t, 3) for t in th]
    res['host_note'] = 'numpy default_rng().binomial on the CSR values + eliminate_zeros() on both parts, one host thread; ' \
                       'not reproducible per cell and gene, and a resident matrix would cross PCIe twice on top of it'
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
