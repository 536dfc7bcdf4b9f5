"""Upload of a sparse count matrix at BASELINE configs[2] size (68 579 x 20 000, the synthetic ~7 % non-zero density of
dca_amd/synth.py), one JSON line:

  sparse_densify_s   the sparse path before CSR upload: toarray() of 8 192-row chunks + pageable copies
  csr_upload_s       prep.upload_sparse (CSR arrays over PCIe, dcahip_csr_expand on the device)
  dense_staged_s     prep._upload of the same matrix passed dense (page-locked, double-buffered)
  dca_dense_s / dca_csr_s   api.dca() end to end, 3 epochs at batch 32, on the dense and on the CSR AnnData

    python tools/bench_csr_upload.py [--out FILE] [--no-dca]
    python tools/bench_csr_upload.py --csr-only       # upload_sparse alone (for rocprofv3 --kernel-trace --stats)

Counts-resident mode (the resident CSR is built and filtered on the device), one JSON line per process; ROUTE = device, or
host: the same code with csr_compress / csr_subset hidden from the ops object, which is the code path before those entries
existed (scipy compresses a dense matrix on the host, every filter uploads the host subset again):

    python tools/bench_csr_upload.py --dense-csr ROUTE   # dense float32 host matrix -> resident CSR (prep.upload_csr),
                                                         # beside the dense staged upload of the same matrix
    python tools/bench_csr_upload.py --prep ROUTE        # prep.normalize_device in counts mode, sparse host input with
                                                         # empty genes and cells (filters on, nothing copied back)
    python tools/bench_csr_upload.py --build-kernels     # one compress upload + one subset (for rocprofv3)
"""
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

from dca_amd import prep                         # noqa: E402
from dca_amd.ops import HipOps                   # noqa: E402


def synthetic_csr(n, G, density=0.07, seed=0, block=4096):
    """Seeded CSR counts built on the host: each element non-zero with probability `density`, values 1 .. 7 (float32)."""
    rng = np.random.default_rng(seed)
    indptr = [np.zeros(1, np.int64)]
    indices = []
    for s in range(0, n, block):
        e = min(n, s + block)
        r, c = np.nonzero(rng.random((e - s, G), dtype=np.float32) < density)
        indices.append(c.astype(np.int32))
        indptr.append(np.cumsum(np.bincount(r, minlength=e - s)) + indptr[-1][-1])
    indices = np.concatenate(indices)
    data = rng.integers(1, 8, len(indices)).astype(np.float32)
    return sp.csr_matrix((data, indices, np.concatenate(indptr)), shape=(n, G))


def densify_upload(X, dev, chunk_rows=8192):
    """The sparse branch of prep._upload as it was before the CSR upload existed."""
    n, G = X.shape
    out = torch.zeros(n, prep._r4(G), dtype=torch.float32, device=dev)
    for s in range(0, n, chunk_rows):
        e = min(n, s + chunk_rows)
        out[s:e, :G] = prep.host_chunk_tensor(X[s:e].toarray()).to(dev)
    return out


class WithoutBuildEntries:
    """An ops object without csr_compress / csr_subset: prep takes its host routes."""

    def __init__(self, ops):
        self._ops = ops

    def __getattr__(self, k):
        if k in ('csr_compress', 'csr_subset'):
            raise AttributeError(k)
        return getattr(self._ops, k)


def densify(X):
    Xd = np.empty(X.shape, np.float32)
    for s in range(0, X.shape[0], 8192):
        Xd[s:s + 8192] = X[s:s + 8192].toarray()
    return Xd


def with_empty_genes_and_cells(X, genes=(3, 1700, 19999), cells=(5, 4400, 68000)):
    """X (CSR) with the entries of some columns and rows removed (columns / rows beyond the shape are skipped)."""
    X = X.copy()
    for c in genes:
        X.data[X.indices == c] = 0
    for r in cells:
        if r < X.shape[0]:
            X.data[X.indptr[r]:X.indptr[r + 1]] = 0
    X.eliminate_zeros()
    return X


def same_csr(a, b):
    return bool(torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
                and torch.equal(a.values.view(torch.int32), b.values.view(torch.int32)))


def bench_dense_csr(a, ops, dev, X, res):
    route_ops = ops if a.dense_csr == 'device' else WithoutBuildEntries(ops)
    Xd = densify(X)
    res['route'] = a.dense_csr
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    csr, ts = timed(lambda: prep.upload_csr(Xd, dev, route_ops), 3 if a.dense_csr == 'device' else 2)
    res['dense_to_csr_s'] = ts
    res['final_csr_bytes'] = int(csr.nbytes)
    res['peak_device_bytes'] = int(torch.cuda.max_memory_allocated() - before)
    res['equals_sparse_upload_bitwise'] = same_csr(csr, prep.upload_csr(X, dev, ops))
    del csr
    dense, ts = timed(lambda: prep._upload(Xd, dev), 3)
    res['dense_staged_s'] = ts
    res['ratio_to_dense_staged'] = round(min(res['dense_to_csr_s']) / min(ts), 2)


def bench_prep(a, ops, dev, X, res):
    import pandas as pd
    from dca_amd._anndata import AnnData
    os.environ['DCA_AMD_RESIDENT'] = 'counts'
    route_ops = ops if a.prep == 'device' else WithoutBuildEntries(ops)
    X = with_empty_genes_and_cells(X)
    res['route'] = a.prep
    res['prep_counts_s'], res['shape_after'] = [], None
    for _ in range(3):
        ad = AnnData(X.copy(), obs=pd.DataFrame(index=pd.RangeIndex(X.shape[0]).astype(str)),
                     var=pd.DataFrame(index=pd.RangeIndex(X.shape[1]).astype(str)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ad, dd = prep.normalize_device(ad, ops=route_ops, to_host=False)
        torch.cuda.synchronize()
        res['prep_counts_s'].append(time.perf_counter() - t0)
        res['shape_after'] = [dd.n, dd.G]
        res['csr_checksum'] = [int(dd.csr.indptr[-1].item()), int(dd.csr.indices.sum(dtype=torch.int64).item()),
                               float(dd.csr.values.sum(dtype=torch.float64).item())]
        del ad, dd


def timed(fn, reps):
    ts = []
    out = None
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=68579)
    ap.add_argument('--G', type=int, default=20000)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-dca', action='store_true')
    ap.add_argument('--csr-only', action='store_true')
    ap.add_argument('--dense-csr', choices=['device', 'host'], default=None)
    ap.add_argument('--prep', choices=['device', 'host'], default=None)
    ap.add_argument('--build-kernels', action='store_true')
    a = ap.parse_args()
    ops = HipOps()
    dev = torch.device('cuda', torch.cuda.current_device())
    t0 = time.perf_counter()
    X = synthetic_csr(a.n, a.G)
    t_gen = time.perf_counter() - t0
    ld = prep._r4(a.G)
    res = dict(n=a.n, G=a.G, nnz=int(X.nnz), density=X.nnz / (a.n * a.G), host_csr_build_s=round(t_gen, 2),
               csr_bytes=int(X.data.nbytes + X.indices.nbytes + X.indptr.nbytes), dense_bytes=a.n * ld * 4)
    if a.dense_csr or a.prep or a.build_kernels:
        if a.dense_csr:
            bench_dense_csr(a, ops, dev, X, res)
        elif a.prep:
            bench_prep(a, ops, dev, X, res)
        else:
            csr = prep.upload_csr(densify(X), dev, ops)
            rows, cols = np.ones(a.n, bool), np.ones(a.G, bool)
            rows[[5, a.n - 1]] = False
            cols[[3, a.G - 1]] = False
            res['subset_nnz'] = prep.subset_csr(ops, csr, rows=rows, cols=cols).nnz
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')
        return
    up = lambda: prep.upload_sparse(X, dev, ops, ld)                     # noqa: E731
    if a.csr_only:
        _, ts = timed(up, 4)
        res['csr_upload_s'] = ts
        print(json.dumps(res))
        return
    csr, ts = timed(up, 5)
    res['csr_upload_s'] = ts
    Xd = np.empty((a.n, a.G), np.float32)
    for s in range(0, a.n, 8192):
        Xd[s:s + 8192] = X[s:s + 8192].toarray()
    dense, ts = timed(lambda: prep._upload(Xd, dev), 5)
    res['dense_staged_s'] = ts
    res['csr_equals_dense_bitwise'] = bool(torch.equal(csr.view(torch.int32), dense.view(torch.int32)))
    del csr
    old, ts = timed(lambda: densify_upload(X, dev), 2)
    res['sparse_densify_s'] = ts
    res['old_equals_dense_bitwise'] = bool(torch.equal(old.view(torch.int32), dense.view(torch.int32)))
    del old, dense
    torch.cuda.empty_cache()
    best = lambda k: min(res[k])                                         # noqa: E731
    res['speedup_vs_densify'] = round(best('sparse_densify_s') / best('csr_upload_s'), 2)
    res['speedup_vs_dense_staged'] = round(best('dense_staged_s') / best('csr_upload_s'), 2)
    res['csr_upload_GBps_of_csr_bytes'] = round(res['csr_bytes'] / best('csr_upload_s') / 1e9, 2)
    if not a.no_dca:
        import pandas as pd
        from dca_amd.api import dca
        from dca_amd._anndata import AnnData

        def run(M):
            ad = AnnData(M, obs=pd.DataFrame(index=pd.RangeIndex(a.n).astype(str)),
                         var=pd.DataFrame(index=pd.RangeIndex(a.G).astype(str)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dca(ad, ae_type='zinb-conddisp', epochs=3, batch_size=32, random_state=0, return_info=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, ad
        res['dca_dense_s'], res['dca_csr_s'] = [], []
        outs = {}
        for rnd in range(2):                    # round 0 warms code objects and graphs for both
            for key, M in (('dense', Xd), ('csr', X)):
                t, ad = run(M)
                res['dca_%s_s' % key].append(round(t, 3))
                outs[key] = ad
        res['dca_X_bitwise_equal'] = bool(np.array_equal(np.asarray(outs['dense'].X).view(np.uint32),
                                                         np.asarray(outs['csr'].X).view(np.uint32)))
        res['dca_loss_history_equal'] = outs['dense'].uns['dca_loss_history'] == outs['csr'].uns['dca_loss_history']
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
