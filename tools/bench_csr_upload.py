"""Upload of a sparse count matrix at BASELINE configs[2] size (68 579 x 20 000, the synthetic ~7 % non-zero density of
dca_amd/synth.py), one JSON line:

  sparse_densify_s   the sparse path before CSR upload: toarray() of 8 192-row chunks + pageable copies
  csr_upload_s       prep.upload_sparse (CSR arrays over PCIe, dcahip_csr_expand on the device)
  dense_staged_s     prep._upload of the same matrix passed dense (page-locked, double-buffered)
  dca_dense_s / dca_csr_s   api.dca() end to end, 3 epochs at batch 32, on the dense and on the CSR AnnData

    python tools/bench_csr_upload.py [--out FILE] [--no-dca]
    python tools/bench_csr_upload.py --csr-only       # upload_sparse alone (for rocprofv3 --kernel-trace --stats)
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
    a = ap.parse_args()
    ops = HipOps()
    dev = torch.device('cuda', torch.cuda.current_device())
    t0 = time.perf_counter()
    X = synthetic_csr(a.n, a.G)
    t_gen = time.perf_counter() - t0
    ld = prep._r4(a.G)
    res = dict(n=a.n, G=a.G, nnz=int(X.nnz), density=X.nnz / (a.n * a.G), host_csr_build_s=round(t_gen, 2),
               csr_bytes=int(X.data.nbytes + X.indices.nbytes + X.indptr.nbytes), dense_bytes=a.n * ld * 4)
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
