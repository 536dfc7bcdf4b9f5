"""The fp64 reference of the neighbour search (dcahip_knn / HipOps.knn / Engine.latent_knn / Autoencoder.neighbors): the
direct form sum_k (a_k - b_k)^2 in double, the k smallest under (d2, index), padded with -1 / inf.  KnnRefOps is the CPU
oracle with the one entry it lacks, so that the Python layers above the kernel run in the CPU suite.  The float criterion
(assert_knn_close) is what a correct fp32 evaluation of the direct form meets and the fp32 Gram form does not."""
import numpy as np
import torch

from oracle.cpu_ops import CpuRefOps


def d2_ref(Q, X):
    """[nq, n] squared distances, fp64, direct form."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    out = np.empty((Q.shape[0], X.shape[0]))
    rows = max(1, (1 << 22) // max(1, X.shape[0] * X.shape[1]))     # [rows, n, d] differences at a time: 32 MiB
    for s in range(0, Q.shape[0], rows):
        out[s:s + rows] = np.square(Q[s:s + rows, None, :] - X[None, :, :]).sum(axis=2)
    return out


def knn_ref(Q, X, k, self_offset=-1, return_full=False):
    """(idx [nq, k] int32, d2 [nq, k] float64): per query the k smallest candidates under (d2, index) ascending, query q's
    own row self_offset + q left out by index (self_offset = -1: nothing), -1 / inf where fewer than k are left."""
    D = d2_ref(Q, X)
    nq, n = D.shape
    full = D.copy()
    if self_offset >= 0:
        q = np.arange(nq)
        own = q + self_offset
        ok = own < n
        D[q[ok], own[ok]] = np.inf                            # taken out below by index, not by value
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.inf)
    for q in range(nq):
        cand = np.arange(n)
        if self_offset >= 0 and self_offset + q < n:
            cand = np.delete(cand, self_offset + q)
        order = cand[np.lexsort((cand, D[q, cand]))][:k]
        idx[q, :len(order)] = order
        d2[q, :len(order)] = D[q, order]
    return (idx, d2, full) if return_full else (idx, d2)


def float_tol(d):
    """Twice the first-order bound of the fp32 direct form, (d + 3) 2^-24 (d - 1 additions, the rounding of each
    difference counted twice through the square, the square itself; inputs exact in fp64)."""
    return 2.0 * (d + 3) * 2.0 ** -24


def assert_knn_close(idx, d2, Q, X, k, self_offset=-1, what='', ref=None):
    """The float-data criterion, for EVERY query: with ref_kth the reference's k-th smallest squared distance of the query
    and tol = float_tol(d),
      - every returned j has ref_d2(i, j) <= ref_kth (1 + tol);
      - every candidate with ref_d2 < ref_kth (1 - tol) is returned;
      - every returned d2 is within tol relative of ref_d2(i, returned j);
      - the returned keys ascend in (d2, index);
    the query's own row is not returned, and the -1 / inf padding is where the reference has it.  ref: what
    knn_ref(Q, X, k, self_offset, return_full=True) returned, when the caller has it already."""
    idx, d2 = np.asarray(idx), np.asarray(d2, np.float64)
    Q, X = np.asarray(Q), np.asarray(X)
    nq, n, d = Q.shape[0], X.shape[0], Q.shape[1]
    assert idx.shape == (nq, k) and d2.shape == (nq, k), (what, idx.shape, d2.shape)
    tol = float_tol(d)
    ridx, rd2, D = ref if ref is not None else knn_ref(Q, X, k, self_offset, return_full=True)
    worst = 0.0
    for q in range(nq):
        m = int((ridx[q] >= 0).sum())
        assert (idx[q, m:] == -1).all() and np.isinf(d2[q, m:]).all(), (what, q, 'padding')
        got = idx[q, :m]
        assert (got >= 0).all() and (got < n).all() and len(set(got.tolist())) == m, (what, q, 'indices')
        own = self_offset + q if self_offset >= 0 else -1
        assert own not in got, (what, q, 'self')
        if m == 0:
            continue
        kth = rd2[q, m - 1]
        ref_of_got = D[q, got]
        assert (ref_of_got <= kth * (1 + tol)).all(), (what, q, 'a returned candidate is too far', ref_of_got.max(), kth)
        must = np.flatnonzero(D[q] < kth * (1 - tol))
        must = must[must != own]
        assert np.isin(must, got).all(), (what, q, 'a candidate that is clearly nearer is missing')
        err = np.abs(d2[q, :m] - ref_of_got)
        assert (err <= tol * ref_of_got).all(), (what, q, 'distance', float((err / np.maximum(ref_of_got, 1e-300)).max()))
        nz = ref_of_got > 0
        if nz.any():
            worst = max(worst, float((err[nz] / ref_of_got[nz]).max()))
        keys = list(zip(d2[q, :m].tolist(), got.tolist()))
        assert keys == sorted(keys), (what, q, 'order')
    print('%s worst relative error of d2 %.2e (tol %.2e)' % (what, worst, tol))
    return worst


def clustered(n=1500, d=32, seed=0):
    """The hard regime of a ReLU latent: 12 clusters at N(50, 1), spread 0.1, fp32; row 7 a copy of row 3."""
    rs = np.random.RandomState(seed)
    centres = rs.normal(50.0, 1.0, (12, d))
    X = (centres[rs.randint(0, 12, n)] + rs.normal(0.0, 0.1, (n, d))).astype(np.float32)
    X[7] = X[3]
    return X


def direct_fp32(Q, X):
    """[nq, n] squared distances by the direct form evaluated sequentially in fp32."""
    Q, X = np.asarray(Q, np.float32), np.asarray(X, np.float32)
    acc = np.zeros((Q.shape[0], X.shape[0]), np.float32)
    for j in range(Q.shape[1]):
        df = Q[:, j][:, None] - X[:, j][None, :]
        acc = acc + df * df
    return acc


def gram_fp32(Q, X):
    """[nq, n] squared distances by |a|^2 + |b|^2 - 2 a.b evaluated in fp32 (the usual GEMM recipe)."""
    Q, X = np.asarray(Q, np.float32), np.asarray(X, np.float32)
    nq = np.zeros(Q.shape[0], np.float32)
    nx = np.zeros(X.shape[0], np.float32)
    dot = np.zeros((Q.shape[0], X.shape[0]), np.float32)
    for j in range(Q.shape[1]):
        nq = nq + Q[:, j] * Q[:, j]
        nx = nx + X[:, j] * X[:, j]
        dot = dot + Q[:, j][:, None] * X[:, j][None, :]
    return (nq[:, None] + nx[None, :]) - np.float32(2) * dot


def knn_from_matrix(D, k, self_offset=-1):
    """Top-k under (value, index) of a given distance matrix (any dtype), the query's own row left out by index."""
    nq, n = D.shape
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.inf, D.dtype)
    for q in range(nq):
        cand = np.arange(n)
        if self_offset >= 0 and self_offset + q < n:
            cand = np.delete(cand, self_offset + q)
        order = cand[np.lexsort((cand, D[q, cand]))][:k]
        idx[q, :len(order)] = order
        d2[q, :len(order)] = D[q, order]
    return idx, d2


class KnnRefOps(CpuRefOps):
    """CpuRefOps + knn (dca_amd.ops.HipOps.knn) from the fp64 reference."""
    name = 'cpu-oracle-knn'

    def knn_splits(self, nq, n, d, k):
        return 1

    def knn(self, Q, X, k, self_offset=-1, splits=0, out=None):
        from dca_amd.neighbors import check_knn_args
        (nq, d), n = Q.shape, X.shape[0]
        check_knn_args(nq, n, d, int(k), int(splits), int(self_offset))
        Qn, Xn = Q.numpy(), X.numpy()
        bad = int((~np.isfinite(Qn)).sum() + (~np.isfinite(Xn)).sum())
        if bad:
            raise ValueError('dca_amd: knn: %d coordinates are not finite (NaN or inf)' % bad)
        idx, d2 = knn_ref(Qn, Xn, int(k), int(self_offset))
        idx, d2 = torch.from_numpy(idx), torch.from_numpy(d2.astype(np.float32))
        if out is not None:
            out[0].copy_(idx)
            out[1].copy_(d2)
            return out
        return idx, d2
