"""The host references of K-MEANS (dcahip_kmeans_seed / dcahip_kmeans_step / dca_amd.cluster / Engine.latent_kmeans /
Autoencoder.cluster): the seeding in exact integers, one Lloyd iteration in fp64 (direct-form distances, argmin under
(d2, index), double sums, one rounding of sum / count, the re-seeding rule), the whole loop with the renumbering, and
KmeansRefOps, the CPU oracle with the entries it lacks so that the Python layers above the kernels run in the CPU suite."""
import math

import numpy as np
import torch

from dca_amd.mcv import philox4x32_10

from _knn_ref import KnnRefOps, clustered, d2_ref  # noqa: F401  (clustered: the float dataset of the tests)

SEED_TAG = 0x6B6D2B2B            # kPhiloxSeedTag (dca_amd/csrc/philox.hpp)
_M64 = (1 << 64) - 1


def _r64(seed, t, init):
    o = philox4x32_10(t, init, 0, SEED_TAG, seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    return (int(o[1]) << 32) | int(o[0])


def seed_ref(X, k, seed=0, init=0):
    """rows [k] (Python ints): the k-means++ draw of include/dcahip.h in exact integers.  m_i is the fp32 rounding of the
    fp64 direct-form distance (the kernel's bits wherever the fp32 arithmetic is exact, as on the integer datasets)."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    rows = [(_r64(seed, 0, init) * n) >> 64]
    m = np.full(n, np.inf, np.float32)
    for t in range(1, k):
        m = np.minimum(m, d2_ref(X, X[rows[-1]][None])[:, 0].astype(np.float32))
        M = float(m.max())
        r = _r64(seed, t, init)
        if M == 0.0:
            rows.append((r * n) >> 64)
            continue
        e = 31 - math.frexp(M)[1]                              # M 2^e in [2^30, 2^31)
        q = [int(math.ldexp(float(v), e)) for v in m]          # exact: a power-of-two scale and a truncation
        assert 1 << 30 <= max(q) < 1 << 31
        T = (r * sum(q)) >> 64
        pre = np.cumsum(np.asarray(q, dtype=object))
        rows.append(int(next(i for i in range(n) if pre[i] > T)))
    return rows


def step_ref(X, C, prev=None):
    """One Lloyd iteration in fp64: dict of labels int32 [n], d2 float64 [n], counts int64 [k], sums float64 [k, d], inertia,
    changed (against prev, -1 everywhere when None), reseeded, C_out float32 [k, d], gap (the smallest relative distance gap
    (second - best) / second over the points; 0 where the second is 0; inf for k = 1)."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    n, k = X.shape[0], C.shape[0]
    D = d2_ref(X, C)
    labels = np.argmin(D, axis=1).astype(np.int32)             # the first of equal minima: the order (d2, c)
    d2 = D[np.arange(n), labels]
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros((k, X.shape[1]))
    np.add.at(sums, labels, X.astype(np.float64))
    C_out = C.copy()
    for c in np.flatnonzero(counts):
        C_out[c] = (sums[c] / counts[c]).astype(np.float32)
    reseeded = 0
    empty = np.flatnonzero(counts == 0)
    if len(empty) and d2.max() > 0:
        far = int(np.flatnonzero(d2 == d2.max()).max())        # the largest key (d2, index)
        C_out[empty[0]] = X[far]
        reseeded = 1
    prev = np.full(n, -1, np.int32) if prev is None else np.asarray(prev)
    gap = np.inf
    if k > 1:
        two = np.partition(D, 1, axis=1)[:, :2]
        gap = float(np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1), 0).min())
    return dict(labels=labels, d2=d2, counts=counts, sums=sums, inertia=float(d2.sum()), changed=int((labels != prev).sum()),
                reseeded=reseeded, C_out=C_out, gap=gap)


def lloyd_ref(X, C0, max_iter=300):
    """The loop of dca_amd.cluster.lloyd on step_ref: dict of labels, centers, inertia, n_iter, converged, counts, gap (the
    smallest gap of any point in any iteration) and reseeds (the iterations that re-seeded)."""
    C = np.asarray(C0, np.float32).copy()
    prev, conv, gap, reseeds = None, 0, np.inf, []
    for it in range(1, max_iter + 1):
        s = step_ref(X, C, prev)
        gap = min(gap, s['gap'])
        if s['reseeded']:
            reseeds.append(it)
        prev, C = s['labels'], s['C_out']
        if s['changed'] == 0 and not s['reseeded']:
            conv = it
            break
    if not conv:
        s = step_ref(X, C, prev)
        gap = min(gap, s['gap'])
    return dict(labels=s['labels'], centers=C, inertia=s['inertia'], n_iter=conv or max_iter, converged=bool(conv),
                counts=s['counts'], gap=gap, reseeds=reseeds)


def kmeans_ref(X, k, n_init=10, max_iter=300, seed=0, init=None):
    """dca_amd.cluster.kmeans on the references: dict of labels, centers, inertia, n_iter, converged, sizes, gap, renumbered
    by size descending (ties by the number in the run)."""
    from dca_amd.cluster import renumber
    X = np.asarray(X, np.float32)
    best = None
    for j in range(1 if init is not None else n_init):
        C0 = np.asarray(init, np.float32) if init is not None else X[seed_ref(X, k, seed, j)]
        run = lloyd_ref(X, C0, max_iter)
        if best is None or run['inertia'] < best['inertia']:
            best = run
    rank, order = renumber(best['counts'])
    return dict(labels=rank[best['labels']].astype(np.int32), centers=best['centers'][order], inertia=best['inertia'],
                n_iter=best['n_iter'], converged=best['converged'], sizes=best['counts'][order], gap=best['gap'])


def int_data(n, d, k, seed=0):
    """(X [n, d], C [k, d]): X integers in [-4, 4] with duplicated rows, C multiples of 0.5 in [-4, 4] with two identical
    centres (k >= 2): every fp32 operation of the distance is exact and integer-valued doubles sum exactly in any order."""
    rs = np.random.RandomState(1000 * seed + 7 * n + 3 * d + k)
    X = rs.randint(-4, 5, (n, d)).astype(np.float32)
    if n > 1:
        X[n - 1] = X[0]
    if n > 5:
        X[5] = X[2]
    C = (rs.randint(-8, 9, (k, d)) * 0.5).astype(np.float32)
    if k > 1:
        C[k - 1] = C[k // 2 - 1] if k > 2 else C[0]
    return X, C


# (d, k, seed) on clustered(1500, d) whose k-means++ start (seed_ref, init 0) keeps the reference's own relative gap
# (second - best) / second >= 1e-3 for every point in every iteration and takes more than one iteration (6, 5, 10, 3, 7 and 2
# iterations at gaps of 1.3e-3, 9.5e-3, 1.5e-3, 5.7e-2, 1.05e-3 and 0.97); the condition is asserted in
# tests/test_kmeans_cpu.py.  Seeds whose gap fell below 1e-3 -- (3, 5, 1 .. 5), (3, 12, 3), (3, 12, 4), (32, 5, 0),
# (128, 40, 0) -- do not qualify.
TRAJECTORY_CASES = [(3, 5, 0), (3, 12, 0), (3, 12, 1), (3, 12, 2), (3, 12, 5), (32, 12, 0)]
TRAJECTORY_GAP = 1e-3


class KmeansRefOps(KnnRefOps):
    """KnnRefOps + kmeans_seed / kmeans_step (dca_amd.ops.HipOps) from the references."""
    name = 'cpu-oracle-kmeans'

    def kmeans_workspace_bytes(self, n, d, k):
        from dca_amd.cluster import check_kmeans_args
        check_kmeans_args(int(n), int(d), int(k))
        return 0

    def kmeans_raise(self, status):
        bad = int(status.item())
        if bad:
            raise ValueError('dca_amd: kmeans: %d coordinates are not finite (NaN or inf)' % bad)

    def kmeans_seed(self, X, k, seed=0, init=0, ws=None):
        from dca_amd.cluster import check_kmeans_args
        check_kmeans_args(X.shape[0], X.shape[1], int(k))
        Xn = X.numpy()
        bad = int((~np.isfinite(Xn)).sum())
        if bad:
            raise ValueError('dca_amd: kmeans: %d coordinates are not finite (NaN or inf)' % bad)
        rows = seed_ref(Xn, int(k), int(seed), int(init))
        return torch.as_tensor(np.asarray(rows, np.int32)), torch.from_numpy(Xn[rows].copy())

    def kmeans_bind(self, X, C_in, C_out, labels, d2, counts, sums, inertia, info, ws, status):
        return lambda it: self.kmeans_step(X, C_in, C_out, labels, d2, counts, sums, inertia, info, it, ws, status, check=False)

    def kmeans_step(self, X, C_in, C_out, labels, d2, counts, sums, inertia, info, it, ws, status, check=True):
        from dca_amd.cluster import check_kmeans_args
        check_kmeans_args(X.shape[0], X.shape[1], C_in.shape[0])
        Xn, Cn = X.numpy(), C_in.numpy()
        status += int((~np.isfinite(Xn)).sum() + (~np.isfinite(Cn)).sum())
        if not int(status.item()):
            s = step_ref(Xn, Cn, labels.numpy())
            labels.copy_(torch.from_numpy(s['labels']))
            d2.copy_(torch.from_numpy(s['d2'].astype(np.float32)))
            counts.copy_(torch.from_numpy(s['counts'].astype(np.int32)))
            sums.copy_(torch.from_numpy(s['sums']))
            inertia[0] = s['inertia']
            info[0], info[1] = s['changed'], s['reseeded']
            if int(info[2]) == 0 and s['changed'] == 0 and not s['reseeded']:
                info[2] = int(it)
            C_out.copy_(torch.from_numpy(s['C_out']))
        if check:
            self.kmeans_raise(status)
