"""The host reference of K-LOUVAIN (dcahip_graph_symmetrize / dcahip_louvain_sweep / HipOps.louvain_level /
dca_amd.community / Engine.latent_louvain / Autoencoder.louvain): the rule of include/dcahip.h restated in Python integers
and numpy integer arrays -- no floating point anywhere, the scores (up to 2^78) as Python ints -- and LouvainRefOps, the CPU
oracle with the entries it lacks so that the Python layers above the kernels run in the CPU suite.  The device must equal
this by ==."""
import numpy as np
import torch

from _groups_ref import GroupRefOps
from _silhouette_ref import SilhouetteRefOps

R = 1024


# ------------------------------------------------------------------------------------------------------------------ the graph
def symmetrize_ref(indices):
    """(rowptr int64 [n + 1], col int64 [2m] ascending in every row, deg int64 [n], bad) of W = A + A^T as unit entries: -1 is
    padding, an entry equal to its row is dropped, any other entry outside 0 .. n-1 is counted in ``bad`` and dropped."""
    idx = np.asarray(indices).astype(np.int64)
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1)
    real = (cols != -1) & (cols != rows)
    ok = real & (cols >= 0) & (cols < n)
    bad = int((real & ~ok).sum())
    r = np.concatenate([rows[ok], cols[ok]])
    c = np.concatenate([cols[ok], rows[ok]])
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    deg = np.bincount(r, minlength=n).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return rowptr, c, deg, bad


def canonical(rowptr, col, wt=None):
    """A CSR with every row sorted by (column, weight): what the order inside a row does not change."""
    rowptr, col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    w = np.ones(len(col), np.int64) if wt is None else np.asarray(wt).astype(np.int64)
    order = np.lexsort((w, col, rows))
    return rowptr, col[order], w[order]


def _rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def degrees_ref(rowptr, col, wt=None):
    w = np.ones(len(col), np.int64) if wt is None else np.asarray(wt).astype(np.int64)
    ki = np.zeros(len(rowptr) - 1, np.int64)
    np.add.at(ki, _rows(rowptr), w)
    return ki


def q_int_ref(rowptr, col, wt, labels, g):
    """(Q_int, inside, tot2, 2m) of a labelling, Python ints: Q_int = 2m R inside - g tot2."""
    rowptr, col, labels = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64), np.asarray(labels).astype(np.int64)
    w = np.ones(len(col), np.int64) if wt is None else np.asarray(wt).astype(np.int64)
    rows = _rows(rowptr)
    inside = int(w[labels[rows] == labels[col]].sum())
    twom = int(w.sum())
    tot = {}
    for lab, k in zip(labels.tolist(), degrees_ref(rowptr, col, wt).tolist()):
        tot[lab] = tot.get(lab, 0) + k
    tot2 = sum(t * t for t in tot.values())
    return twom * R * inside - g * tot2, inside, tot2, twom


def modularity_ref(indices, labels, resolution=1.0):
    """(Q_int, 2m) of any labelling of the graph of an index array; the modularity is Q_int / ((2m)^2 R)."""
    rowptr, col, _, _ = symmetrize_ref(indices)
    q, _, _, twom = q_int_ref(rowptr, col, None, labels, int(round(resolution * R)))
    return q, twom


# ------------------------------------------------------------------------------------------------------------------ one sweep
def sweep_ref(rowptr, col, wt, labels, g, parity, twom=None):
    """One synchronous sweep from ``labels`` (values in 0 .. n-1): returns (labels_new int64 [n], moved, inside, tot2) with
    the sums taken from the NEW labels, all Python ints.  Even parity admits only c < own, odd only c > own; the highest score
    strictly above staying wins, ties to the lowest c; the self-loop is left out of k_{i,c}."""
    rowptr, col, labels = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64), np.asarray(labels).astype(np.int64)
    n = len(labels)
    w = np.ones(len(col), np.int64) if wt is None else np.asarray(wt).astype(np.int64)
    rows = _rows(rowptr)
    ki = degrees_ref(rowptr, col, wt)
    tot = np.zeros(n, np.int64)
    np.add.at(tot, labels, ki)
    if twom is None:
        twom = int(w.sum())
    M = twom * R
    off = col != rows
    key = rows[off] * n + labels[col[off]]
    uk, inv = np.unique(key, return_inverse=True)
    kic = np.zeros(len(uk), np.int64)
    np.add.at(kic, inv, w[off])
    ur, uc = uk // n, uk % n
    own = labels[ur]
    kia = np.zeros(n, np.int64)
    kia[ur[uc == own]] = kic[uc == own]
    O = lambda a: np.asarray(a).astype(object)
    stay = O(kia) * M - g * O(ki) * (O(tot[labels]) - O(ki))
    adm = (uc < own) if parity % 2 == 0 else (uc > own)
    ur, uc, kic = ur[adm], uc[adm], kic[adm]
    new = labels.copy()
    if len(ur):
        score = O(kic) * M - g * O(ki[ur]) * O(tot[uc])
        starts = np.flatnonzero(np.concatenate([[True], ur[1:] != ur[:-1]]))
        counts = np.diff(np.concatenate([starts, [len(ur)]]))
        gmax = np.maximum.reduceat(score, starts)
        at_max = np.array(score == np.repeat(gmax, counts), dtype=bool)
        best_c = np.minimum.reduceat(np.where(at_max, uc, n), starts)
        v = ur[starts]
        move = np.array(gmax > stay[v], dtype=bool)
        new[v[move]] = best_c[move]
    moved = int((new != labels).sum())
    _, inside, tot2, _ = q_int_ref(rowptr, col, wt, new, g)
    return new, moved, inside, tot2


# ------------------------------------------------------------------------------------------------------------------ one level
class RefLevel:
    """The state machine of a level (the contract of dca_amd.ops.LouvainLevel, on host tensors)."""

    def __init__(self, rowptr, col, wt, twom, g, max_sweeps, labels=None, best_q=None):
        self.rowptr, self.col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)
        self.wt = None if wt is None else np.asarray(wt).astype(np.int64)
        self.n, self.twom, self.g, self.max_sweeps = len(self.rowptr) - 1, int(twom), int(g), int(max_sweeps)
        lab = np.arange(self.n, dtype=np.int64) if labels is None else np.asarray(labels).astype(np.int64)
        self.best = q_int_ref(self.rowptr, self.col, self.wt, lab, self.g)[0] if best_q is None else int(best_q)
        self.done, self.sweeps, self.idle, self.kept = 0, 0, 0, False
        self.last = dict(moved=0, inside=0, tot2=0)
        self.ki = torch.from_numpy(degrees_ref(self.rowptr, self.col, self.wt).astype(np.int32))
        self._set(lab)
        self.labels_new, self.tot_new = self.labels.clone(), torch.zeros_like(self.tot)

    def _totals(self, lab):
        tot = np.zeros(self.n, np.int64)
        np.add.at(tot, lab, self.ki.numpy().astype(np.int64))
        return torch.from_numpy(tot.astype(np.int32))

    def _set(self, lab):
        self._lab = lab
        self.labels, self.tot = torch.from_numpy(lab.astype(np.int32)), self._totals(lab)

    def sweep(self, s):
        self.kept = False
        if self.done:
            return
        new, moved, inside, tot2 = sweep_ref(self.rowptr, self.col, self.wt, self._lab, self.g, s, self.twom)
        self.labels_new, self.tot_new = torch.from_numpy(new.astype(np.int32)), self._totals(new)
        self.last = dict(moved=moved, inside=inside, tot2=tot2)
        q = self.twom * R * inside - self.g * tot2
        self.sweeps += 1
        if moved == 0:
            self.idle += 1
            if self.idle >= 2:
                self.done = 2
        elif q > self.best:
            self.kept, self.best, self.idle = True, q, 0
            self._set(new)
        else:
            self.done = 1
        if not self.done and self.sweeps >= self.max_sweeps:
            self.done = 3

    def read(self, s):
        return dict(done=self.done, sweeps=self.sweeps, q=self.best, idle=self.idle, kept=self.kept, **self.last)


def level_ref(rowptr, col, wt, twom, g, max_sweeps):
    """(labels int64 [n], Q_int, sweeps run) of one level from singletons."""
    lev = RefLevel(rowptr, col, wt, twom, g, max_sweeps)
    s = 0
    while not lev.done:
        lev.sweep(s)
        s += 1
    return lev._lab, lev.best, lev.sweeps


# --------------------------------------------------------------------------------------------------------------- aggregation
def relabel_ref(labels):
    """(cu int64 [n], nc): communities renumbered by their lowest member vertex."""
    first = {}
    for i, lab in enumerate(np.asarray(labels).tolist()):
        first.setdefault(lab, i)
    rank = {lab: r for r, lab in enumerate(sorted(first, key=first.get))}
    return np.array([rank[lab] for lab in np.asarray(labels).tolist()], dtype=np.int64), len(rank)


def aggregate_ref(rowptr, col, wt, cu, nc):
    """The coarse CSR (rowptr, col ascending in every row, wt), a dictionary of Python ints: the weight of (a, b) = the sum of
    the entries (i, j) with cu[i] = a, cu[j] = b."""
    rowptr, col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)
    w = np.ones(len(col), np.int64) if wt is None else np.asarray(wt).astype(np.int64)
    acc = {}
    for a, b, x in zip(np.asarray(cu)[_rows(rowptr)].tolist(), np.asarray(cu)[col].tolist(), w.tolist()):
        acc[(a, b)] = acc.get((a, b), 0) + x
    keys = sorted(acc)
    deg = np.bincount(np.array([a for a, _ in keys], dtype=np.int64), minlength=nc) if keys else np.zeros(nc, np.int64)
    return (np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), np.array([b for _, b in keys], dtype=np.int64),
            np.array([acc[k] for k in keys], dtype=np.int64))


# -------------------------------------------------------------------------------------------------------------- the whole run
def louvain_ref(indices, resolution=1.0, max_levels=32, max_sweeps=1000):
    """dict of labels int64 [n] (numbered by size descending, ties by lowest member), q_int, twom, g, level_sizes, n_sweeps,
    sizes: dca_amd.community.louvain restated."""
    g = int(round(resolution * R))
    rowptr, col, _, bad = symmetrize_ref(indices)
    assert bad == 0
    n = len(rowptr) - 1
    twom = len(col)
    wt = None
    members = np.arange(n, dtype=np.int64)
    level_sizes, n_sweeps, q = [], [], 0
    while twom > 0 and len(level_sizes) < max_levels:
        labels, q, sweeps = level_ref(rowptr, col, wt, twom, g, max_sweeps)
        n_sweeps.append(sweeps)
        cu, nc = relabel_ref(labels)
        if nc == len(rowptr) - 1:
            break
        members = cu[members]
        level_sizes.append(nc)
        rowptr, col, wt = aggregate_ref(rowptr, col, wt, cu, nc)
    nc = level_sizes[-1] if level_sizes else n
    sizes = np.bincount(members, minlength=nc).astype(np.int64)
    order = np.lexsort((np.arange(nc), -sizes))
    rank = np.empty(nc, np.int64)
    rank[order] = np.arange(nc)
    return dict(labels=rank[members], q_int=q, twom=twom, g=g, level_sizes=level_sizes, n_sweeps=n_sweeps, sizes=sizes[order])


# ----------------------------------------------------------------------------------------------------------------- fixtures
_cache = {}


def blobs(n, d, centers, sigma, seed):
    """n points in d dimensions around ``centers`` blob centres drawn from N(0, 10^2), blob spread sigma (float32)."""
    rs = np.random.RandomState(seed)
    C = rs.randn(centers, d) * 10.0
    which = rs.randint(0, centers, n)
    return (C[which] + rs.randn(n, d) * sigma).astype(np.float32), which


def knn_indices(X, k):
    """Exact k nearest other points under (d2, index), int32 [n, k] (fp64 direct form)."""
    X = np.asarray(X, np.float64)
    sq = (X * X).sum(1)
    out = np.empty((len(X), k), np.int32)
    for s in range(0, len(X), 512):
        D = sq[s:s + 512, None] + sq[None, :] - 2.0 * X[s:s + 512] @ X.T
        D[np.arange(len(D)), np.arange(s, s + len(D))] = np.inf
        out[s:s + 512] = np.argsort(D, axis=1, kind='stable')[:, :k]
    return out


# (points, k, blobs, sigma): the graphs of the quality condition; the first recovers its 6 blobs exactly
FIXTURES = {'blobs600': (600, 10, 6, 1.0), 'blobs3000': (3000, 15, 12, 1.5), 'one3000': (3000, 15, 1, 1.0)}


def fixture(name):
    """(indices int32 [n, k], planted blob of every point) of a named graph, computed once."""
    if ('fx', name) not in _cache:
        n, k, b, sigma = FIXTURES[name]
        X, which = blobs(n, 8, b, sigma, seed=n + b)
        _cache[('fx', name)] = (knn_indices(X, k), which)
    return _cache[('fx', name)]


def fixture_ref(name, resolution=1.0):
    """louvain_ref of a named graph, computed once and left unchanged."""
    if ('ref', name, resolution) not in _cache:
        _cache[('ref', name, resolution)] = louvain_ref(fixture(name)[0], resolution)
    return _cache[('ref', name, resolution)]


def cliques(sizes):
    """An index array whose graph is disjoint cliques of the given sizes joined in a ring by single edges (-1 padded), and
    the planted labels."""
    n, k = sum(sizes), max(sizes)
    idx = np.full((n, k), -1, np.int32)
    planted = np.empty(n, np.int64)
    start = 0
    for c, s in enumerate(sizes):
        for i in range(s):
            others = [start + j for j in range(s) if j != i]
            idx[start + i, :len(others)] = others
        planted[start:start + s] = c
        start += s
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for c in range(len(sizes)):                      # the last vertex of clique c points to the first of the next one
        nxt = starts[(c + 1) % len(sizes)]
        idx[starts[c + 1] - 1, sizes[c] - 1] = nxt
    return idx, planted


def wide_case(sign):
    """A 4-vertex weighted graph on which vertex 0's two scores (staying with vertex 1 in community 0, moving to community 2
    in an odd sweep) are of size 2^69 and differ by exactly ``sign`` (+1: it moves, -1: it stays): g = 65535, T = 2m chosen
    with 1024 T = 65535 k_0 + sign.  Returns (rowptr, col, wt, labels, g, twom)."""
    g = 65535
    inv = pow(1024, -1, g)
    T = (sign * inv) % g
    T += ((3 << 29) - T + g - 1) // g * g                  # the first such T from 1.5 * 2^30 up
    k0 = (1024 * T - sign) // g
    assert 1024 * T - g * k0 == sign and T < 1 << 31
    wa = 1000
    w1 = wa + 1
    s0 = k0 - wa - w1
    s1 = 1 << 28
    k1, k2 = wa + s1, w1 + s1
    s3 = T - k0 - k1 - k2
    assert s0 > 0 and s3 > 0
    rows = [[(0, s0), (1, wa), (2, w1)], [(0, wa), (1, s1)], [(0, w1), (2, s1)], [(3, s3)]]
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], dtype=np.int64)
    wt = np.array([w for r in rows for _, w in r], dtype=np.int64)
    return rowptr, col, wt, np.array([0, 0, 2, 3], dtype=np.int64), g, int(T)


# ------------------------------------------------------------------------------------------------------------------- the ops
class LouvainRefOps(SilhouetteRefOps, GroupRefOps):
    """The CPU oracle + graph_symmetrize and louvain_level (dca_amd.ops.HipOps) from the integer reference."""
    name = 'cpu-oracle-louvain'

    def graph_symmetrize_workspace_bytes(self, n, k):
        from dca_amd.community import check_graph_args
        check_graph_args(int(n), int(k))
        return 0

    def graph_symmetrize(self, idx):
        from dca_amd.community import check_graph_args
        if idx.dtype != torch.int32 or idx.dim() != 2:
            raise ValueError('dca_amd: louvain: the neighbour indices are a 2-d int32 tensor with unit column stride')
        n, k = idx.shape
        check_graph_args(n, k)
        rowptr, col, deg, bad = symmetrize_ref(idx.numpy())
        if bad:
            raise ValueError('dca_amd: louvain: %d neighbour indices lie outside 0 .. %d (and are not the padding -1)' % (bad, n - 1))
        return torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)), torch.from_numpy(deg.astype(np.int32))

    def louvain_level(self, rowptr, col, wt, twom, g, max_sweeps, labels=None, best_q=None):
        from dca_amd.community import check_level_args
        check_level_args(rowptr.numel() - 1, col.numel(), int(twom), int(g), int(max_sweeps))
        return RefLevel(rowptr.numpy(), col.numpy(), None if wt is None else wt.numpy(), twom, g, max_sweeps,
                        None if labels is None else labels.numpy(), best_q)
