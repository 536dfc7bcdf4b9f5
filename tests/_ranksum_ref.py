"""The reference of the Wilcoxon rank-sum integers (dcahip_ranksum / Engine.rank_sums, include/dcahip.h) in two forms:
rank_ref by scipy.stats.rankdata and brute-force counting, rank_scan as the sorted-scan restatement the kernel is built
on (run starts and ends by scans, the tie term of a reference comparison by the identity of the kernel's header).
RankSumRefOps is the CPU oracle with the one entry it lacks, so that the Python layers above the kernel run in the CPU
suite."""
import numpy as np
from scipy.stats import rankdata

from oracle.cpu_ops import CpuRefOps, _mat, _vec


def _tie_term(v):
    """sum of t^3 - t over the runs of equal values of v."""
    t = np.unique(np.asarray(v, np.float64), return_counts=True)[1].astype(np.int64)
    return int((t ** 3 - t).sum())


def rank_ref(x, order, gstart, K, ref=-1):
    """(rank2 [K, g], tie [K, g]) int64 of the gene-major matrix x [g, n]: per row the cells order lists (group c =
    positions gstart[c] .. gstart[c + 1]) compared as real numbers (float64 compares -0.0 equal to 0.0).
    ref < 0: rank2 = 2 x the sum of the group's mid-ranks among all listed cells (scipy.stats.rankdata), tie over all of them.
    ref >= 0: rank2 = 2 U of the group against group ref -- for c != ref from the mid-ranks of the two groups pooled
    (U = R - n_c (n_c + 1) / 2), for c == ref by counting pairs (2 for a smaller, 1 for an equal ref cell); tie over the
    two groups pooled (row ref: ref alone).  A NaN among a row's listed cells: -1 in the whole row."""
    x = np.asarray(x, np.float32)
    order, gstart = np.asarray(order, np.int64), np.asarray(gstart, np.int64)
    g = x.shape[0]
    rank2, tie = np.zeros((K, g), np.int64), np.zeros((K, g), np.int64)
    for j in range(g):
        v = x[j, order].astype(np.float64)
        if np.isnan(v).any():
            rank2[:, j], tie[:, j] = -1, -1
            continue
        parts = [v[gstart[c]:gstart[c + 1]] for c in range(K)]
        if ref < 0:
            r2 = np.rint(2.0 * rankdata(v, method='average')).astype(np.int64) if len(v) else np.zeros(0, np.int64)
            for c in range(K):
                rank2[c, j] = r2[gstart[c]:gstart[c + 1]].sum()
            tie[:, j] = _tie_term(v)
            continue
        vr = parts[ref]
        for c in range(K):
            vc = parts[c]
            if c == ref:
                rank2[c, j] = sum(2 * int((vr < a).sum()) + int((vr == a).sum()) for a in vc)
                tie[c, j] = _tie_term(vr)
            else:
                pooled = np.concatenate([vc, vr])
                r2 = np.rint(2.0 * rankdata(pooled, method='average')).astype(np.int64) if len(pooled) else np.zeros(0, np.int64)
                rank2[c, j] = r2[:len(vc)].sum() - len(vc) * (len(vc) + 1)
                tie[c, j] = _tie_term(pooled)
    return rank2, tie


def rank_scan(x, order, gstart, K, ref=-1):
    """The same numbers in the form the kernel computes them: a STABLE sort of the listed cells (ties keep group order),
    run starts a and ends b by scans over the sorted positions, P = the exclusive prefix count of ref cells; every cell adds
    a + b + 1 (rest) or P(a) + P(b) (ref); the tie term with ref is sum over runs of t_r^3 - t_r plus, per same-group
    sub-run of c != ref, (t_c + t_r)^3 - t_r^3 - t_c."""
    x = np.asarray(x, np.float32)
    order, gstart = np.asarray(order, np.int64), np.asarray(gstart, np.int64)
    g, m = x.shape[0], len(order)
    code0 = np.repeat(np.arange(K), np.diff(gstart))
    rank2, tie = np.zeros((K, g), np.int64), np.zeros((K, g), np.int64)
    for j in range(g):
        v = x[j, order].astype(np.float64)
        if np.isnan(v).any():
            rank2[:, j], tie[:, j] = -1, -1
            continue
        if m == 0:
            continue
        perm = np.argsort(v, kind='stable')
        k, c = v[perm], code0[perm]
        pos = np.arange(m)
        head = np.r_[True, k[1:] != k[:-1]]
        tail = np.r_[head[1:], True]
        a = np.maximum.accumulate(np.where(head, pos, -1))
        b = np.minimum.accumulate(np.where(tail, pos + 1, m + 1)[::-1])[::-1]
        if ref < 0:
            np.add.at(rank2[:, j], c, a + b + 1)
            t = (b - a)[head]
            tie[:, j] = (t ** 3 - t).sum()
            continue
        isref = (c == ref).astype(np.int64)
        P = np.r_[0, np.cumsum(isref)]                                  # P[p] = ref cells at positions below p
        np.add.at(rank2[:, j], c, P[a] + P[b])
        tr = P[b] - P[a]
        common = (tr ** 3 - tr)[head].sum()
        shead = head | np.r_[True, c[1:] != c[:-1]]
        stail = np.r_[shead[1:], True]
        sb = np.minimum.accumulate(np.where(stail, pos + 1, m + 1)[::-1])[::-1]
        tc = sb - pos
        sel = shead & (c != ref)
        tie[:, j] = common
        np.add.at(tie[:, j], c[sel], ((tc + tr) ** 3 - tr ** 3 - tc)[sel])
    return rank2, tie


def order_of(codes, K):
    """(order int32 [m], gstart int32 [K + 1], counts int64 [K]) of per-cell codes (-1: in no group): the labelled cells
    group after group, cells ascending inside a group."""
    codes = np.asarray(codes)
    lab = np.flatnonzero(codes >= 0)
    order = lab[np.argsort(codes[lab], kind='stable')].astype(np.int32)
    counts = np.bincount(codes[lab], minlength=K).astype(np.int64)
    return order, np.r_[0, np.cumsum(counts)].astype(np.int32), counts


class RankSumRefOps(CpuRefOps):
    """CpuRefOps + ranksum (include/dcahip.h, dcahip_ranksum) by rank_ref."""
    name = 'cpu-oracle-ranksum'

    def ranksum_workspace_bytes(self, g, n):
        assert g >= 1 and 1 <= n <= 2097151
        return 16

    def ranksum(self, x, ldx, g, n, order, m, gstart, K, ref, rank2, tie, ldr, ws):
        assert 1 <= K <= 4096 and 0 <= m <= n and -1 <= ref < K and ldx >= n and ldr >= g
        o = _vec(order, m) if m else np.zeros(0, np.int64)
        r2, t = rank_ref(_mat(x, g, n, ldx), o, _vec(gstart, K + 1), K, ref)
        _mat(rank2, K, g, ldr)[:] = r2
        _mat(tie, K, g, ldr)[:] = t
