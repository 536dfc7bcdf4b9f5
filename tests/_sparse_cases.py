"""What the K-SPARSE tests share (tests/test_sparse_edges_gpu.py, tests/test_sparse_cases_cpu.py): numpy only.

  * dense_input / reference_fwd / reference_dw: the fp64 network input X = (f(Y / fac) - mean) / std, Z = X[rows] W + b and
    gW = X[rows]^T dZ with its column-sum row, each with the magnitude its bound is stated against (|err| <= 1e-6 * that);
  * edge_counts: synthetic counts with every lookup class of the byte-store kernels planted where those kernels change path;
  * decode_lut: the per-cell table of dcahip_enc0_lut back to numbers;
  * a restatement of the launch plans (gene chunks of the forward, row splits of the two weight-gradient forms) written from
    include/dcahip.h and the comments of dca_amd/csrc/dcahip_sparse.hip -- used ONLY to assert that a named shape reaches
    the path it is named for: a retuning of those heuristics then fails the tests loudly instead of leaving them testing
    nothing.
"""
import functools

import numpy as np

from conftest import synth_counts


def f32(a):
    """Rounded to fp32 (what a kernel reads), widened to fp64 (what the reference computes with)."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ references
def dense_input(Y, fac, do_log, mean, std):
    x = Y / fac[:, None] if fac is not None else Y.copy()
    if do_log:
        x = np.log1p(x)
    if mean is not None:
        x = x - mean[None, :]
    if std is not None:
        x = x / std[None, :]
    return x


def _terms(Y, fac, do_log, mean, std, rows):
    """L / std of the batch rows and mean / std: the two operands the kernels sum separately."""
    Ls = dense_input(Y, fac, do_log, None, std)[rows]
    ms = None
    if mean is not None:
        ms = mean / std if std is not None else mean.copy()
    return Ls, ms


def reference_fwd(Y, fac, do_log, mean, std, rows, W, b):
    """Z = X[rows] W + b in fp64 and Z_abs = |L / std| |W| + |mean / std| |W| + |b|: the kernel forms L (W / std) and
    sum_g (mean / std) W separately, so with a mean the bound carries both magnitudes (no mean: the second term is absent;
    no std: std = 1; no bias: no |b|)."""
    X = dense_input(Y, fac, do_log, mean, std)[rows]
    Z = X @ W
    Ls, ms = _terms(Y, fac, do_log, mean, std, rows)
    Z_abs = np.abs(Ls) @ np.abs(W)
    if ms is not None:
        Z_abs = Z_abs + (np.abs(ms) @ np.abs(W))[None, :]
    if b is not None:
        Z = Z + b[None, :]
        Z_abs = Z_abs + np.abs(b)[None, :]
    return Z, Z_abs


def reference_dw(Y, fac, do_log, mean, std, rows, dZ):
    """gW = X[rows]^T dZ, the bias row colsum(dZ), gW_abs and the bias row's magnitude max_j sum_c |dZ[c, j]|.
    gW_abs = |L / std|^T |dZ| and, with a mean, |mean / std| (colsum |dZ| + |colsum dZ|): the kernel forms sum_c L dZ and
    mean * colsum(dZ) separately -- the column sum carries the rounding of its |dZ| terms, the product that of its value."""
    X = dense_input(Y, fac, do_log, mean, std)[rows]
    gW = X.T @ dZ
    col = dZ.sum(0)
    Ls, ms = _terms(Y, fac, do_log, mean, std, rows)
    gW_abs = np.abs(Ls).T @ np.abs(dZ)
    if ms is not None:
        gW_abs = gW_abs + np.abs(ms)[:, None] * np.abs(dZ).sum(0)[None, :] + np.abs(ms)[:, None] * np.abs(col)[None, :]
    return gW, col, gW_abs, float(np.abs(dZ).sum(0).max())


# ------------------------------------------------------------------------------------------------ counts
# One value per lookup class: last entry of the forward's LDS table / first beyond it (31, 32), the same for the first
# weight-gradient kernel (63, 64) and for the ring kernel and the table in memory (127, 128), the largest byte that is a
# count (254), an escape whose value is exactly 255, and escapes beyond (256, 70 000).
EDGE_VALUES = (31, 32, 63, 64, 127, 128, 254, 255, 256, 70000)


def edge_positions(nb, G):
    """{value: [(batch row, gene), ...]} -- for every value of EDGE_VALUES, in this order:
         first batch row, a gene of the lower lane half of the forward (gene % 128 < 64)
         first batch row, a gene of its upper lane half (gene % 128 >= 64)
         last batch row
         first gene, a row of the lower lane half of the weight gradient (row % 16 < 8)
         first gene, a row of its upper half (row % 16 >= 8)
         last gene
       Where the matrix is too small for all of it the indices wrap by modulo (later positions then overwrite earlier ones);
       none lies outside [0, nb) x [0, G)."""
    pos = {}
    for i, v in enumerate(EDGE_VALUES):
        up = 8 + (i % 8) + 16 * (i // 8)
        pos[v] = [(0, (1 + i) % G), (0, (64 + 1 + i) % G), (nb - 1, (G - 2 - i) % G),
                  ((1 + (i % 7) + 16 * (i // 7)) % nb, 0), (up % nb, 0), ((nb - 2 - i) % nb, G - 1)]
    return pos


def edge_rows(nb, G):
    """Batch rows of the row that is all escapes and of the row that is all zeros: the first two rows from nb // 3 on
    that hold no planted value.  A batch without two such rows (fewer than 35 rows) takes nb // 3 and 2 nb // 3, and the
    planted values then overwrite part of them."""
    taken = {r for cells in edge_positions(nb, G).values() for r, _ in cells}
    free = [r % nb for r in range(nb // 3, nb // 3 + nb) if r % nb not in taken]
    if len(free) >= 2:
        return free[0], free[1]
    return (nb // 3) % nb, (2 * nb // 3) % nb


@functools.lru_cache(maxsize=None)
def _synth(n, G, seed):
    """(computed once per shape: the tests that share a shape plant into copies)"""
    return synth_counts(n, G, seed)


def edge_counts(n, G, seed, rows=None):
    """synth_counts(n, G, seed) with, over the batch rows `rows` (storage rows in batch order; default all n in order):
    one row entirely >= 255 (the overflow scan runs in every lane of a K step and the row's list is G long), one row
    entirely 0, then EDGE_VALUES at edge_positions."""
    Y = _synth(n, G, seed).copy()
    rows = np.arange(n) if rows is None else np.asarray(rows)
    nb = len(rows)
    big, zero = edge_rows(nb, G)
    Y[rows[big], :] = 255 + (np.arange(G) * 37) % 1500
    if zero != big:
        Y[rows[zero], :] = 0
    for v, cells in edge_positions(nb, G).items():
        for r, g in cells:
            Y[rows[r], g] = v
    return Y


# ------------------------------------------------------------------------------------------------ the table
def decode_lut(lutp):
    """int32 [n, 128, 2] of dcahip_enc0_lut -> fp64 [n, 128]: an entry is {p0 | p1 << 16, p2}, each piece a bf16."""
    w = np.ascontiguousarray(lutp).astype(np.int64) & 0xffffffff
    assert w.ndim == 3 and w.shape[2] == 2
    assert ((w[..., 1] >> 16) == 0).all(), 'high half of the second word is not 0'
    bf = lambda bits: (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return bf(w[..., 0] & 0xffff) + bf(w[..., 0] >> 16) + bf(w[..., 1] & 0xffff)


# ------------------------------------------------------------------------------------------------ the plans
def _cdiv(a, b):
    return (a + b - 1) // b


def compact_ld(G):
    return _cdiv(G, 16) * 16


# forward: a workgroup holds 256 batch rows; the genes go in super steps of 128 (two macro steps of 64); about 256
# workgroups in all, at most 32 gene chunks of whole super steps
def fl_row_groups(B):
    return _cdiv(B, 256)


def fl_n_ms(G):
    return 2 * _cdiv(G, 128)


def fl_ms_per(B, G):
    nsk = max(1, min(32, 256 // fl_row_groups(B)))
    return 2 * _cdiv(fl_n_ms(G) // 2, nsk)


def fl_plan(B, G):
    n_ms, per = fl_n_ms(G), fl_ms_per(B, G)
    chunks = _cdiv(n_ms, per)
    return dict(row_groups=fl_row_groups(B), ldc=compact_ld(G), n_ms=n_ms, ms_per=per, chunks=chunks,
                last_chunk_ms=n_ms - (chunks - 1) * per)


# weight gradient, first form: 256 genes per workgroup, row splits of whole 64-row blocks, at most 16 splits (about one
# workgroup per CU), at most 2048 rows per split.  Ring form (64 units; by the shape from 1024 rows): 512 genes per
# workgroup, splits of whole 16-row K steps, at most 1024 rows per split.
def dw_second_form(H1, B, form):
    return H1 == 64 and (form == 2 or (form == 0 and B >= 1024))


def _splits(B, groups, rb, max_rs):
    ns = max(1, min(256 // groups, _cdiv(B, rb), 16))
    return max(ns, _cdiv(B, max_rs))


def dw2_splits(B, G):
    return _splits(B, _cdiv(G, 512), 16, 1024)


def dw_splits(B, G, H1, form):
    if dw_second_form(H1, B, form):
        return dw2_splits(B, G)
    return _splits(B, _cdiv(G, 256), 64, 2048)


def dw_rows_per_split(B, ns, H1, form):
    rb = 16 if dw_second_form(H1, B, form) else 64
    return _cdiv(_cdiv(B, ns), rb) * rb


def dw_plan(B, G, H1, form):
    """groups: gene groups (workgroups per split); splits; rows per split; units per split (64-row blocks of the first form,
    16-row K steps of the ring form); empty: splits that receive no row; last_rows: rows of the last split that has any."""
    ring = dw_second_form(H1, B, form)
    ns = dw_splits(B, G, H1, form)
    rs = dw_rows_per_split(B, ns, H1, form)
    used = _cdiv(B, rs)
    return dict(ring=ring, groups=_cdiv(G, 512 if ring else 256), splits=ns, rows_per_split=rs,
                units_per_split=rs // (16 if ring else 64), empty=ns - used, last_rows=B - (used - 1) * rs)


# ------------------------------------------------------------------------------------------------ the named shapes
# (B, G) -> what the shape is there for, as numbers of fl_plan: asserted by the CPU test and again before every launch.
FWD_SHAPES = [
    ((1, 1), dict(row_groups=1, ldc=16, chunks=1)),                        # one live row, one gene
    ((31, 16), dict(row_groups=1, ldc=16, chunks=1)),                      # below one wave
    ((33, 17), dict(row_groups=1, ldc=32, chunks=1)),                      # above one wave
    ((32, 63), dict(row_groups=1, ldc=64, chunks=1)),                      # the upper lane half never holds a stored byte
    ((255, 64), dict(row_groups=1, ldc=64, chunks=1)),                     # the 256-row boundary ...
    ((256, 65), dict(row_groups=1, ldc=80, chunks=1)),                     # ... ldc ends inside the upper half's loads
    ((257, 127), dict(row_groups=2, ldc=128, chunks=1)),                   # ... a second row group of one row
    ((40, 128), dict(n_ms=2, chunks=1)),                                   # on a super step
    ((70, 129), dict(n_ms=4, ms_per=2, chunks=2)),                         # one past it
    ((64, 257), dict(n_ms=6, ms_per=2, chunks=3)),
    ((40, 4230), dict(row_groups=1, ms_per=4, chunks=17, last_chunk_ms=4)),
    ((2305, 3400), dict(row_groups=10, ms_per=4, chunks=14, last_chunk_ms=2)),
    ((2100, 40), dict(row_groups=9, chunks=1)),
]

# (B, G) -> numbers of dw_plan for the first form (32, 64 and 128 units alike) and for the ring form (64 units)
DW_SHAPES = [
    ((1, 1), dict(groups=1, splits=1, units_per_split=1), dict(groups=1, splits=1, units_per_split=1)),
    ((15, 17), dict(groups=1, splits=1, units_per_split=1, last_rows=15), dict(splits=1, units_per_split=1)),
    ((33, 255), dict(groups=1, splits=1, units_per_split=1), dict(groups=1, splits=3, units_per_split=1, last_rows=1)),
    ((257, 127), dict(splits=5, units_per_split=1, empty=0, last_rows=1), dict(splits=16, units_per_split=2, empty=7, last_rows=1)),
    ((150, 520), dict(groups=3, splits=3, units_per_split=1), dict(groups=2, splits=10, units_per_split=1)),
    ((2100, 40), dict(splits=16, rows_per_split=192, units_per_split=3, empty=5, last_rows=180),
     dict(splits=16, rows_per_split=144, units_per_split=9, empty=1, last_rows=84)),
    ((2305, 3400), dict(groups=14, splits=16, units_per_split=3, empty=3, last_rows=1),
     dict(groups=7, splits=16, units_per_split=10, empty=1, last_rows=65)),
    ((4200, 33), dict(splits=16, rows_per_split=320, units_per_split=5, empty=2, last_rows=40),
     dict(splits=16, rows_per_split=272, units_per_split=17, empty=0, last_rows=120)),
]
