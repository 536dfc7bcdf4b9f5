"""The cases of the dcahip_sgemm variant tests: plain data and the helper that builds the operands of one case (numpy
only).  tests/test_gemm_variants_cpu.py keeps the table complete against the host-side plan query dcahip_sgemm_plan (which
tile, arithmetic and loader width a case reaches), tests/test_gemm_variants_gpu.py runs every case against fp64.

A case is (ta, tb, M, N, K, split_k, align, flags).
  ta, tb   : the layout -- NN (0, 0), TN (1, 0: A stored [K, M]), NT (0, 1: B stored [N, K])
  split_k  : 0 the library's heuristic, -1 the exact-fp32 kernels with that heuristic, > 0 forced
  align    : 'v4'   both operands 16-byte aligned, lda and ldb multiples of 4 (16-byte loads), or ONE reason for scalar loads:
             'lda'  lda % 4 == 1          'ldb'  ldb % 4 == 1
             'offA' A starts one float past a 16-byte boundary          'offB' the same for B
  flags    : any of
             b  bias [N]                                  c  column sums of B into row M of C (NN and TN)
             p  A's storage rows gathered through perm[cursor + r]      u  cursor without perm: storage row cursor + r
             l  ldc not a multiple of 4                   s  a base of the scale-invariance test (no b, no c)
"""
import numpy as np

NN, TN, NT = (0, 0), (1, 0), (0, 1)
LAYOUTS = {'NN': NN, 'TN': TN, 'NT': NT}
ALIGNS = ('v4', 'lda', 'ldb', 'offA', 'offB')
CURSOR = 5                     # first row of the batch in perm (flag p) or in the storage (flag u)
SPARE_ROWS = 4                 # storage rows behind the batch that no case may read


def _rows(layout, shapes):
    return [layout + r for r in shapes]


# One block per tile of make_plan; every base shape in the three layouts, aligned and with one reason for scalar loads, over
# split_k 0 / -1 / 3, once with a ragged ldc.  What each row reaches is not written here: the CPU test asks the library.
CASES = (
    # ---- 128 x 64 tiles (N <= 64, M < 2048): bases 45 x 6 x 3 (K < 32, one ragged tile), 130 x 33 x 70, 2047 x 64 x 40
    _rows(NN, [(45, 6, 3, 0, 'v4', 'bc'), (45, 6, 3, -1, 'lda', ''), (130, 33, 70, 0, 'v4', 's'), (130, 33, 70, 3, 'offB', 'l'),
               (2047, 64, 40, 0, 'v4', 'p'), (2047, 64, 40, -1, 'ldb', '')])
    + _rows(TN, [(45, 6, 3, 0, 'v4', 'c'), (45, 6, 3, 3, 'offA', ''),              # forced 3 of one K chunk: no split left
                 (130, 33, 70, 0, 'v4', 's'), (130, 33, 70, -1, 'ldb', 'c'),
                 (2047, 64, 40, 0, 'v4', 'l'), (2047, 64, 40, 3, 'lda', 'p')])     # forced 3 of two K chunks: 2
    + _rows(NT, [(45, 6, 3, 0, 'v4', 'l'), (45, 6, 3, -1, 'offB', ''), (130, 33, 70, 0, 'v4', 's'), (130, 33, 70, 3, 'lda', 'b'),
                 (2047, 64, 40, -1, 'v4', 's'), (2047, 64, 40, 0, 'offA', 'l')])
    # ---- 64 x 128 tiles (N > 64, M <= 64): bases 33 x 130 x 70, 64 x 65 x 99 (NN with N < 128: exact)
    + _rows(NN, [(33, 130, 70, 0, 'v4', 's'), (33, 130, 70, -1, 'v4', 's'), (33, 130, 70, 3, 'ldb', 'c'),
                 (33, 130, 70, -1, 'offA', ''), (64, 65, 99, 0, 'v4', 'bcl'), (64, 65, 99, 3, 'lda', 'bc')])
    + _rows(TN, [(33, 130, 70, 0, 'v4', 's'), (33, 130, 70, 3, 'offB', 'c'), (64, 65, 99, -1, 'v4', 'l'),
                 (64, 65, 99, 0, 'lda', 'p')])
    + _rows(NT, [(33, 130, 70, 0, 'v4', 's'), (33, 130, 70, -1, 'ldb', 'l'), (64, 65, 99, -1, 'v4', 's'),
                 (64, 65, 99, 3, 'offA', 'l'), (64, 65, 99, 7, 'v4', '')])         # forced 7 of four K chunks: 4
    # ---- 128 x 128 tiles (M * N > 2048 * 512): bases 1030 x 1021 x 70, 8300 x 127 x 40 (NN with N < 128: exact)
    + _rows(NN, [(1030, 1021, 70, 0, 'v4', 's'), (1030, 1021, 70, 3, 'offA', 'b'), (1030, 1021, 70, -1, 'ldb', ''),
                 (8300, 127, 40, 0, 'v4', 's'), (8300, 127, 40, 3, 'lda', 'l')])
    + _rows(TN, [(1030, 1021, 70, 0, 'v4', 's'), (1030, 1021, 70, -1, 'offB', 'l'), (8300, 127, 40, 0, 'v4', 'c'),
                 (8300, 127, 40, 3, 'offA', '')])
    + _rows(NT, [(1030, 1021, 70, 0, 'v4', 's'), (1030, 1021, 70, 3, 'ldb', ''), (8300, 127, 40, -1, 'v4', 's'),
                 (8300, 127, 40, -1, 'lda', '')])
    # ---- 64 x 64 tiles, skinny outputs (N <= 64, M >= 2048): bases 2049 x 33 x 70, 2048 x 64 x 40
    + _rows(NN, [(2049, 33, 70, 0, 'v4', 'b'), (2049, 33, 70, 3, 'offB', ''), (2048, 64, 40, 0, 'v4', 'u'),
                 (2048, 64, 40, -1, 'lda', 'l')])
    + _rows(TN, [(2049, 33, 70, 0, 'v4', 'l'), (2049, 33, 70, -1, 'offA', ''), (2048, 64, 40, 0, 'v4', 'c'),
                 (2048, 64, 40, 3, 'ldb', 'u')])
    + _rows(NT, [(2049, 33, 70, 0, 'v4', 'l'), (2049, 33, 70, -1, 'lda', ''), (2048, 64, 40, -1, 'v4', ''),
                 (2048, 64, 40, 3, 'offB', 'p')])
    # ---- 64 x 64 tiles, mid-size outputs (M > 64, N > 64, M * N <= 2048 * 512): bases 130 x 131 x 70, 257 x 190 x 99
    + _rows(NN, [(130, 131, 70, 0, 'v4', 's'), (130, 131, 70, -1, 'v4', 's'), (130, 131, 70, 3, 'lda', 'l'),
                 (257, 190, 99, 0, 'v4', 'bc'), (257, 190, 99, -1, 'offB', '')])
    + _rows(TN, [(130, 131, 70, 0, 'v4', 's'), (130, 131, 70, 3, 'ldb', ''), (257, 190, 99, 0, 'v4', 'c'),
                 (257, 190, 99, -1, 'offA', 'l')])
    + _rows(NT, [(130, 131, 70, 0, 'v4', 's'), (130, 131, 70, -1, 'v4', 's'), (130, 131, 70, 3, 'offA', 'l'),
                 (257, 190, 99, 0, 'v4', 'p'), (257, 190, 99, 3, 'ldb', '')])      # forced 3 of four K chunks: 2 of 2 chunks
    # ---- the endings: 16 or more splits of at most 65536 outputs (16 lanes per output), and of more (one lane)
    + _rows(NN, [(32, 64, 1000, 0, 'v4', 'bp'), (33, 130, 2100, 0, 'v4', 'c'), (2049, 33, 2100, 0, 'ldb', 'b')])
    + _rows(TN, [(33, 130, 2100, 0, 'lda', 'c')])
    + _rows(NT, [(2049, 33, 2100, 0, 'v4', '')])
    # ---- the other side of the plan's boundaries: M = 65 and N = 65 (64 x 64 mid), N = 64 at M = 130, N = 128 at M = 8300
    #      (three bf16 pieces), M * N = 2048 * 512 (64 x 64) and one row more (128 x 128)
    + _rows(NN, [(65, 130, 70, 0, 'v4', ''), (8300, 128, 40, 0, 'v4', '')])
    + _rows(TN, [(130, 64, 70, 0, 'v4', '')])
    + _rows(NT, [(130, 65, 70, 0, 'v4', ''), (2048, 512, 40, 0, 'v4', ''), (2049, 512, 40, 0, 'v4', '')])
)


def case_id(case):
    ta, tb, M, N, K, split, align, flags = case
    return '%s-%dx%dx%d-s%d-%s%s' % ('TN' if ta else 'NT' if tb else 'NN', M, N, K, split, align, '-' + flags if flags else '')


def r4(n):
    return n + (-n) % 4


def leading_dims(case):
    """(lda, ldb, ldc) of a case.  An aligned leading dimension leaves four floats of padding behind every row."""
    ta, tb, M, N, K, split, align, flags = case
    ca = M if ta else K
    cb = K if tb else N
    lda = r4(ca) + 4 + (1 if align == 'lda' else 0)
    ldb = r4(cb) + 4 + (1 if align == 'ldb' else 0)
    ldc = r4(N) + 4 + (3 if 'l' in flags else 0)
    return lda, ldb, ldc


def offsets(case):
    """Floats between a 64-byte aligned allocation and the first element of A and of B."""
    align = case[6]
    return (1 if align == 'offA' else 0), (1 if align == 'offB' else 0)


def operands(case, values=None, scale=None):
    """The fp32 operands of a case as the kernel sees them, and the fp64 matrices the reference multiplies.

    a_store [rows, lda], b_store [rows, ldb]: storage images.  Everything a correct kernel never reads is NaN: the padding
    behind every row, and with a gather every storage row outside the batch (the rows perm names before the cursor too).
    perm (int32 or None), cursor (int or None), bias (fp32 or None); opA [M, K], opB [K, N] in fp64 from the fp32 values.
    values: a function (rng, shape) -> array for the entries (default: uniform in (-1, 1)).
    scale: integer exponents (a_m [M], b_n [N], s_k [K]): op(A)[m, k] is multiplied by 2^(a_m + s_k) and op(B)[k, n] by
    2^(b_n - s_k), exactly, so that the product is the unscaled one times 2^(a_m + b_n)."""
    ta, tb, M, N, K, split, align, flags = case
    rng = np.random.RandomState(7 * M + 3 * N + K + 1000 * ta + 2000 * tb + 10 * ALIGNS.index(align) + max(split, 0))
    draw = values or (lambda r, shape: r.uniform(-1, 1, shape))
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    lda, ldb, ldc = leading_dims(case)
    A = np.asarray(draw(rng, (ra, ca)), np.float32)
    Bm = np.asarray(draw(rng, (rb, cb)), np.float32)
    if scale is not None:
        a_m, b_n, s_k = (np.asarray(e, np.int32) for e in scale)
        A = np.ldexp(A, (s_k[:, None] + a_m[None, :]) if ta else (a_m[:, None] + s_k[None, :]))
        Bm = np.ldexp(Bm, (b_n[:, None] - s_k[None, :]) if tb else (b_n[None, :] - s_k[:, None]))
        assert A.dtype == np.float32 and Bm.dtype == np.float32
    perm = cursor = None
    if 'p' in flags:
        n_store = CURSOR + ra + SPARE_ROWS
        order = rng.permutation(n_store).astype(np.int32)
        perm, cursor = order[:CURSOR + ra].copy(), CURSOR
        rows = perm[CURSOR:]
    elif 'u' in flags:
        n_store, cursor = CURSOR + ra + SPARE_ROWS, CURSOR
        rows = np.arange(CURSOR, CURSOR + ra)
    else:
        n_store, rows = ra, np.arange(ra)
    a_store = np.full((n_store, lda), np.nan, np.float32)
    a_store[rows, :ca] = A
    b_store = np.full((rb, ldb), np.nan, np.float32)
    b_store[:, :cb] = Bm
    bias = rng.uniform(-1, 1, N).astype(np.float32) if 'b' in flags else None
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    return dict(a_store=a_store, b_store=b_store, perm=perm, cursor=cursor, bias=bias, lda=lda, ldb=ldb, ldc=ldc,
                opA=A64.T if ta else A64, opB=B64.T if tb else B64)
