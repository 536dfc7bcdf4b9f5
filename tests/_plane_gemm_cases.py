"""The cases of the plane-product variant tests (dcahip_gemm_p3: three bf16 pieces; dcahip_gemm_h2: two fp16 pieces): plain
data, the helper that builds the operands of one case, and numpy restatements of the split kernels (numpy only).
tests/test_plane_gemm_cases_cpu.py keeps the table complete against the host-side plan query dcahip_gemm_planes_plan,
tests/test_plane_gemm_variants_gpu.py runs every case against fp64, tests/test_plane_split_gpu.py compares the split kernels
with the restatements bit for bit.

A case is (pieces, ta, tb, M, N, K, split_k, flags).
  pieces   : 3 dcahip_gemm_p3, 2 dcahip_gemm_h2
  ta, tb   : NN (0, 0), NT (0, 1: B stored [N, K]), TN (1, 0: A stored [K, M]), TT (1, 1)
  K        : as passed to the product.  With an operand contiguous along k (every layout but TN) it is a multiple of 8; where
             K % 16 == 8 the data are three shorter (K - 3) and the rest is the zero padding include/dcahip.h asks for
  split_k  : 0 the library's heuristic, > 0 forced
  flags    : any of
             b  bias [N]                                  c  column sums of B into row M of C (NN and TN)
             p  A's storage rows gathered through perm[cursor + r]      u  cursor without perm (three pieces only, both)
             l  ldc not a multiple of 4                   s  a base of the scale-invariance test
"""
import numpy as np

NN, NT, TN, TT = (0, 0), (0, 1), (1, 0), (1, 1)
LAYOUTS = {'NN': NN, 'NT': NT, 'TN': TN, 'TT': TT}
CURSOR = 5                     # first row of the batch in perm (flag p) or in the storage (flag u)
SPARE_ROWS = 4                 # storage rows behind the batch that no case may read
ALPHA = 0.37                   # the caller's factor of the two-piece product
TAIL_CASES = ((3, 0, 1, 256, 65537, 128), (3, 0, 1, 256, 65536, 128), (2, 1, 0, 300, 33000, 128))


def _rows(pieces, layout, shapes):
    return [(pieces,) + layout + r for r in shapes]


# What each row reaches is not written here: the CPU test asks the library.
CASES = tuple(
    # ---- gemm_p3_kernel (128 x 128 tiles): one ragged tile, two by two, three by one; K = 8, 40, 264 (the heuristic splits
    #      from nine K chunks on) and 1048; every layout with perm + cursor and with the cursor alone
    _rows(3, NN, [(45, 6, 8, 0, 'bc'), (130, 131, 40, 0, 's'), (257, 100, 264, 0, 'l'), (130, 131, 1048, 0, 'bc'),
                  (45, 6, 40, 3, 'p'), (257, 100, 40, 0, 'u')])                    # forced 3 of two K chunks: 2
    + _rows(3, NT, [(45, 6, 8, 0, 'l'), (130, 131, 40, 0, 's'), (257, 100, 264, 0, 'b'), (130, 131, 40, 0, 'p'),
                    (257, 100, 1048, 0, 'u')])
    + _rows(3, TN, [(45, 6, 37, 0, 'c'), (130, 131, 40, 0, 's'), (257, 100, 264, 0, 'cp'), (130, 131, 1048, 0, 'u'),
                    (45, 6, 8, 0, 'bl')])
    + _rows(3, TT, [(45, 6, 8, 0, ''), (130, 131, 40, 0, 's'), (257, 100, 264, 3, 'b'), (130, 131, 40, 0, 'p'),
                    (257, 100, 1048, 0, 'ul')])
    # ---- gemm_p3w_kernel (256 x 256 tiles, eight waves): bases 256 x 1024, 1024 x 256, 300 x 900, 513 x 515; K = 16, 32, 48
    #      (one, two, three steps of the ring), 64, 272 (the heuristic split) and a forced split of 80 whose last slab is one step
    + _rows(3, NN, [(256, 1024, 16, 0, 's'), (300, 900, 48, 0, 'b'), (513, 515, 272, 0, 'bl'), (300, 900, 64, 0, ''),
                    (1024, 256, 32, 0, 'c'), (300, 900, 80, 2, 'c'), (513, 515, 64, 0, 'bc')])
    + _rows(3, NT, [(1024, 256, 16, 0, ''), (513, 515, 32, 0, 's'), (300, 900, 272, 0, 'b'), (256, 1024, 80, 2, 'l')])
    + _rows(3, TN, [(300, 900, 16, 0, ''), (256, 1024, 48, 0, 's'), (1024, 256, 272, 0, ''), (513, 515, 64, 0, 'l'),
                    (513, 515, 32, 0, 'c'), (300, 900, 80, 2, 'bc'), (256, 1024, 272, 0, 'c')])
    + _rows(3, TT, [(513, 515, 48, 0, 's'), (1024, 256, 64, 0, 'b'), (300, 900, 80, 2, ''), (256, 1024, 272, 0, '')])
    # ---- gemm_h2w_kernel (the same body on two pieces; NN reaches it with column sums only)
    + _rows(2, NN, [(256, 1024, 16, 0, 'cs'), (300, 900, 48, 0, 'bc'), (513, 515, 272, 0, 'c'), (1024, 256, 80, 2, 'cl')])
    + _rows(2, NT, [(1024, 256, 32, 0, 's'), (513, 515, 16, 0, 'b'), (300, 900, 272, 0, 'b'), (256, 1024, 80, 2, '')])
    + _rows(2, TN, [(300, 900, 32, 0, 's'), (256, 1024, 64, 0, ''), (1024, 256, 272, 0, 'l'), (513, 515, 48, 0, ''),
                    (513, 515, 16, 0, 'c'), (300, 900, 80, 2, 'bc'), (1024, 256, 64, 0, 'c')])
    + _rows(2, TT, [(513, 515, 48, 0, 's'), (1024, 256, 16, 0, 'b'), (300, 900, 80, 2, ''), (256, 1024, 272, 0, 'l')])
    # ---- gemm_h2m_kernel (128 x 256 tiles, four waves: NN without column sums)
    + _rows(2, NN, [(256, 1024, 16, 0, 's'), (1024, 256, 32, 0, 'b'), (300, 900, 48, 0, 'l'), (513, 515, 64, 0, ''),
                    (513, 515, 272, 0, 'b'), (300, 900, 80, 2, 'b')])
    # ---- the other side of the plan's boundaries: M = 255, N = 255, M N = 2^18 - 256, K % 16 == 8, a gather at a wide shape
    + _rows(3, NT, [(255, 1100, 64, 0, ''), (256, 1023, 64, 0, ''), (300, 900, 64, 0, 'u')])
    + _rows(3, TN, [(1100, 255, 64, 0, '')])
    + _rows(3, NN, [(256, 1024, 40, 0, ''), (300, 900, 64, 0, 'p')])
    # ---- the tail sum: 257 tiles (one tail tile in two K slices) next to 256 (none); with column sums two tile rows, 258 tiles
    + _rows(3, NT, [(256, 65537, 128, 0, 'b'), (256, 65536, 128, 0, '')])
    + _rows(2, TN, [(300, 33000, 128, 0, 'bc')])
)


def layout_name(case):
    return {v: k for k, v in LAYOUTS.items()}[(case[1], case[2])]


def case_id(case):
    pieces, ta, tb, M, N, K, split, flags = case
    return 'p%d-%s-%dx%dx%d-s%d%s' % (pieces, layout_name(case), M, N, K, split, '-' + flags if flags else '')


def r8(n):
    return n + (-n) % 8


def r4(n):
    return n + (-n) % 4


def data_depth(case):
    """The K of the data: K - 3 where the passed K is the zero-padded one (a k-contiguous operand and K % 16 == 8)."""
    pieces, ta, tb, M, N, K, split, flags = case
    return K - 3 if ((not ta or tb) and K % 16 == 8) else K


def ldc_of(case):
    N, flags = case[4], case[7]
    return r4(N) + 4 + (3 if 'l' in flags else 0)


def _operand(mat, kc, rows, n_store, rows_pass, ext_pass):
    """One operand.  mat: its fp32 data [r, c]; kc: contiguous along k; rows: the storage row of every passed row (passed
    rows behind the data are zero rows); n_store: storage rows.  Returns the fp32 source image (ld = r8(columns) + 8, NaN
    behind every row's data), the extent the split kernel gets, the geometry of the planes and the mask of the plane
    elements a correct product cannot depend on."""
    r, c = mat.shape
    ld = r8(c) + 8
    ldp = r8(ext_pass) + 8
    dense = np.array_equal(rows, np.arange(len(rows)))   # no gather: the split stops at the last passed row
    src = np.full((n_store, ld), np.nan, np.float32)
    if not dense:
        src[:, :c] = 0.25                                # storage rows outside the batch: finite here, poisoned in the planes
    src[rows[:r], :c] = mat
    src[rows[r:rows_pass], :c] = 0.0                     # zero rows of an operand whose rows are k
    poison = np.zeros((n_store, ldp), bool)
    # columns behind the 16-byte units a tile reads; for an operand contiguous along m / n the columns extent .. r8(extent) too
    # (they reach outputs that are never stored).  A k-contiguous operand's K padding (c .. ext_pass) must stay zero.
    poison[:, (r8(ext_pass) if kc else ext_pass):] = True
    unused = np.ones(n_store, bool)
    unused[rows[:rows_pass]] = False
    poison[unused] = True
    return dict(src=src, ld=ld, R=rows_pass if dense else n_store, C=c, rows_alloc=n_store, ldp=ldp, poison=poison)


def operands(case, values=None, scale=None):
    """The operands of a case and the fp64 matrices the reference multiplies.

    a, b: dicts of _operand -- the test splits src [R, C] (leading dimension ld) into zeroed planes [pieces][rows_alloc][ldp] on the device
    and then writes the NaN pattern of the plane type wherever `poison` is set.  perm (int32 or None), cursor (int or None),
    bias (fp32 or None), ldc; opA [M, k], opB [k, N] in fp64 from the fp32 values (k = data_depth(case)).
    values: a function (rng, shape) -> array for the entries (default: uniform in (-1, 1)).
    scale, three pieces: integer exponents (a_m [M], b_n [N], s_k [k]): op(A)[m, k] is multiplied by 2^(a_m + s_k) and
    op(B)[k, n] by 2^(b_n - s_k), exactly.  Two pieces: (s, t), all of A times 2^s and all of B times 2^t."""
    pieces, ta, tb, M, N, K, split, flags = case
    kd = data_depth(case)
    rng = np.random.RandomState(7 * M + 3 * N + K + 1000 * ta + 2000 * tb + 10 * pieces + split)
    draw = values or (lambda r, shape: r.uniform(-1, 1, shape))
    ra, ca = (kd, M) if ta else (M, kd)
    rb, cb = (N, kd) if tb else (kd, N)
    A = np.asarray(draw(rng, (ra, ca)), np.float32)
    Bm = np.asarray(draw(rng, (rb, cb)), np.float32)
    if scale is not None and pieces == 3:
        a_m, b_n, s_k = (np.asarray(e, np.int32) for e in scale)
        A = np.ldexp(A, (s_k[:, None] + a_m[None, :]) if ta else (a_m[:, None] + s_k[None, :]))
        Bm = np.ldexp(Bm, (b_n[:, None] - s_k[None, :]) if tb else (b_n[None, :] - s_k[:, None]))
    elif scale is not None:
        A, Bm = np.ldexp(A, np.int32(scale[0])), np.ldexp(Bm, np.int32(scale[1]))
    assert A.dtype == np.float32 and Bm.dtype == np.float32
    ra_pass = K if ta else M                              # storage rows the product names
    rb_pass = N if tb else K
    perm = cursor = None
    if 'p' in flags:
        n_store = CURSOR + ra_pass + SPARE_ROWS
        order = rng.permutation(n_store).astype(np.int32)
        perm, cursor = order[:CURSOR + ra_pass].copy(), CURSOR
        rows = perm[CURSOR:]
    elif 'u' in flags:
        n_store, cursor = CURSOR + ra_pass + SPARE_ROWS, CURSOR
        rows = np.arange(CURSOR, CURSOR + ra_pass)
    else:
        n_store, rows = ra_pass + SPARE_ROWS, np.arange(ra_pass)
    a = _operand(A, not ta, rows, n_store, ra_pass, M if ta else K)
    b = _operand(Bm, bool(tb), np.arange(rb_pass), rb_pass + SPARE_ROWS, rb_pass, K if tb else N)
    bias = rng.uniform(-1, 1, N).astype(np.float32) if 'b' in flags else None
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    return dict(a=a, b=b, perm=perm, cursor=cursor, bias=bias, ldc=ldc_of(case),
                opA=A64.T if ta else A64, opB=B64.T if tb else B64)


# ---- numpy restatements of the split kernels (what tests/test_plane_split_gpu.py compares bits against)

def block_exp(m):
    """h2_block_exp: the exponent that brings a block's largest magnitude m into [2^13, 2^14), clamped to [-60, 60]; 0 for an
    all-zero block and for a non-finite maximum."""
    m = np.float32(m)
    if not (m > 0) or not np.isfinite(m):
        return 0
    e = 14 - int(np.frexp(m)[1])
    return max(-60, min(60, e))


def h2_split(x, e):
    """dcahip_split_planes_h2 on fp32 x with block exponent e: (h1, h2) as numpy.float16 -- round to nearest even of the fp32
    product x 2^e, then of the exact fp32 residual."""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        xs = x * np.float32(2.0 ** int(e))
        h1 = xs.astype(np.float16)
        h2 = (xs - h1.astype(np.float32)).astype(np.float16)
    return h1, h2


def bf16_rne(x):
    """fp32 -> the 16 bits of its bf16 (round to nearest even on the upper 16 bits; finite values)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def p3_split(x):
    """dcahip_split_planes on fp32 x: the three bf16 pieces as uint16 bit patterns -- bf16_rne of x, of the exact fp32
    residual, and of that one's residual."""
    r = np.asarray(x, np.float32)
    out = []
    for _ in range(3):
        h = bf16_rne(r)
        out.append(h)
        r = r - bf16_to_f32(h)
    return out


def split_inputs(rng, shape, pieces):
    """The values the split kernels are compared on.  Two pieces: six decades below the block's maximum, so that second
    pieces reach the fp16 denormals and vanish; three pieces: magnitudes in [2^-100, 2^100] (where the bf16 conversion
    flushes is not pinned).  Both with +0 and -0."""
    if pieces == 2:
        x = rng.standard_normal(shape) * np.exp(rng.uniform(-14, 0, shape))
    else:
        x = np.ldexp(rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape), rng.randint(-99, 101, shape))
    x = np.asarray(x, np.float32).reshape(-1)
    x[::17] = 0.0
    x[5::29] = -0.0
    return x.reshape(shape)
