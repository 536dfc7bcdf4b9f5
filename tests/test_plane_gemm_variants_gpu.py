"""Every kernel instantiation and ending the plane products can launch -- dcahip_gemm_p3 (gemm_p3_kernel, gemm_p3w_kernel) and
dcahip_gemm_h2 (gemm_h2w_kernel, gemm_h2m_kernel), four layouts, column sums, the ordered split-K reduce and the tail sum --
against fp64, on the cases of tests/_plane_gemm_cases.py (tests/test_plane_gemm_cases_cpu.py proves on the host that the table
reaches all of them).

Bounds (none of them new, include/dcahip.h): three pieces 5e-7 of sum|ab| (+ |bias|) per element; two pieces 1e-6 alpha
sum|ab| (+ |bias|); the column-sum row as tests/test_gemm_p3_gpu.py and tests/test_gemm_h2_gpu.py hold it.  The planes are
made by the split kernels and then carry the NaN pattern of their type wherever a correct product may not depend on them
(tests/_plane_gemm_cases.py says where)."""
import numpy as np
import pytest
import torch

import _plane_gemm_cases as PC

pytestmark = pytest.mark.gpu

SENTINEL = 123.0
WS_GUARD = 64                  # floats behind the workspace the library asked for


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _bits(t):
    return t.view(torch.int32)


def make_planes(ops, pieces, opnd):
    """The planes of one operand [pieces, rows_alloc, ldp] through the split kernels, poisoned; two pieces: and the exponent word."""
    src = torch.from_numpy(opnd['src']).cuda()
    dtype = torch.bfloat16 if pieces == 3 else torch.float16
    planes = torch.zeros(pieces, opnd['rows_alloc'], opnd['ldp'], dtype=dtype, device='cuda')
    exp = None
    if pieces == 3:
        ops.split_planes(src, opnd['ld'], opnd['R'], opnd['C'], planes)
    else:
        exp = torch.zeros(2, dtype=torch.int32, device='cuda')
        ops.absmax_exp(src, opnd['ld'], opnd['R'], opnd['C'], exp)
        ops.split_planes_h2(src, opnd['ld'], opnd['R'], opnd['C'], planes, exp)
    planes[:, torch.from_numpy(opnd['poison']).cuda()] = float('nan')
    return planes, exp


class Problem:
    """The device operands of one case; run() is one call of the product into a fresh C and a fresh workspace."""

    def __init__(self, ops, case, alpha=PC.ALPHA, **kw):
        self.ops, self.case, self.alpha = ops, case, alpha
        pieces, ta, tb, M, N, K, split, flags = case
        self.o = o = PC.operands(case, **kw)
        self.A, self.ea = make_planes(ops, pieces, o['a'])
        self.B, self.eb = make_planes(ops, pieces, o['b'])
        self.bias = torch.from_numpy(o['bias']).cuda() if o['bias'] is not None else None
        self.perm = torch.from_numpy(o['perm']).cuda() if o['perm'] is not None else None
        self.cursor = torch.tensor([o['cursor']], dtype=torch.int64, device='cuda') if o['cursor'] is not None else None
        self.colsum = 'c' in flags
        self.Mo = M + int(self.colsum)
        self.plan = ops.gemm_planes_plan(pieces, ta, tb, M, N, K, gather=o['cursor'] is not None, colsum_row=self.colsum,
                                         split_k=split)
        assert self.plan[11] % 4 == 0
        self.ws_floats = self.plan[11] // 4

    def run(self, **kw):
        pieces, ta, tb, M, N, K, split, flags = self.case
        o = self.o
        C = torch.full((self.Mo + 1, o['ldc']), SENTINEL, device='cuda')         # one guard row, ldc > N
        ws = torch.full((self.ws_floats + WS_GUARD,), float('nan'), device='cuda')
        wsv = ws[:self.ws_floats] if self.ws_floats else None
        if pieces == 3:
            self.ops.gemm_p3(ta, tb, M, N, K, self.A, self.B, C, o['ldc'], bias=self.bias, perm=self.perm, cursor=self.cursor,
                             colsum_row=self.colsum, split_k=split, ws=wsv)
        else:
            self.ops.gemm_h2(ta, tb, M, N, K, self.A, self.B, C, o['ldc'], exp_a=self.ea, exp_b=self.eb, alpha=self.alpha,
                             bias=self.bias, colsum_row=self.colsum, split_k=split, ws=wsv, **kw)
        torch.cuda.synchronize()
        return C, ws

    def reference(self):
        """(ref, mag) of rows 0 .. M - 1 in fp64, the factor and the bias included."""
        o, f = self.o, (self.alpha if self.case[0] == 2 else 1.0)
        ref = f * (o['opA'] @ o['opB'])
        mag = abs(f) * (np.abs(o['opA']) @ np.abs(o['opB']))
        if o['bias'] is not None:
            ref += o['bias'].astype(np.float64)
            mag += np.abs(o['bias'].astype(np.float64))
        return ref, mag


def kernel_name(pieces, plan):
    return ('gemm_p3_kernel', 'gemm_p3w_kernel' if pieces == 3 else 'gemm_h2w_kernel', 'gemm_h2m_kernel')[plan[0]]


@pytest.mark.parametrize('case', PC.CASES, ids=PC.case_id)
def test_plane_gemm_variant_vs_fp64(ops, case):
    pieces, ta, tb, M, N, K, split, flags = case
    p = Problem(ops, case)
    o = p.o
    kernel, bm, bn, mtiles, ntiles, nsplit, kslab, tfirst, tsplit, tkslab, cs, wsb = p.plan
    C, ws = p.run()
    out = C.cpu().numpy()

    # nothing outside [M (+ 1), N] changes, nothing behind the workspace either; no poisoned plane element and no unwritten
    # workspace element reached the output
    assert (out[p.Mo:] == SENTINEL).all() and (out[:, N:] == SENTINEL).all()
    assert torch.isnan(ws[p.ws_floats:]).all()
    assert np.isfinite(out[:p.Mo, :N]).all(), np.argwhere(~np.isfinite(out[:p.Mo, :N]))[:5]

    ref, mag = p.reference()
    err = np.abs(out[:M, :N].astype(np.float64) - ref)
    tol = (5e-7 if pieces == 3 else 1e-6) * mag + 1e-30
    print('%s: %s %dx%d, split %d, tail %d x %d; max err / sum|ab| = %.3g' % (
        PC.case_id(case), kernel_name(pieces, p.plan), bm, bn, nsplit, mtiles * ntiles - tfirst if tsplit > 1 else 0, tsplit,
        float((err / mag).max())))
    assert (err <= tol).all(), (err.max(), float((err / mag).max()), np.argwhere(err > tol)[:5])
    if p.colsum:
        Bkn = o['opB']
        if pieces == 3:
            np.testing.assert_allclose(out[M, :N], Bkn.sum(axis=0), rtol=0, atol=3e-6 * np.abs(Bkn).sum(axis=0).max())
        else:
            np.testing.assert_allclose(out[M, :N], p.alpha * Bkn.sum(axis=0), rtol=0,
                                       atol=2e-6 * p.alpha * np.abs(Bkn).sum(axis=0).max())

    # deterministic: the same call gives the same bits
    C2, _ = p.run()
    assert torch.equal(_bits(C), _bits(C2))


SCALE_CASES = [c for c in PC.CASES if 's' in c[7]]


def _magnitudes(rng, shape):
    """Entries of magnitude in [1/4, 1): scaled by at most 2^+-40 they, their pieces and every partial sum of their products
    stay far from overflow and from the denormals."""
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 1.0, shape)


@pytest.mark.parametrize('case', [c for c in SCALE_CASES if c[0] == 3], ids=PC.case_id)
def test_gemm_p3_is_invariant_under_power_of_two_scaling(ops, case):
    """Rows of op(A) times 2^a_m, columns of op(B) times 2^b_n, the k-th element of A times 2^s_k and of B times 2^-s_k
    (integers in [-20, 20]): every piece and every product is the unscaled one times a power of two, and so is every
    rounding -- the output equals the unscaled output times 2^(a_m + b_n) bit for bit."""
    pieces, ta, tb, M, N, K, split, flags = case
    rng = np.random.RandomState(31 * M + 17 * N + K)
    a_m, b_n, s_k = (rng.randint(-20, 21, n) for n in (M, N, PC.data_depth(case)))
    plain = Problem(ops, case, values=_magnitudes)
    scaled = Problem(ops, case, values=_magnitudes, scale=(a_m, b_n, s_k))
    assert plain.plan == scaled.plan
    out = plain.run()[0].cpu().numpy()[:M, :N]
    got = scaled.run()[0].cpu().numpy()[:M, :N]
    want = np.ldexp(out, (a_m[:, None] + b_n[None, :]).astype(np.int32))
    assert want.dtype == np.float32 and np.isfinite(want).all() and (np.abs(want) > 1e-30).all()
    differ = np.argwhere(want.view(np.int32) != got.view(np.int32))
    assert differ.size == 0, (len(differ), differ[:5], [(want[i, j], got[i, j]) for i, j in differ[:5]])


@pytest.mark.parametrize('case', [c for c in SCALE_CASES if c[0] == 2], ids=PC.case_id)
def test_gemm_h2_is_invariant_under_power_of_two_scaling(ops, case):
    """All of A times 2^s, all of B times 2^t: the exponent words move by -s and -t, the planes keep their bits, and C is the
    unscaled C times 2^(s + t) bit for bit (the column-sum row times 2^t)."""
    pieces, ta, tb, M, N, K, split, flags = case
    s, t = 7, -11
    plain = Problem(ops, case, values=_magnitudes)
    scaled = Problem(ops, case, values=_magnitudes, scale=(s, t))
    assert int(scaled.ea[0]) == int(plain.ea[0]) - s and int(scaled.eb[0]) == int(plain.eb[0]) - t
    assert -60 < int(scaled.ea[0]) < 60 and -60 < int(scaled.eb[0]) < 60
    assert torch.equal(plain.A.view(torch.int16), scaled.A.view(torch.int16))
    assert torch.equal(plain.B.view(torch.int16), scaled.B.view(torch.int16))
    out = plain.run()[0].cpu().numpy()
    got = scaled.run()[0].cpu().numpy()
    want = out.copy()
    want[:M, :N] = np.ldexp(out[:M, :N], np.int32(s + t))
    if 'c' in flags:
        want[M, :N] = np.ldexp(out[M, :N], np.int32(t))
    assert np.isfinite(want).all() and (np.abs(want[:plain.Mo, :N]) > 1e-30).all()
    differ = np.argwhere(want.view(np.int32) != got.view(np.int32))
    assert differ.size == 0, (len(differ), differ[:5])


# one base per kernel, with column sums where the kernel has them
NAN_CASES = [(3, 0, 0, 130, 131, 1048, 0, 'bc'), (3, 0, 0, 1024, 256, 32, 0, 'c'), (3, 1, 0, 300, 900, 80, 2, 'bc'),
             (2, 0, 0, 256, 1024, 16, 0, 'cs'), (2, 1, 0, 513, 515, 16, 0, 'c'), (2, 0, 0, 513, 515, 272, 0, 'b')]


def _with_nan(which, r, c):
    """values for PC.operands: uniform entries, one NaN in the stored matrix of A (which = 0) or B (1) at [r, c]."""
    calls = []

    def draw(rng, shape):
        x = rng.uniform(-1, 1, shape)
        if len(calls) == which:
            x[r, c] = np.nan
        calls.append(shape)
        return x
    return draw


@pytest.mark.parametrize('case', NAN_CASES, ids=PC.case_id)
def test_nan_stays_nan_and_stays_local(ops, case):
    """A NaN at op(A)[m, k] makes row m of C NaN, one at op(B)[k, n] column n and the column-sum entry n; every other element
    keeps the bits of the clean run.  The block maximum ignores NaN: the exponent words do not move."""
    assert case in PC.CASES
    pieces, ta, tb, M, N, K, split, flags = case
    kd = PC.data_depth(case)
    m, n, k = M - 3, N - 2, kd - 1
    clean = Problem(ops, case, values=_with_nan(2, 0, 0))
    base = clean.run()[0].cpu().numpy()
    assert np.isfinite(base[:clean.Mo, :N]).all()
    for which, (r, c) in ((0, (k, m) if ta else (m, k)), (1, (n, k) if tb else (k, n))):
        p = Problem(ops, case, values=_with_nan(which, r, c))
        if pieces == 2:
            assert int(p.ea[0]) == int(clean.ea[0]) and int(p.eb[0]) == int(clean.eb[0])
        got = p.run()[0].cpu().numpy()
        hit = np.zeros(got.shape, bool)
        if which == 0:
            hit[m, :N] = True
        else:
            hit[:clean.Mo, n] = True
        assert np.isnan(got[hit]).all(), (which, np.argwhere(hit & ~np.isnan(got))[:5])
        same = got.view(np.int32) == base.view(np.int32)
        assert same[~hit].all(), (which, np.argwhere(~same & ~hit)[:5])


# ---- the ends of the block exponent (two pieces, the smallest wide shape, on both kernels)
END_CASES = [(2, 0, 0, 256, 1024, 16, 0, 's'), (2, 1, 0, 256, 1024, 64, 0, '')]


def _block(top, positive=False):
    """values: magnitudes in [1/2, 1) x 2^top, so that the block's maximum lies in [2^(top - 1), 2^top)."""
    def draw(rng, shape):
        sign = 1.0 if positive else rng.choice([-1.0, 1.0], shape)
        return np.ldexp(sign * rng.uniform(0.5, 1.0, shape), top)
    return draw


def _two_blocks(top_a, top_b, positive=False):
    calls = []

    def draw(rng, shape):
        calls.append(shape)
        return _block(top_a if len(calls) == 1 else top_b, positive)(rng, shape)
    return draw


@pytest.mark.parametrize('case', END_CASES, ids=PC.case_id)
@pytest.mark.parametrize('tops', [(-49, 1), (1, -59), (-49, -59)], ids=lambda t: 'A2^%d-B2^%d' % t)
def test_gemm_h2_below_the_supported_range(ops, case, tops):
    """A block whose largest magnitude is 2^-50 or 2^-60 gets the clamped exponent +60: its scaled maximum is 2^10 or 2^0
    and its pieces keep the absolute floor 2^-25 only, i.e. D = 2^-25 2^-e of the data.  The bound is the contract plus that
    floor: 1e-6 alpha sum|ab| + alpha sum(Da |b| + |a| Db)."""
    assert case in PC.CASES
    pieces, ta, tb, M, N, K, split, flags = case
    p = Problem(ops, case, values=_two_blocks(*tops))
    ea, eb = int(p.ea[0]), int(p.eb[0])
    assert (ea, eb) == tuple(60 if t < 0 else 14 - t for t in tops)
    out = p.run()[0].cpu().numpy()[:M, :N]
    assert np.isfinite(out).all()
    ref, mag = p.reference()
    assert (np.abs(ref) > 2.0 ** -126).sum() > 0.99 * ref.size
    da, db = 2.0 ** (-25 - ea), 2.0 ** (-25 - eb)
    floor = p.alpha * (da * np.abs(p.o['opB']).sum(axis=0)[None, :] + db * np.abs(p.o['opA']).sum(axis=1)[:, None])
    err = np.abs(out.astype(np.float64) - ref)
    print('%s A 2^%d B 2^%d: max err / sum|ab| = %.3g, floor / sum|ab| = %.3g' % (
        PC.case_id(case), tops[0], tops[1], float((err / mag).max()), float((floor / mag).max())))
    # (a result below the smallest normal fp32 is rounded to a denormal: half a unit of 2^-149 on top)
    assert (err <= 1e-6 * mag + floor + 2.0 ** -150).all(), float((err / mag).max())


@pytest.mark.parametrize('case', END_CASES, ids=PC.case_id)
def test_gemm_h2_above_the_supported_range_is_never_finite(ops, case):
    """A block whose largest magnitude is 2^80: the clamp at -60 leaves 2^20, beyond fp16 -- every piece is Inf and every
    output non-finite, never a finite wrong number."""
    pieces, ta, tb, M, N, K, split, flags = case
    p = Problem(ops, case, values=_two_blocks(81, 1))
    assert int(p.ea[0]) == -60
    assert torch.isinf(p.A[0][~torch.from_numpy(p.o['a']['poison']).cuda()].float()).all()
    out = p.run()[0].cpu().numpy()
    assert not np.isfinite(out[:M, :N]).any()
    assert (out[M:] == SENTINEL).all() and (out[:, N:] == SENTINEL).all()


@pytest.mark.parametrize('case', END_CASES, ids=PC.case_id)
@pytest.mark.parametrize('sign', [1, -1], ids=['plus126', 'minus126'])
def test_gemm_h2_exponent_sum_at_its_ends_and_one_step_beyond(ops, case, sign):
    """ea + eb = +126 and -126, from blocks at the clamp (+-60 each) and static exponents of +-6 in all: the scale
    2^-(ea + eb) is still a power of two of fp32 and the product meets the contract (the factor alpha keeps the true result,
    and alpha 2^-(ea + eb), among the normal numbers).  One step beyond is refused before any launch: C stays untouched."""
    pieces, ta, tb, M, N, K, split, flags = case
    add_a, add_b = 4 * sign, 2 * sign
    if sign > 0:
        # the data: magnitudes below 2^-60; the planes' producer hands them over times 2^add, and the clamp gives +60
        top_a, top_b, alpha = -60, -60, 1.5
    else:
        # the data: magnitudes in [2^77, 2^78) and [2^75, 2^76); times 2^add both blocks' maxima lie in [2^73, 2^74), the last
        # binade before the clamp at -60 does anything: the scaled maxima are in [2^13, 2^14)
        top_a, top_b, alpha = 78, 76, 1.5 * 2.0 ** -44
    p = Problem(ops, case, alpha=alpha, values=_two_blocks(top_a, top_b, positive=True))
    # what the producer wrote: the data times 2^add (exact); the planes and the words are made from that
    for opnd, add in ((p.o['a'], add_a), (p.o['b'], add_b)):
        opnd['src'] = np.ldexp(opnd['src'], np.int32(add))
    p.A, p.ea = make_planes(ops, 2, p.o['a'])
    p.B, p.eb = make_planes(ops, 2, p.o['b'])
    assert int(p.ea[0]) == 60 * sign and int(p.eb[0]) == 60 * sign
    assert torch.isfinite(p.A[:, ~torch.from_numpy(p.o['a']['poison']).cuda()].float()).all()
    out = p.run(exp_a_add=add_a, exp_b_add=add_b)[0].cpu().numpy()
    ref, mag = p.reference()
    assert np.isfinite(ref).all() and (np.abs(ref) > 2.0 ** -120).all() and (np.abs(ref) < 2.0 ** 120).all()
    err = np.abs(out[:M, :N].astype(np.float64) - ref)
    # below the range (sign > 0) the pieces keep their absolute floor, as in test_gemm_h2_below_the_supported_range
    floor = 0.0
    if sign > 0:
        d = 2.0 ** (-25 - 60)
        floor = alpha * (d * 2.0 ** -add_a * np.abs(p.o['opB']).sum(axis=0)[None, :] + d * 2.0 ** -add_b * np.abs(p.o['opA']).sum(axis=1)[:, None])
    print('%s ea + eb = %d: max err / sum|ab| = %.3g' % (PC.case_id(case), 126 * sign, float((err / mag).max())))
    assert (err <= 1e-6 * mag + floor).all(), float((err / mag).max())
    for da, db in ((sign, 0), (0, sign), (-8 * sign, 3 * sign)):
        C = torch.full((p.Mo + 1, p.o['ldc']), SENTINEL, device='cuda')
        ws = torch.zeros(max(p.ws_floats, 4), device='cuda')
        with pytest.raises(RuntimeError):
            ops.gemm_h2(ta, tb, M, N, K, p.A, p.B, C, p.o['ldc'], exp_a=p.ea, exp_b=p.eb, exp_a_add=add_a + da,
                        exp_b_add=add_b + db, alpha=alpha, ws=ws)
        torch.cuda.synchronize()
        assert (C == SENTINEL).all()
