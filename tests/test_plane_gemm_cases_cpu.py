"""The case table of the plane-product variant tests (tests/_plane_gemm_cases.py) reaches every (kernel instantiation, ending)
pair dcahip_gemm_p3 and dcahip_gemm_h2 can launch, and stays complete when the plan changes: no GPU needed.  The host-side
query dcahip_gemm_planes_plan is the one function both products take their kernel, tiles, K split, tail and workspace from,
so what it answers is what a launch would run.  The numpy restatements of the split kernels meet the project's bounds."""
import ctypes
import itertools

import numpy as np
import pytest

import _plane_gemm_cases as PC

EINVAL = -22
INT_MAX = 2 ** 31 - 1
LAYS = ('NN', 'NT', 'TN', 'TT')
NONE, REDUCE, TAIL = 'none', 'splitk_reduce<1>', 'tail_sum'

# A pair is ((kernel, template arguments), ending).  From the dispatch of dcahip_gemm.hip:
#   gemm_p3_kernel<A_KC, B_KC>          four layouts; no column-sum parameter (a run-time flag)
#   gemm_p3w_kernel<A_KC, B_KC, CS>     NN and TN with and without CS, NT, TT
#   gemm_h2w_kernel<A_KC, B_KC, CS>     NN with CS only, NT, TN with and without CS, TT
#   gemm_h2m_kernel<false>              NN without column sums
# A_KC = !ta, B_KC = tb.


def inst(kernel, lay, cs=None):
    ta, tb = PC.LAYOUTS[lay]
    args = (not ta, bool(tb)) + (() if cs is None else (cs,))
    return (kernel, args)


WIDE = ([inst('gemm_p3w_kernel', l, False) for l in LAYS] + [inst('gemm_p3w_kernel', l, True) for l in ('NN', 'TN')]
        + [inst('gemm_h2w_kernel', l, False) for l in ('NT', 'TN', 'TT')] + [inst('gemm_h2w_kernel', l, True) for l in ('NN', 'TN')])
H2M = ('gemm_h2m_kernel', (False,))
# every instantiation without an ending launch and with the ordered split-K reduce: the table reaches exactly these
REACHABLE = {(i, e) for i in [inst('gemm_p3_kernel', l) for l in LAYS] + WIDE + [H2M] for e in (NONE, REDUCE)}
# every eight-wave instantiation can take the tail.  The tail branch of gemm_wide_body (the slice's K range on the way in, the
# tile-local store on the way out) does not depend on A_KC, B_KC or CS, and a tail case is 70 MB of output: the table holds
# one per piece count, the sweep below finds all eleven
REACHABLE_TAIL = {(i, TAIL) for i in WIDE}
UNREACHABLE = {
    'tail_plan answers for the 256 x 256 tiles only': {(inst('gemm_p3_kernel', l), TAIL) for l in LAYS},
    'the four-wave kernel never takes the tail (planes_plan drops it)': {(H2M, TAIL)},
    'two pieces, NN without column sums: gemm_h2m_kernel takes these': {(inst('gemm_h2w_kernel', 'NN', False), e) for e in (NONE, REDUCE, TAIL)},
    'B k-contiguous stays on the eight-wave kernel (measured slower on four)': {(('gemm_h2m_kernel', (True,)), e) for e in (NONE, REDUCE, TAIL)},
    'colsum_row && tb is DCAHIP_EINVAL': {(inst(k, l, True), e) for k in ('gemm_p3w_kernel', 'gemm_h2w_kernel') for l in ('NT', 'TT')
                                           for e in (NONE, REDUCE, TAIL)},
}
# (a tail never holds tile row 0 under column sums -- tail_plan refuses -- so no tail tile ever owes a column sum: that is a
# property of every CS pair above, not a pair of its own)


@pytest.fixture(scope='module')
def lib():
    from dca_amd import build, hip
    L = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ('dcahip_gemm_planes_plan', 'dcahip_gemm_p3_workspace_bytes', 'dcahip_gemm_h2_workspace_bytes',
                 'dcahip_gemm_h2_supported'):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = hip._SIGNATURES[name]
    return L


def plan(L, pieces, ta, tb, M, N, K, gather, colsum, split):
    out = (ctypes.c_int * 12)()
    rc = L.dcahip_gemm_planes_plan(pieces, ta, tb, M, N, K, gather, colsum, split, ctypes.addressof(out))
    return rc, tuple(out)


def case_plan(L, case):
    pieces, ta, tb, M, N, K, split, flags = case
    rc, out = plan(L, pieces, ta, tb, M, N, K, int('p' in flags or 'u' in flags), int('c' in flags), split)
    assert rc == 0, PC.case_id(case)
    return out


def pair(pieces, ta, tb, out):
    kernel, ending = out[0], (REDUCE if out[5] > 1 else TAIL if out[8] > 1 else NONE)
    if kernel == 0:
        assert pieces == 3
        return (('gemm_p3_kernel', (not ta, bool(tb))), ending)
    if kernel == 2:
        assert pieces == 2 and not ta and not tb and not out[10]
        return (H2M, ending)
    assert kernel == 1
    return (('gemm_p3w_kernel' if pieces == 3 else 'gemm_h2w_kernel', (not ta, bool(tb), bool(out[10]))), ending)


def table_reach(L):
    reach = {}
    for case in PC.CASES:
        reach.setdefault(pair(case[0], case[1], case[2], case_plan(L, case)), PC.case_id(case))
    return reach


def test_table_is_well_formed(lib):
    assert len(set(PC.CASES)) == len(PC.CASES)
    assert 70 <= len(PC.CASES) <= 100
    for case in PC.CASES:
        pieces, ta, tb, M, N, K, split, flags = case
        assert pieces in (2, 3) and (ta, tb) in PC.LAYOUTS.values() and set(flags) <= set('bcpuls') and split >= 0, case
        assert not ('c' in flags and tb) and not ('p' in flags and 'u' in flags), case
        assert not (pieces == 2 and set(flags) & set('pu')), case
        assert not ('s' in flags and ('b' in flags or (pieces == 3 and 'c' in flags))), case
        assert K % 8 == 0 or (ta and not tb), case
        assert pieces == 3 or lib.dcahip_gemm_h2_supported(M, N, K), case
        assert 0 < PC.data_depth(case) <= K
        # operands and outputs stay near 1M elements; the tail cases (257 tiles and more of 256 x 256) are the exception
        if case[:6] in PC.TAIL_CASES:
            assert M * N < 17 * 2 ** 20 + 2 ** 10 and K == 128, case
        else:
            assert max(M * N, M * K, N * K) < 1.2 * 2 ** 20, case
    assert {c[:6] for c in PC.CASES} >= set(PC.TAIL_CASES)


def test_table_reaches_every_reachable_pair(lib):
    assert len(REACHABLE) == 32 and len(REACHABLE_TAIL) == 11
    listed = set().union(*UNREACHABLE.values())
    assert not listed & (REACHABLE | REACHABLE_TAIL)
    reach = table_reach(lib)
    got = set(reach)
    assert got - REACHABLE_TAIL == REACHABLE, (sorted(REACHABLE - got), sorted(got - REACHABLE - REACHABLE_TAIL))
    tails = got & REACHABLE_TAIL
    assert {k[0][0] for k in tails} == {'gemm_p3w_kernel', 'gemm_h2w_kernel'}, tails
    assert any(k[0][1][2] for k in tails), 'a tail under column sums'
    # a forced split larger than the number of K chunks is cut down; a forced split whose last slab is one 16-k step
    forced = [(c, case_plan(lib, c)) for c in PC.CASES if c[6] > 0]
    assert any(1 < out[5] < c[6] for c, out in forced), forced
    for kernel in (('gemm_p3w_kernel',), ('gemm_h2w_kernel',), ('gemm_h2m_kernel',)):
        assert any(pair(c[0], c[1], c[2], out)[0][0] == kernel[0] and out[5] == 2 and c[5] - out[6] == 16 for c, out in forced), kernel


def test_both_sides_of_every_boundary_of_the_plan(lib):
    kern = {}
    for c in PC.CASES:
        kern[c[:6] + ('g' if set(c[7]) & set('pu') else '',)] = case_plan(lib, c)
    k = lambda *key: kern[key][0]
    # M or N = 255 / 256, M N = 2^18 - / +, K % 16, gather on / off at a wide shape
    assert k(3, 0, 1, 255, 1100, 64, '') == 0 and k(3, 1, 0, 1100, 255, 64, '') == 0 and k(3, 0, 1, 256, 1023, 64, '') == 0
    assert k(3, 0, 1, 256, 1024, 80, '') == 1 and k(3, 0, 1, 1024, 256, 16, '') == 1
    assert 256 * 1023 < 2 ** 18 <= 256 * 1024
    assert k(3, 0, 0, 256, 1024, 40, '') == 0 and k(3, 0, 0, 256, 1024, 16, '') == 1
    assert k(3, 0, 0, 300, 900, 64, 'g') == 0 and k(3, 0, 1, 300, 900, 64, 'g') == 0 and k(3, 0, 0, 300, 900, 64, '') == 1
    # 256 / 257 tiles
    full, tail = kern[(3, 0, 1, 256, 65536, 128, '')], kern[(3, 0, 1, 256, 65537, 128, '')]
    assert full[3] * full[4] == 256 and full[8] == 1 and full[11] == 0
    assert tail[3] * tail[4] == 257 and tail[7:10] == (256, 2, 64) and tail[11] == 2 * 256 * 256 * 4
    cs = kern[(2, 1, 0, 300, 33000, 128, '')]
    assert cs[3:5] == (2, 129) and cs[7:10] == (256, 2, 64) and cs[10] == 1 and cs[7] // cs[4] > 0
    # The rest of the tail rule, from the plan alone (a case there is more than 50 MB of output).  A partial round of `rem`
    # tiles is cut into 256 / rem K slices, which is fewer than two from rem = 129 on: tail_plan's own limit `rem > 200` decides
    # nothing (rem = 200 and 201 both answer no tail).  With column sums a tail that would begin in tile row 0 is refused.
    def slices(M, N, K=128, colsum=0):
        rc, out = plan(lib, 3, 1, 0, M, N, K, 0, colsum, 0)
        assert rc == 0 and out[0] == 1 and out[3] * out[4] == -(-M // 256) * -(-N // 256)
        return out[3] * out[4] % 256, out[8]
    assert slices(257, 191 * 256 + 1) == (128, 2) and slices(1025, 76 * 256 + 1) == (129, 1)
    assert slices(257, 227 * 256 + 1) == (200, 1) and slices(256, 456 * 256 + 1) == (201, 1)
    assert slices(256, 65537, colsum=1) == (1, 1) and slices(300, 33000, colsum=1) == (2, 2)
    assert slices(256, 65537, K=64) == (1, 1) and slices(256, 65537, K=512) == (1, 8)       # at least four steps per slice, at most 8


def test_scale_invariance_bases_cover_every_kernel_and_layout(lib):
    got = {}
    for case in PC.CASES:
        if 's' in case[7]:
            out = case_plan(lib, case)
            key = (case[0], out[0], PC.layout_name(case))
            assert key not in got, ('two bases for one kernel and layout', PC.case_id(case), got[key])
            got[key] = PC.case_id(case)
    want = {(3, k, l) for k in (0, 1) for l in LAYS} | {(2, 1, l) for l in LAYS} | {(2, 2, 'NN')}
    assert set(got) == want, (want - set(got), set(got) - want)


def test_table_covers_bias_column_sums_and_gathers(lib):
    seen = set()
    for case in PC.CASES:
        out = case_plan(lib, case)
        p = pair(case[0], case[1], case[2], out)
        lay, flags = PC.layout_name(case), case[7]
        if 'b' in flags:
            seen.add(('bias', case[0], p[1]))
        if 'c' in flags:
            seen.add(('colsum', case[0], lay, out[5] > 1))
        for g in 'pu':
            if g in flags:
                assert out[0] == 0
                seen.add((g, lay))
    want = ({('bias', pc, e) for pc in (2, 3) for e in (NONE, REDUCE, TAIL)}
            | {('colsum', pc, l, s) for pc in (2, 3) for l in ('NN', 'TN') for s in (False, True)}
            | {(g, l) for g in 'pu' for l in LAYS})
    assert want <= seen, want - seen


def expect_ok(L, pieces, ta, tb, M, N, K, gather, colsum):
    if colsum and tb:
        return False
    if (not ta or tb) and K % 8:
        return False
    if pieces == 2:
        wide = M >= 256 and N >= 256 and M * N >= 2 ** 18 and K % 16 == 0
        assert bool(L.dcahip_gemm_h2_supported(M, N, K)) == wide
        return wide and not gather
    return True


def test_sweep_finds_nothing_outside_the_table_and_the_workspace_follows_the_plan(lib):
    reach = set(table_reach(lib))
    sizes = (1, 33, 128, 255, 256, 257, 513, 1030, 8300, 33000)
    found = {}
    for M, N, K, (lay, (ta, tb)), pieces, gather, colsum, split in itertools.product(
            sizes, sizes, (8, 16, 40, 48, 272, 4112), PC.LAYOUTS.items(), (2, 3), (0, 1), (0, 1), (0, 3)):
        rc, out = plan(lib, pieces, ta, tb, M, N, K, gather, colsum, split)
        at = (pieces, lay, M, N, K, gather, colsum, split)
        if not expect_ok(lib, pieces, ta, tb, M, N, K, gather, colsum):
            assert rc == EINVAL, at
            continue
        assert rc == 0, at
        found.setdefault(pair(pieces, ta, tb, out), at)
        kernel, bm, bn, mt, nt, S, kslab, tfirst, tsplit, tkslab, cs, ws = out
        assert (bm, bn) == {0: (128, 128), 1: (256, 256), 2: (128, 256)}[kernel], at
        assert mt == -(-M // bm) and nt == -(-N // bn) and kslab % 32 == 0, at
        assert S >= 1 and (S - 1) * kslab < K <= S * kslab, at                              # no empty K split
        assert cs == int(kernel == 1 and bool(colsum)), at
        if tsplit > 1:
            assert kernel == 1 and S == 1 and tkslab % 16 == 0 and (tsplit - 1) * tkslab < K <= tsplit * tkslab, at
            assert 0 < tfirst == mt * nt - mt * nt % 256 and (not colsum or tfirst // nt > 0), at
            want = (mt * nt - tfirst) * tsplit * 256 * 256 * 4
        else:
            want = S * (M + colsum) * N * 4 if S > 1 else 0
            # (the four-wave kernel asks for what the eight-wave plan of its shape asks, a tail's bytes included)
            if kernel == 2 and S == 1:
                want = plan(lib, 2, 1, 0, M, N, K, 0, 0, split)[1][11]
        assert ws == min(want, INT_MAX), at
        if pieces == 3:
            assert min(lib.dcahip_gemm_p3_workspace_bytes(M, N, K, colsum, split), INT_MAX) >= ws, at
        else:
            assert min(lib.dcahip_gemm_h2_workspace_bytes(M, N, K, colsum, split), INT_MAX) == ws, at
    new = {p: at for p, at in found.items() if p not in reach and p not in REACHABLE_TAIL}
    assert not new, ('reached by the plane products, by no case of tests/_plane_gemm_cases.py', new)
    assert set(found) == REACHABLE | REACHABLE_TAIL, (REACHABLE | REACHABLE_TAIL) ^ set(found)


def test_plan_query_rejects_what_the_products_reject(lib):
    ok = dict(pieces=3, ta=0, tb=0, M=8, N=8, K=8, gather=0, colsum=0, split=0)
    assert plan(lib, **ok)[0] == 0
    for bad in (dict(M=0), dict(N=-1), dict(K=0), dict(pieces=1), dict(pieces=4), dict(tb=1, colsum=1), dict(K=12),
                dict(ta=1, tb=1, K=12), dict(pieces=2), dict(pieces=2, M=512, N=512, K=24),
                dict(pieces=2, M=512, N=512, K=32, gather=1), dict(pieces=2, M=255, N=2048, K=32)):
        assert plan(lib, **dict(ok, **bad))[0] == EINVAL, bad
    assert plan(lib, **dict(ok, ta=1, K=12))[0] == 0            # TN: no operand is contiguous along k
    assert plan(lib, **dict(ok, pieces=2, M=512, N=512, K=32))[0] == 0
    assert lib.dcahip_gemm_planes_plan(3, 0, 0, 8, 8, 8, 0, 0, 0, None) == EINVAL


def test_restatements_of_the_splits_meet_the_bounds_of_the_project():
    """h2_split: max(2^-22 |x 2^e|, 2^-25) (dca_amd/csrc/h2_math.hpp); p3_split: 2^-23 |x| (as
    tests/test_gemm_p3_gpu.py::test_split_planes_reconstructs_fp32), on the inputs tests/test_plane_split_gpu.py uses."""
    rng = np.random.RandomState(0)
    x = PC.split_inputs(rng, (301, 77), 2)
    e = PC.block_exp(np.abs(x).max())
    assert 2.0 ** 13 <= np.abs(x).max() * 2.0 ** e < 2.0 ** 14
    h1, h2 = PC.h2_split(x, e)
    xs = np.ldexp(x.astype(np.float64), e)
    err = np.abs(h1.astype(np.float64) + h2.astype(np.float64) - xs)
    assert (err <= np.maximum(2.0 ** -22 * np.abs(xs), 2.0 ** -25)).all()
    assert (np.abs(h2[h2 != 0]).min() < 2.0 ** -14) and (h2 == 0).any()          # denormal second pieces, and vanished ones
    for m, want in ((0.0, 0), (np.inf, 0), (np.nan, 0), (1.0, 13), (1.99, 13), (2.0, 12), (2.0 ** -47, 60), (2.0 ** -48, 60),
                    (2.0 ** -140, 60), (2.0 ** 73, -60), (2.0 ** 74, -60), (2.0 ** 100, -60), (2.0 ** -46, 59)):
        assert PC.block_exp(m) == want, (m, PC.block_exp(m))
    # down to a largest magnitude of 2^-140 the pieces keep the bound (the absolute floor carries it below 2^-47)
    for top in (-46, -60, -100, -140):
        y = np.ldexp(rng.uniform(-1, 1, 4096), top).astype(np.float32)
        y[0] = np.ldexp(np.float32(1), top)
        ey = PC.block_exp(np.abs(y).max())
        g1, g2 = PC.h2_split(y, ey)
        ys = np.ldexp(y.astype(np.float64), ey)
        assert (np.abs(g1.astype(np.float64) + g2.astype(np.float64) - ys) <= np.maximum(2.0 ** -22 * np.abs(ys), 2.0 ** -25)).all(), top
    # at 2^100 the clamp at -60 leaves 2^40: the pieces overflow
    with np.errstate(all='ignore'):
        assert not np.isfinite(PC.h2_split(np.float32(2.0 ** 100), PC.block_exp(2.0 ** 100))[0])

    x3 = PC.split_inputs(rng, (301, 77), 3)
    p = PC.p3_split(x3)
    s = sum(PC.bf16_to_f32(h).astype(np.float64) for h in p)
    assert (np.abs(s - x3.astype(np.float64)) <= 2.0 ** -23 * np.abs(x3)).all()
    assert (p[0][x3 == 0] & 0x7FFF == 0).all()
    # round to nearest EVEN on the upper 16 bits: 1 + 2^-8 is a tie (down), 1 + 2^-8 + 2^-9 is above it, 1 + 2^-7 + 2^-8 a tie (up)
    hand = np.array([1.0, 1.00390625, 1.005859375, 1.01171875, 2.0 ** -100], np.float32)
    assert [hex(v) for v in PC.bf16_rne(hand)] == ['0x3f80', '0x3f80', '0x3f81', '0x3f82', '0xd80']
