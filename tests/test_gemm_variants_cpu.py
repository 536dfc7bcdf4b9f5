"""The case table of the dcahip_sgemm variant tests (tests/_gemm_cases.py) reaches every kernel instantiation dcahip_sgemm
can launch, and stays complete when the plan changes: no GPU needed.  The host-side query dcahip_sgemm_plan is the one
function dcahip_sgemm takes its tile, arithmetic and loader width from, so what it answers is what a launch would run."""
import ctypes
import itertools

import pytest

import _gemm_cases as GC

EINVAL = -22
TILES = [(128, 64), (64, 128), (128, 128), (64, 64)]
X3, EXACT = 1, 0

# The ten instantiations of the 48 that the dispatch never launches:
#   the weight gradient (TN) is always exact -- the split kernel's larger LDS images cost it more than the matrix phase
#   returns (dcahip_gemm.hip, sgemm_plan) -- on every tile and loader width: 8
#   NN on the 128 x 64 tile means N <= 64, and NN runs on three bf16 pieces from 128 columns up only: 2
UNREACHABLE = ({(t, 'TN', v, X3) for t in TILES for v in (4, 1)}
               | {((128, 64), 'NN', v, X3) for v in (4, 1)})
REACHABLE = {(t, l, v, a) for t in TILES for l in GC.LAYOUTS for v in (4, 1) for a in (EXACT, X3)} - UNREACHABLE


@pytest.fixture(scope='module')
def lib():
    from dca_amd import build, hip
    L = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ('dcahip_sgemm_plan', 'dcahip_sgemm_workspace_bytes'):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = hip._SIGNATURES[name]
    return L


def plan(L, ta, tb, M, N, K, colsum, split, a_addr, lda, b_addr, ldb):
    out = (ctypes.c_int * 8)()
    rc = L.dcahip_sgemm_plan(ta, tb, M, N, K, colsum, split, a_addr, lda, b_addr, ldb, ctypes.addressof(out))
    return rc, tuple(out)


def reduce_class(split, outputs):
    """The ending: no reduce, 16 lanes per output, one lane per output below / from 16 splits (include/dcahip.h)."""
    from dca_amd.ops import HipOps
    lanes = HipOps.sgemm_reduce_lanes(split, outputs)
    return 'none' if lanes == 0 else 'reduce<16>' if lanes == 16 else 'reduce<1>, split >= 16' if split >= 16 else 'reduce<1>'


def case_plan(L, case):
    ta, tb, M, N, K, split, align, flags = case
    lda, ldb, _ = GC.leading_dims(case)
    oa, ob = GC.offsets(case)
    rc, out = plan(L, ta, tb, M, N, K, int('c' in flags), split, 0x10000 + 4 * oa, lda, 0x20000 + 4 * ob, ldb)
    assert rc == 0, GC.case_id(case)
    return out


def variant(layout, out):
    return ((out[0], out[1]), layout, out[7], out[6])


def layout_name(case):
    return 'TN' if case[0] else 'NT' if case[1] else 'NN'


def table_reach(L):
    variants, endings = {}, {}
    for case in GC.CASES:
        out = case_plan(L, case)
        outputs = (case[2] + ('c' in case[7])) * case[3]
        variants.setdefault(variant(layout_name(case), out), GC.case_id(case))
        endings.setdefault(reduce_class(out[4], outputs), GC.case_id(case))
    return variants, endings


def test_table_is_well_formed():
    assert len(set(GC.CASES)) == len(GC.CASES)
    assert 70 <= len(GC.CASES) <= 90
    for case in GC.CASES:
        ta, tb, M, N, K, split, align, flags = case
        assert (ta, tb) in GC.LAYOUTS.values() and align in GC.ALIGNS and set(flags) <= set('bcpuls'), case
        assert not ('c' in flags and tb) and not ('p' in flags and 'u' in flags), case
        assert not ('s' in flags and set(flags) & set('bc')), case
        assert K < 3000                                   # the exact kernels' chain bound is applied up to there
        # operands stay near 1M floats; the one larger is A of 2049 x 33 x 2100 (16 or more splits of more than 65536 outputs)
        assert max(M * N, M * K, N * K) < (4.2 if (M, K) == (2049, 2100) else 1.2) * 2 ** 20, case
    # each reason for scalar loads on each layout
    seen = {(layout_name(c), c[6]) for c in GC.CASES}
    assert seen == set(itertools.product(GC.LAYOUTS, GC.ALIGNS)), set(itertools.product(GC.LAYOUTS, GC.ALIGNS)) - seen


def test_table_reaches_every_reachable_variant(lib):
    assert len(REACHABLE) == 38
    variants, endings = table_reach(lib)
    assert set(variants) == REACHABLE, (sorted(REACHABLE - set(variants)), sorted(set(variants) - REACHABLE))
    assert set(endings) == {'none', 'reduce<1>', 'reduce<16>', 'reduce<1>, split >= 16'}, endings
    # a forced split larger than the number of K chunks: the empty trailing splits are dropped
    forced = [(c, case_plan(lib, c)) for c in GC.CASES if c[5] > (c[4] + 31) // 32]
    assert any(out[4] == 1 for _, out in forced) and any(1 < out[4] < c[5] for c, out in forced), forced
    # both sides of every boundary of the plan
    tiles = {(c[2], c[3]): case_plan(lib, c)[:2] for c in GC.CASES}
    for (M, N), tile in {(64, 65): (64, 128), (65, 130): (64, 64), (130, 64): (128, 64), (130, 65): (64, 64),
                         (2047, 64): (128, 64), (2048, 64): (64, 64), (2048, 512): (64, 64), (2049, 512): (128, 128)}.items():
        assert tiles[(M, N)] == tile, (M, N, tiles[(M, N)])
    arith = {(c[2], c[3]): case_plan(lib, c)[6] for c in GC.CASES if (c[0], c[1]) == GC.NN and c[5] >= 0}
    assert arith[(8300, 127)] == EXACT and arith[(8300, 128)] == X3


def test_scale_invariance_bases_cover_every_tile_layout_and_arithmetic(lib):
    want = {(t, l, a) for (t, l, v, a) in REACHABLE}
    got = {}
    for case in GC.CASES:
        if 's' in case[7]:
            out = case_plan(lib, case)
            key = ((out[0], out[1]), layout_name(case), out[6])
            assert key not in got, ('two bases for one kernel', GC.case_id(case), got[key])
            got[key] = GC.case_id(case)
    assert set(got) == want, (want - set(got), set(got) - want)


def test_table_covers_bias_column_sums_and_gathers(lib):
    """Bias in the kernel and in the reduce on both arithmetics; column sums on NN and TN with and without split (NN: both
    arithmetics) and with scalar loads; the three gathers."""
    seen = set()
    for case in GC.CASES:
        out = case_plan(lib, case)
        lay, split, flags = layout_name(case), out[4] > 1, case[7]
        if 'b' in flags:
            seen.add(('bias', split, out[6]))
        if 'c' in flags:
            seen.add(('colsum', lay, split, out[6]))
            if out[7] == 1:
                seen.add(('colsum', 'V1'))
        for g in 'pu':
            if g in flags:
                seen.add((g, lay))
    want = ({('bias', s, a) for s in (False, True) for a in (EXACT, X3)}
            | {('colsum', 'NN', s, a) for s in (False, True) for a in (EXACT, X3)}
            | {('colsum', 'TN', s, EXACT) for s in (False, True)} | {('colsum', 'V1')}
            | {('p', 'NN'), ('p', 'NT'), ('p', 'TN'), ('u', 'NN'), ('u', 'TN')})
    assert want <= seen, want - seen


def test_sweep_finds_no_variant_outside_the_table(lib):
    variants, endings = table_reach(lib)
    sizes = (1, 33, 64, 65, 127, 128, 300, 1030, 2047, 2048, 2049, 8300)
    addrs = ((0x10000, 0x20000, 0, 0), (0x10004, 0x20000, 0, 0), (0x10000, 0x20004, 0, 0),
             (0x10000, 0x20000, 1, 0), (0x10000, 0x20000, 0, 1))
    found_v, found_e = {}, {}
    for M, N, K, (lay, (ta, tb)), split in itertools.product(sizes, sizes, (3, 40, 2100), GC.LAYOUTS.items(), (-1, 0, 3)):
        ca, cb = (M if ta else K), (K if tb else N)
        for a_addr, b_addr, da, db in addrs:
            rc, out = plan(lib, ta, tb, M, N, K, 0, split, a_addr, GC.r4(ca) + da, b_addr, GC.r4(cb) + db)
            assert rc == 0
            found_v.setdefault(variant(lay, out), (lay, M, N, K, split))
            for colsum in ((0,) if tb else (0, 1)):
                found_e.setdefault(reduce_class(out[4], (M + colsum) * N), (lay, M, N, K, split))
    new_v = {v: at for v, at in found_v.items() if v not in variants}
    new_e = {e: at for e, at in found_e.items() if e not in endings}
    assert not new_v and not new_e, ('reached by dcahip_sgemm, by no case of tests/_gemm_cases.py', new_v, new_e)
    assert set(found_v) <= REACHABLE


def test_workspace_bytes_follow_the_plan(lib):
    for case in GC.CASES:
        ta, tb, M, N, K, split, align, flags = case
        colsum = int('c' in flags)
        out = case_plan(lib, case)
        assert out[2] == -(-M // out[0]) and out[3] == -(-N // out[1]) and out[5] % 32 == 0
        assert (out[4] - 1) * out[5] < K <= out[4] * out[5], (GC.case_id(case), out)       # no empty split
        want = out[4] * (M + colsum) * N * 4 if out[4] > 1 else 0
        assert lib.dcahip_sgemm_workspace_bytes(ta, tb, M, N, K, colsum, split) == want, GC.case_id(case)


def test_plan_query_rejects_what_sgemm_rejects(lib):
    ok = dict(ta=0, tb=0, M=8, N=8, K=8, colsum=0, split=0, a_addr=0x10000, lda=8, b_addr=0x20000, ldb=8)
    assert plan(lib, **ok)[0] == 0
    for bad in (dict(M=0), dict(N=-1), dict(K=0), dict(a_addr=None), dict(b_addr=None), dict(ta=1, tb=1),
                dict(tb=1, colsum=1)):
        assert plan(lib, **dict(ok, **bad))[0] == EINVAL, bad
    assert lib.dcahip_sgemm_plan(0, 0, 8, 8, 8, 0, 0, 0x10000, 8, 0x20000, 8, None) == EINVAL
