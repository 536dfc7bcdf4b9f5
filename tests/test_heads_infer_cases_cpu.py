"""The host half of the inference heads kernel's edge tests (tests/_heads_infer_cases.py, run on the device by
tests/test_heads_infer_gpu.py): the case table reaches every path it was written for, and the fp64 oracle is the reference the
device tests take it for -- exact at the clips, NaN for NaN, and met by its own fp32 evaluation within the device tests'
tolerance."""
import numpy as np

import _heads_infer_cases as C
from oracle import zinb_np as Z


def _paths():
    return {c.name: C.expected_path(c) for c in C.LAYOUT_CASES}


def test_every_case_takes_the_path_it_claims():
    for c in C.LAYOUT_CASES:
        p = C.expected_path(c)
        assert (p.V, p.nseg, p.items, p.triggers) == c.claim, (c.name, p)
        assert c.heads_in == c.heads_out and c.heads_out
        assert c.name[:2] == 'v%d' % p.V and '_%dx%d' % (c.B, c.G) in c.name
        if c.in_place:
            assert (c.ldo, c.ooffs, c.out_shift) == (c.lda, c.offs, 0)


def test_every_path_is_reached():
    P = _paths()

    def reached(V, nseg=None, stride=False, **kw):
        return [n for n, p in P.items() if p.V == V and p.stride == stride and (nseg is None or (p.nseg > 1) == (nseg > 1))
                and all(getattr(C.BY_NAME[n], k) == v for k, v in kw.items())]
    shapes = lambda names: {(C.BY_NAME[n].B, C.BY_NAME[n].G) for n in names}                # noqa: E731
    # V = 4: one segment (the four shapes, in and out of place with lda != ldo), several segments, grid-stride
    one = reached(4, 1)
    assert {(1, 1), (7, 50), (33, 1024)} <= shapes(one)
    assert any(c.lda == 156 and c.ldo == 160 and not c.in_place for c in map(C.BY_NAME.get, one))
    assert any(c.in_place and (c.B, c.G) == (7, 50) and c.heads_out == C.HEADS for c in map(C.BY_NAME.get, one))
    several = reached(4, 2)
    assert {(5, 1028), (3, 2052), (9, 3076)} <= shapes(several)
    assert all(P[n].last == 1 for n in several if C.BY_NAME[n].G % 4 == 0)              # the last segment holds one quad
    assert any(C.BY_NAME[n].G % 4 and P[n].last > 1 for n in several)                  # ... and a ragged quad in a later segment
    assert {P[n].nseg for n in several} >= {2, 3, 4}
    stride4 = reached(4, stride=True)
    assert {(4100, 8), (1400, 3076)} <= shapes(stride4) and P['v4_1400x3076'].items == 5600 and P['v4_4100x8'].nseg == 1
    # V = 1: each trigger alone, several segments, grid-stride
    alone = {P[n].triggers for n in reached(1, 1)}
    assert {('lda',), ('ldo',), ('in_ptr',), ('out_ptr',)} <= alone
    sev1 = reached(1, 2)
    assert {(4, 257), (3, 515)} <= shapes(sev1) and {P['v1_4x257'].last, P['v1_3x515'].last} == {1, 3}
    stride1 = reached(1, stride=True)
    assert (130, 8193) in shapes(stride1) and P['v1_130x8193'].items == 4290
    # every subset of the outputs and the linear mean, on both forms
    for V, B, G in ((4, 7, 50), (1, 9, 37)):
        subsets = {C.BY_NAME[n].heads_out for n in reached(V, 1, B=B, G=G, flags=0, in_place=True)}
        assert subsets >= set(C.SUBSETS) and len(C.SUBSETS) == 7
        assert reached(V, 1, flags=C.MSE)
    # the pairs compared bit for bit hold the same values and differ in what they are compared over
    for a, b in C.SAME_BITS_IN_OUT:
        ca, cb = C.BY_NAME[a], C.BY_NAME[b]
        assert (ca.B, ca.G, ca.flags) == (cb.B, cb.G, cb.flags) and ca.in_place and not cb.in_place and P[a].V == P[b].V
    for a, b in C.SAME_BITS_V1_V4:
        ca, cb = C.BY_NAME[a], C.BY_NAME[b]
        assert (ca.B, ca.G, ca.flags) == (cb.B, cb.G, cb.flags) and (P[a].V, P[b].V) == (1, 4)
    assert {P[n].V for n in C.NAN_CASES} == {1, 4}


def test_the_predicates_follow_the_host_code():
    """expected_path against the lines of dcahip_zinb_heads_infer it restates, on layouts around every condition."""
    mk = lambda **kw: C.Case('x', 3, 37, 120, 120, (0, 40, 80), (0, 40, 80), 0, False, C.HEADS, C.HEADS, 0, None)._replace(**kw)  # noqa: E731
    assert C.expected_path(mk()).V == 4
    assert C.expected_path(mk(lda=122)).V == 1 and C.expected_path(mk(ldo=123)).V == 1
    assert C.expected_path(mk(G=5, lda=4, offs=(0, 0, 0), heads_in=('mean',), heads_out=('mean',))).triggers == ('ld<Gp',)
    assert C.expected_path(mk(offs=(0, 41, 80))).triggers == ('in_ptr',)
    assert C.expected_path(mk(offs=(0, 41, 80), heads_in=('mean', 'pi'), heads_out=('mean', 'pi'))).V == 4     # NULL: not looked at
    assert C.expected_path(mk(out_shift=2)).triggers == ('out_ptr',) and C.expected_path(mk(out_shift=4)).V == 4
    p = C.expected_path(mk(B=17, G=1025, lda=3 * 1028, ldo=3 * 1028))
    assert (p.V, p.nseg, p.items, p.last, p.stride) == (4, 2, 34, 1, False)
    assert C.expected_path(mk(B=17, G=1025, lda=3 * 1028)).triggers == ('ld<Gp',)          # ldo = 120 < Gp
    p = C.expected_path(mk(B=17, G=1025, lda=3 * 1028 + 1, ldo=3 * 1028))
    assert (p.V, p.nseg, p.items, p.last) == (1, 5, 85, 1)
    assert not C.expected_path(mk(B=4096, G=8)).stride and C.expected_path(mk(B=4097, G=8)).stride


def test_value_cases_are_planted_and_fp32():
    v = C.value_cases()
    assert len(v['mean']) == 5 * len(C.MEAN_VALUES) and len(v['disp']) == 5 * len(C.DISP_VALUES) and len(v['pi']) == 5 * len(C.PI_VALUES)
    for h, a in v.items():
        np.testing.assert_array_equal(a, a.astype(np.float32).astype(np.float64))
        x = a.reshape(-1, 5)
        with np.errstate(invalid='ignore'):
            assert ((np.diff(x, axis=1) > 0) | np.isinf(x[:, 1:])).all(), h       # two distinct fp32 steps to either side
        for B, G in ((7, 50), (9, 37)):
            np.testing.assert_array_equal(C.inputs(B, G)[h].reshape(-1)[:len(a)], a)
    assert 0 < v['mean'][5 * C.MEAN_VALUES.index(1e-40) + 2] < 1.2e-38                 # a denormal, not flushed on the way
    minus0 = [i for i, x in enumerate(C.PI_VALUES) if x == 0 and np.signbit(x)]
    assert len(minus0) == 1 and np.signbit(v['pi'][5 * minus0[0] + 2]) and v['pi'][5 * minus0[0] + 1] < 0 < v['pi'][5 * minus0[0] + 3]
    d = C.inputs(1, 1)                                                             # a shape that holds one value of each
    assert d['mean'].shape == (1, 1) and d['mean'][0, 0] == v['mean'][0]


def test_oracle_at_and_beyond_the_clips():
    d, r = C.inputs(7, 50), C.reference(7, 50)
    sf = d['sf'][:, None] * np.ones((1, 50))
    lo32, hi32 = np.float64(np.float32(np.log(1e-5))), np.float64(np.float32(np.log(1e6)))
    am, mu = d['mean'], r['mean']
    step = lambda x: float(np.spacing(np.float32(abs(x))))                          # noqa: E731
    # one fp32 step outside the window and anything beyond: the clip constant times sf, exactly
    below, above = am <= lo32 - step(lo32), am >= hi32 + step(hi32)
    assert below.sum() >= 10 and above.sum() >= 12
    np.testing.assert_array_equal(mu[below], (Z.MEAN_MIN * sf)[below])
    np.testing.assert_array_equal(mu[above], (Z.MEAN_MAX * sf)[above])
    # the five values around each clip straddle it: exp() of the outer ones is clipped, of the inner ones is not
    for x0, const in ((lo32, Z.MEAN_MIN), (hi32, Z.MEAN_MAX)):
        i = np.flatnonzero(am.reshape(-1)[:60] == x0)[0]
        five = mu.reshape(-1)[i - 2:i + 3] / sf.reshape(-1)[i - 2:i + 3]
        assert (five == const).any() and (five != const).any() and (np.abs(five / const - 1) < 4e-6).all()
    ad, th = d['disp'], r['disp']
    low, high = ad <= np.float64(np.float32(-9.2103)) + 2 * step(9.2103), ad >= 1e4
    assert low.sum() >= 25 and high.sum() >= 12
    assert (th[low] == Z.DISP_MIN).all() and (th[high] == Z.DISP_MAX).all()
    inside = (ad >= np.float64(np.float32(-9.21))) & (ad < 9999.9995)
    assert (th[inside] > Z.DISP_MIN).all() and (th[inside] < Z.DISP_MAX).all()
    assert th.reshape(-1)[5 * C.DISP_VALUES.index(9999.999) + 2] < Z.DISP_MAX
    ap, pi = d['pi'], r['pi']
    assert (pi[ap == -np.inf] == 0).all() and (pi[ap == np.inf] == 1).all() and (ap == -np.inf).sum() >= 3 <= (ap == np.inf).sum()
    assert (pi[ap == 0] == 0.5).all() and ((pi >= 0) & (pi <= 1)).all()
    assert 0 < pi.reshape(-1)[5 * C.PI_VALUES.index(-104.0) + 2] < C.ATOL            # what the absolute term is there for
    assert all(np.isfinite(x).all() for x in r.values())


def test_oracle_keeps_nan_and_changes_nothing_else():
    for B, G in ((7, 50), (9, 37)):
        clean, nan = C.reference(B, G), C.reference(B, G, nan=True)
        pos = C.nan_positions(B, G)
        assert len(set(pos.values())) == 3 and pos['mean'][1] == G - 1 and G % 4          # the last column of a ragged quad
        n_values = max(len(v) for v in C.value_cases().values())
        for h, (r, c) in pos.items():
            assert r * G + c >= n_values                                               # behind the planted values
            assert np.isnan(C.inputs(B, G, nan=True)[h][r, c])
            m = np.zeros((B, G), bool)
            m[r, c] = True
            assert np.isnan(nan[h][m]).all() and not np.isnan(nan[h][~m]).any()
            np.testing.assert_array_equal(nan[h][~m], clean[h][~m])
        lin = C.reference(B, G, C.MSE, nan=True)['mean']
        assert np.isnan(lin[pos['mean']]) and np.isnan(lin).sum() == 1


def test_fp32_oracle_meets_the_device_tolerance():
    """The bound the device tests hold the kernel to is one the reference formula meets when numpy evaluates it in fp32."""
    for B, G in ((7, 50), (9, 37)):
        for flags in (0, C.MSE):
            for nan in (False, True):
                d = C.inputs(B, G, nan)
                ref, f32 = C.reference(B, G, flags, nan), C.oracle(d, flags, np.float32)
                for h in C.HEADS:
                    assert f32[h].dtype == np.float32
                    if flags & C.MSE and h == 'mean':
                        # one fp32 product: the fp64 product of two fp32 numbers is exact, so its rounding IS the fp32 result
                        # (beyond the fp32 range: infinite), bit for bit -- what the device test asks of the linear mean
                        with np.errstate(over='ignore'):
                            r32 = ref[h].astype(np.float32)
                        np.testing.assert_array_equal(f32[h], r32)                         # (NaN equal to NaN)
                        np.testing.assert_array_equal(np.signbit(f32[h]), np.signbit(r32))
                        continue
                    ok = C.within(f32[h], ref[h])
                    assert ok.all(), (h, flags, nan, np.argwhere(~ok)[:5], f32[h][~ok][:5], ref[h][~ok][:5], C.worst(f32[h], ref[h]))
    assert not C.within(np.float32(1.0 + 4e-6), 1.0) and C.within(0.0, 1e-38) and not C.within(0.0, 2e-38)
    assert not C.within(1.0, np.nan) and not C.within(np.nan, 1.0) and C.within(np.nan, np.nan)
    assert C.within(np.inf, np.inf) and not C.within(3e38, np.inf)
