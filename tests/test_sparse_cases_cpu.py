"""What tests/test_sparse_edges_gpu.py judges the byte-store first-layer kernels with (tests/_sparse_cases.py) is itself
checked here, without a GPU: the fp64 references against a per-element loop, edge_counts for every planted class at every
position, decode_lut on entries made by hand, and the restatement of the launch plans for the numbers each named shape is
there for."""
import math

import numpy as np
import pytest

import _sparse_cases as SC


def _problem(n, G, H1, seed, with_mean, with_std, with_fac, do_log):
    rng = np.random.RandomState(seed)
    Y = SC.edge_counts(n, G, seed)
    fac = SC.f32(rng.lognormal(0, 0.4, n)) if with_fac else None
    mean = SC.f32(rng.normal(0.5, 0.3, G)) if with_mean else None
    std = SC.f32(rng.uniform(0.5, 2.0, G)) if with_std else None
    rows = rng.permutation(n)[:max(1, n - 2)]
    W, b = SC.f32(rng.normal(0, 0.1, (G, H1))), SC.f32(rng.normal(0, 0.3, H1))
    dZ = SC.f32(rng.normal(0, 1e-3, (len(rows), H1)))
    return Y, fac, do_log, mean, std, rows, W, b, dZ


@pytest.mark.parametrize('n,G', [(5, 3), (7, 9)])
@pytest.mark.parametrize('with_mean,with_std', [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize('with_fac,do_log', [(True, True), (False, False)])
def test_references_equal_a_per_element_loop(n, G, with_mean, with_std, with_fac, do_log):
    H1 = 4
    Y, fac, do_log, mean, std, rows, W, b, dZ = _problem(n, G, H1, 10 * n + G, with_mean, with_std, with_fac, do_log)
    B = len(rows)

    def L(c, g):
        v = Y[rows[c], g] / (fac[rows[c]] if fac is not None else 1.0)
        return math.log1p(v) if do_log else v
    sd = lambda g: std[g] if std is not None else 1.0
    mu = lambda g: mean[g] if mean is not None else 0.0
    Z, Za = np.zeros((B, H1)), np.zeros((B, H1))
    gW, gWa = np.zeros((G, H1)), np.zeros((G, H1))
    for c in range(B):
        for j in range(H1):
            z, za = b[j], abs(b[j])
            for g in range(G):
                z += (L(c, g) - mu(g)) / sd(g) * W[g, j]
                za += abs(L(c, g) / sd(g)) * abs(W[g, j]) + abs(mu(g) / sd(g)) * abs(W[g, j])
            Z[c, j], Za[c, j] = z, za
    for g in range(G):
        for j in range(H1):
            s = sum(dZ[c, j] for c in range(B))
            sa = sum(abs(dZ[c, j]) for c in range(B))
            gW[g, j] = sum((L(c, g) - mu(g)) / sd(g) * dZ[c, j] for c in range(B))
            gWa[g, j] = sum(abs(L(c, g) / sd(g)) * abs(dZ[c, j]) for c in range(B)) + abs(mu(g) / sd(g)) * (sa + abs(s))
    Zr, Zr_abs = SC.reference_fwd(Y, fac, do_log, mean, std, rows, W, b)
    gWr, col, gWr_abs, bmag = SC.reference_dw(Y, fac, do_log, mean, std, rows, dZ)
    np.testing.assert_allclose(Zr, Z, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(Zr_abs, Za, rtol=1e-12)
    np.testing.assert_allclose(gWr, gW, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gWr_abs, gWa, rtol=1e-12)
    np.testing.assert_allclose(col, dZ.sum(0), rtol=1e-12, atol=1e-18)
    assert bmag == pytest.approx(np.abs(dZ).sum(0).max(), rel=1e-12)
    # no bias: Z and its magnitude lose exactly the bias terms
    Z0, Z0_abs = SC.reference_fwd(Y, fac, do_log, mean, std, rows, W, None)
    np.testing.assert_allclose(Z0, Z - b, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(Z0_abs, Za - np.abs(b), rtol=1e-12)


@pytest.mark.parametrize('nb,G', [(40, 128), (70, 129), (257, 127), (150, 520)])
def test_edge_counts_plants_every_class_at_every_position(nb, G):
    n = nb + 9
    rows = np.random.RandomState(nb).permutation(n)[:nb]
    Y = SC.edge_counts(n, G, 3, rows)
    assert Y.shape == (n, G) and (Y >= 0).all() and (Y == np.floor(Y)).all()
    Yb = Y[rows]
    pos = SC.edge_positions(nb, G)
    assert sorted(pos) == sorted(SC.EDGE_VALUES)
    cells = [c for v in pos.values() for c in v]
    assert len(set(cells)) == len(cells), 'two planted values share a cell'
    for v, (lo0, up0, last_row, lo_g0, up_g0, last_gene) in pos.items():
        for r, g in (lo0, up0, last_row, lo_g0, up_g0, last_gene):
            assert Yb[r, g] == v
        assert lo0[0] == 0 and lo0[1] % 128 < 64 and up0[0] == 0 and up0[1] % 128 >= 64       # both lane halves of the forward
        assert last_row[0] == nb - 1 and last_gene[1] == G - 1
        assert lo_g0[1] == 0 and lo_g0[0] % 16 < 8 and up_g0[1] == 0 and up_g0[0] % 16 >= 8   # ... of the weight gradient
    big, zero = SC.edge_rows(nb, G)
    assert big != zero and (Yb[big] >= 255).all() and (Yb[zero] == 0).all()
    assert len(np.unique(Yb[big])) > G // 2           # a long list of distinct values, not one constant


@pytest.mark.parametrize('nb,G', [(1, 1), (2, 5), (15, 17), (31, 16), (33, 17), (32, 63), (33, 255)])
def test_edge_counts_wraps_inside_a_small_matrix(nb, G):
    for r, g in (c for v in SC.edge_positions(nb, G).values() for c in v):
        assert 0 <= r < nb and 0 <= g < G
    Y = SC.edge_counts(nb + 2, G, 1, np.arange(2, nb + 2))
    assert Y.shape == (nb + 2, G) and (Y >= 0).all() and (Y == np.floor(Y)).all()
    # the last planted position of the last value is never overwritten
    r, g = SC.edge_positions(nb, G)[SC.EDGE_VALUES[-1]][-1]
    assert Y[2 + r, g] == SC.EDGE_VALUES[-1]


def test_decode_lut_on_entries_made_by_hand():
    bf = lambda x: int(np.float32(x).view(np.uint32)) >> 16          # exact for the values below
    p = [(1.0, 2.0 ** -9, 2.0 ** -18), (3.0, -2.0 ** -8, -2.0 ** -17), (0.0, 0.0, 0.0)]
    lut = np.zeros((1, 128, 2), np.int64)
    for k, (a, b, c) in enumerate(p):
        lut[0, k] = (bf(a) | bf(b) << 16, bf(c))
    lut32 = lut.astype(np.uint32).view(np.int32).reshape(1, 128, 2)  # the second entry's first word is negative as int32
    assert lut32[0, 1, 0] < 0
    got = SC.decode_lut(lut32)
    assert got.shape == (1, 128)
    assert [got[0, k] for k in range(3)] == [a + b + c for a, b, c in p]
    bad = lut32.copy(); bad[0, 5, 1] = 1 << 16
    with pytest.raises(AssertionError):
        SC.decode_lut(bad)


def test_plans_of_the_named_forward_shapes():
    for (B, G), want in SC.FWD_SHAPES:
        plan = SC.fl_plan(B, G)
        assert {k: plan[k] for k in want} == want, (B, G, plan)
        assert plan['chunks'] <= 32 and plan['ms_per'] % 2 == 0 and 0 < plan['last_chunk_ms'] <= plan['ms_per']
    shapes = [s for s, _ in SC.FWD_SHAPES]
    assert SC.fl_plan(32, 63)['ldc'] <= 64                       # no stored byte at gene offsets 64 ..: the upper half never loads
    assert SC.fl_plan(256, 65)['ldc'] == 64 + 16                 # of the upper half's four loads only the first is inside the row
    assert len(set(shapes)) == 13


def test_plans_of_the_named_weight_gradient_shapes():
    for (B, G), first, ring in SC.DW_SHAPES:
        for H1 in (32, 64, 128):
            plan = SC.dw_plan(B, G, H1, 1)
            assert not plan['ring'] and {k: plan[k] for k in first} == first, (B, G, H1, plan)
            assert plan['rows_per_split'] <= 2048 and plan['rows_per_split'] % 64 == 0
        plan = SC.dw_plan(B, G, 64, 2)
        assert plan['ring'] and {k: plan[k] for k in ring} == ring, (B, G, plan)
        assert plan['rows_per_split'] <= 1024 and plan['rows_per_split'] % 16 == 0
        # by the shape (form 0): the ring form for 64 units from 1024 rows, the first form otherwise
        assert SC.dw_plan(B, G, 64, 0)['ring'] == (B >= 1024)
        assert not SC.dw_plan(B, G, 32, 0)['ring'] and not SC.dw_plan(B, G, 128, 0)['ring']
    # the single-buffer kernel (128 units) takes a second and a third block in a split: its request / deposit of a later block
    assert SC.dw_plan(2100, 40, 128, 0)['units_per_split'] == 3 and SC.dw_plan(4200, 33, 128, 0)['units_per_split'] == 5
    # the double-buffered loop (32 units) goes round more than once
    assert SC.dw_plan(4200, 33, 32, 0)['units_per_split'] == 5
    assert SC.dw2_splits(257, 127) == 16 and SC.dw_splits(257, 127, 64, 1) == 5
    assert SC.dw_rows_per_split(4200, 16, 64, 2) == 272 and SC.dw_rows_per_split(4200, 16, 64, 1) == 320
