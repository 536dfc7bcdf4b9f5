"""Gene cross-products on the MI355X: dcahip_gram alone -- exact on integer data (the fragment map of the fp64 matrix
instruction, the mirror and the cols gather), against fp64 within the derived bound E of tests/_gram_ref.py at the edges of
the tile, of the instruction's depth and of the staging depth and on both sides of the plan's slice boundary, its bitwise
properties and its argument checks; Engine.gene_gram in both residency modes against what predict_chunk writes;
Autoencoder.gene_correlation, top_partners and `dca --genecorr` end to end against np.corrcoef of predict().

Every bar is E_ij = (m + 4) 2^-53 sum_r |d_ri| |d_rj| of the call's own operands (m kept rows), plus half an ulp of the
preloaded accumulator where the result is added to one (tests/_gram_ref.py derives both)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine
from _gram_ref import (SHAPES, VARIANTS, MAX_G, U, plan, boundary_shapes, row_block_shape, case, int_case, gram_ref, bound,
                       acc_half_ulp, to_int_tensor)
from oracle import net_np as N

pytestmark = pytest.mark.gpu

EINVAL = -22
ALL_SHAPES = SHAPES + list(boundary_shapes())
_ids = lambda s: '%dx%d' % s


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _base(G, ldc):
    """Known accumulator contents: small integers, none of them zero, symmetric over the square; (cross, dsum)."""
    i = torch.arange(G)[:, None]
    j = torch.arange(ldc)[None, :]
    sq = (1 + (i + j) % 8).to(torch.float64)
    sq[:, G:] = 77.0
    return sq.cuda(), (1 + torch.arange(G) % 5).to(torch.float64).cuda()


def _call(ops, c, B, G, pad=2, rows=None, acc=None):
    """One dcahip_gram call on the operands c (rows: a slice of them) onto the preloaded accumulators (acc: onto these)."""
    rows = slice(0, B) if rows is None else rows
    x = torch.full((B, c['ldx']), float('nan'), dtype=torch.float32)
    x[:, :c['x'].shape[1]] = torch.from_numpy(c['x'])
    x = x[rows].contiguous().cuda()
    b = x.shape[0]
    keep = to_int_tensor(None if c['keep'] is None else c['keep'][rows])
    cross, dsum = _base(G, G + pad) if acc is None else acc
    nws = ops.gram_workspace_doubles(b, G)
    ws = torch.full((nws,), float('nan'), dtype=torch.float64, device='cuda') if nws else None
    cols = to_int_tensor(c['cols'])
    ops.gram(x, c['ldx'], cols.cuda() if cols is not None else None, keep.cuda() if keep is not None else None,
             torch.from_numpy(c['shift']).cuda(), b, G, cross, G + pad, dsum, ws)
    torch.cuda.synchronize()
    return cross, dsum


# ---------------------------------------------------------------------------------------------------- (a) exact layout
@pytest.mark.parametrize('shape', ALL_SHAPES, ids=_ids)
def test_integer_data_is_exact(ops, shape):
    """Integer-valued fp32 data with |x| <= 64 and integer shifts: every sum is exact in double, so cross and dsum equal
    the int64 numpy result bit for bit.  A wrong row map of the fp64 result fragment (the f32 formula puts 3 of 4 results in
    the wrong row), a wrong mirror or a wrong cols gather cannot pass: the data is not symmetric in any way."""
    B, G = shape
    c = int_case(shape)
    base_c, base_d = _base(G, G + 2)
    cross, dsum = _call(ops, c, B, G)
    assert torch.equal(cross[:, G:], base_c[:, G:])                              # ldc > G: the pad is not touched
    got_c = (cross - base_c)[:, :G].cpu().numpy()
    got_d = (dsum - base_d).cpu().numpy()
    assert np.array_equal(got_d, c['dsum'].astype(np.float64))
    wrong = np.argwhere(got_c != c['cross'].astype(np.float64))
    assert not len(wrong), (len(wrong), wrong[:8].tolist())


def test_integer_data_is_exact_over_two_row_blocks(ops):
    """More rows than fit the workspace beside the partial tiles: the call takes them in two row blocks, one after the
    other onto the same accumulators (the only shape of this file that does; exact, so any row lost or taken twice shows)."""
    B, G = shape = row_block_shape()
    assert len(plan(B, G)['blocks']) == 2 and plan(B, G)['S'] == 2 and ops.gram_workspace_doubles(B, G) * 8 <= 64 << 20
    c = int_case(shape)
    base_c, base_d = _base(G, G + 2)
    cross, dsum = _call(ops, c, B, G)
    assert np.array_equal((dsum - base_d).cpu().numpy(), c['dsum'].astype(np.float64))
    assert np.array_equal((cross - base_c)[:, :G].cpu().numpy(), c['cross'].astype(np.float64))
    assert torch.equal(cross[:, G:], base_c[:, G:])


# ---------------------------------------------------------------------------------------------------- (b) against fp64
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', ALL_SHAPES, ids=_ids)
def test_kernel_against_fp64(ops, shape, variant):
    B, G = shape
    c = case(shape, variant)
    p = plan(B, G)
    base_c, base_d = _base(G, G + 2)
    cross, dsum = _call(ops, c, B, G)
    assert torch.equal(cross[:, G:], base_c[:, G:])                              # ldc > G: the pad is not touched
    if variant == 'keepnone':                                                   # no kept row: the accumulators keep their bits
        assert torch.equal(cross, base_c) and torch.equal(dsum, base_d)
        return
    assert torch.equal(cross[:, :G], cross[:, :G].T)                            # symmetric bit for bit
    got_c, got_d = (cross - base_c)[:, :G].cpu().numpy(), (dsum - base_d).cpu().numpy()      # exact: the base is small integers
    assert np.isfinite(got_c).all() and np.isfinite(got_d).all()                # no NaN of a row that is out, of the pad, of ws
    bar_c = bound(c['absprod'], c['m']) + acc_half_ulp(cross[:, :G].cpu().numpy())
    bar_d = bound(c['absd'], c['m']) + acc_half_ulp(dsum.cpu().numpy())
    e_c, e_d = np.abs(got_c - c['cross']), np.abs(got_d - c['dsum'])
    print('%s %s (%d slices): worst error / bar cross %.3f, dsum %.3f' % (shape, variant, p['S'], (e_c / bar_c).max(),
                                                                          (e_d / bar_d).max()))
    assert (e_c <= bar_c).all(), float((e_c / bar_c).max())
    assert (e_d <= bar_d).all(), float((e_d / bar_d).max())


def test_shapes_reach_both_sides_of_the_slice_boundary():
    multi, single = boundary_shapes()
    assert multi in ALL_SHAPES and single in ALL_SHAPES
    assert plan(*multi)['S'] > 1 and plan(*single)['S'] == 1 and plan(*multi)['capmax'] > 1 == plan(*single)['capmax']
    assert {plan(*s)['S'] > 1 for s in SHAPES} == {True, False}                  # the small shapes take both forms too


# ---------------------------------------------------------------------------------------------------- (c) bitwise properties
@pytest.mark.parametrize('shape', [(37, 65), (300, 200), boundary_shapes()[1]], ids=_ids)
def test_two_calls_give_the_same_bits(ops, shape):
    B, G = shape
    c = case(shape, 'keep10')
    a_c, a_d = _call(ops, c, B, G)
    b_c, b_d = _call(ops, c, B, G)
    assert torch.equal(a_c, b_c) and torch.equal(a_d, b_d)
    assert torch.equal(a_c[:, :G], a_c[:, :G].T)


@pytest.mark.parametrize('shape', [(70, 130), (300, 200)], ids=_ids)
def test_two_halves_accumulate_to_the_whole(ops, shape):
    """The kernel ADDS: the first half of the rows, then the second half onto the same accumulators, against one call --
    both are sums of the same terms, each inside E of the whole (plus the accumulators' roundings)."""
    B, G = shape
    c = case(shape, 'plain')
    whole_c, whole_d = _call(ops, c, B, G)
    acc = _call(ops, c, B, G, rows=slice(0, B // 2))
    half_c, half_d = _call(ops, c, B, G, rows=slice(B // 2, B), acc=acc)
    assert torch.equal(half_c[:, :G], half_c[:, :G].T)
    bar_c = 2 * bound(c['absprod'], c['m']) + 3 * acc_half_ulp(whole_c[:, :G].cpu().numpy())
    bar_d = 2 * bound(c['absd'], c['m']) + 3 * acc_half_ulp(whole_d.cpu().numpy())
    assert ((half_c - whole_c)[:, :G].abs().cpu().numpy() <= bar_c).all()
    assert ((half_d - whole_d).abs().cpu().numpy() <= bar_d).all()
    base_c, _ = _base(G, G + 2)
    e = np.abs((half_c - base_c)[:, :G].cpu().numpy() - c['cross'])
    assert (e <= bound(c['absprod'], c['m']) + 2 * acc_half_ulp(half_c[:, :G].cpu().numpy())).all()


# ---------------------------------------------------------------------------------------------------- (d) invalid arguments
def test_kernel_argument_errors_launch_nothing(ops):
    from dca_amd import hip
    L, p = hip.lib(), hip.ptr
    B, G = 40, 8                                                      # two slices: a workspace is needed
    x = torch.ones(B, G, dtype=torch.float32, device='cuda')
    sh = torch.zeros(G, dtype=torch.float64, device='cuda')
    cross = torch.full((G, G), 7.0, dtype=torch.float64, device='cuda')
    dsum = torch.full((G,), 9.0, dtype=torch.float64, device='cuda')
    assert plan(B, G)['S'] == 2
    ws = torch.zeros(ops.gram_workspace_doubles(B, G), dtype=torch.float64, device='cuda')

    def call(B=B, G=G, x_=x, sh_=sh, cross_=cross, dsum_=dsum, ws_=ws, ldx=G, ldc=G):
        return L.dcahip_gram(p(x_), ldx, None, None, p(sh_), B, G, p(cross_), ldc, p(dsum_), p(ws_), hip.stream())
    assert call(x_=None) == EINVAL and call(sh_=None) == EINVAL and call(cross_=None) == EINVAL and call(dsum_=None) == EINVAL
    assert call(ldc=G - 1) == EINVAL and call(ldx=0) == EINVAL and call(G=0) == EINVAL and call(G=MAX_G + 1) == EINVAL
    assert call(B=-1) == EINVAL and call(ws_=None) == EINVAL
    q = L.dcahip_gram_workspace_doubles
    assert q(B, 0) == EINVAL and q(B, MAX_G + 1) == EINVAL and q(0, G) == 0
    assert q(4096, MAX_G) == plan(4096, MAX_G)['ws'] == (64 << 20) // 8 and q(4096, 512) == plan(4096, 512)['ws']
    torch.cuda.synchronize()
    assert (cross == 7.0).all() and (dsum == 9.0).all()
    assert call(B=0) == 0                                              # no rows: nothing to add, not an error
    torch.cuda.synchronize()
    assert (cross == 7.0).all() and (dsum == 9.0).all()
    assert call() == 0
    assert call(B=32, ws_=None) == 0                                   # one slice: no workspace is needed
    torch.cuda.synchronize()
    assert (cross == 7.0 + B + 32).all() and (dsum == 9.0 + B + 32).all()      # d = 1 - 0 in every row


# ---------------------------------------------------------------------------------------------------- (e) Engine.gene_gram
HS = (12, 5, 12)


def test_engine_gene_gram_in_both_residency_modes(ops, monkeypatch):
    """Engine.gene_gram on dense and on counts-resident data: identical bit for bit, and within E of the reference evaluated
    on what predict_chunk returns for the same rows (the same fp32 values).  Chunks of 64 do not divide the 150 rows; the
    keep mask empties the first chunk, so the shift is zeros."""
    import scipy.sparse as sp
    from dca_amd import prep
    from dca_amd._anndata import AnnData
    from dca_amd.engine import Engine
    n, G, ae = 150, 33, 'zinb-conddisp'
    p = {k: np.asarray(v, np.float32) for k, v in N.init_params(ae, G, HS, batchnorm=True, seed=4).items()}
    cols = np.random.default_rng(0).permutation(G)[:20]
    keep = np.ones(n, bool)
    keep[:64] = False
    keep[70::9] = False
    res, x = {}, None
    for form in ('dense', 'counts'):
        monkeypatch.setenv('DCA_AMD_RESIDENT', form)
        ad = AnnData(sp.csr_matrix(synth_counts(n, G, 11).astype(np.float32)),
                     obs=pd.DataFrame(index=['c%d' % i for i in range(n)]), var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
        ad, dd = prep.normalize_device(ad, filter_min_counts=False, ops=ops)
        assert (dd.csr is not None) == (form == 'counts')
        eng = Engine(ae, G, G, HS, True, 0.05, ops=ops)
        eng.set_params(p)
        if form == 'dense':
            eng.attach_device_data(dd.X, dd.Y, dd.sf, norm=dd.norm, compact=False)
        else:
            eng.attach_counts(dd.csr, dd.sf, dd.norm)
        res[form] = eng.gene_gram(cols, keep=keep, chunk=64)
        full = eng.gene_gram(cols, chunk=64)
        torch.cuda.synchronize()
        if form == 'dense':
            x = np.concatenate([eng.predict_chunk(s, min(64, n - s), {'mean'})['mean'].cpu().numpy() for s in range(0, n, 64)])
            res['full'] = full
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    for k in ('cross', 'dsum', 'shift'):
        assert torch.equal(res['dense'][k], res['counts'][k]), k
    assert res['dense']['count'] == res['counts']['count'] == int(keep.sum())
    assert not res['dense']['shift'].cpu().numpy().any()
    for r, kp in ((res['dense'], keep), (res['full'], None)):
        shift = r['shift'].cpu().numpy()
        ref = gram_ref(x, cols, kp, shift)
        m = ref[4]
        cross, dsum = r['cross'].cpu().numpy(), r['dsum'].cpu().numpy()
        assert np.array_equal(cross, cross.T) and r['count'] == m
        # three chunks are added onto the accumulator one after the other: half an ulp each
        e_c, bar_c = np.abs(cross - ref[0]), bound(ref[2], m) + 3 * acc_half_ulp(cross)
        e_d, bar_d = np.abs(dsum - ref[1]), bound(ref[3], m) + 3 * acc_half_ulp(dsum)
        print('engine: worst error / bar cross %.3f, dsum %.3f' % ((e_c / bar_c).max(), (e_d / bar_d).max()))
        assert (e_c <= bar_c).all() and (e_d <= bar_d).all()
    np.testing.assert_allclose(res['full']['shift'].cpu().numpy(), x[:64][:, cols].astype(np.float64).mean(axis=0), rtol=1e-13)


# ---------------------------------------------------------------------------------------------------- (f) the model path
@pytest.fixture(scope='module')
def trained():
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G = 200, 40
    np.random.seed(0)
    ad = AnnData(synth_counts(n, G, 4).astype(np.float32), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    ad = io.normalize(ad)
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(16, 8, 16))
    net.build()
    train(ad, net, epochs=2, early_stop=0, reduce_lr=0, verbose=False)
    x = np.asarray(net.predict(ad, copy=True).X, np.float32)
    return ad, net, x


def _r_bar(v, shift):
    """The bar on r from the reference values v [m, g] (float64 of the fp32 numbers the device summed) and the shift the
    device used: delta_ij = E_ij / sqrt(C_ii C_jj) + E_ii / C_ii + E_jj / C_jj with C the reference's centred cross-products
    and E_ij = (m + 4) 2^-53 sum |d_i| |d_j| <= (m + 4) 2^-53 sqrt(D_i D_j), D_i = sum d_i^2 = C_ii + m (mean_i - shift_i)^2
    (Cauchy-Schwarz, the shift offset included)."""
    m = v.shape[0]
    mean = v.mean(axis=0)
    C = (v - mean).T @ (v - mean)
    Cd = np.diagonal(C)
    D = Cd + m * (mean - shift) ** 2
    E = (m + 4) * U * np.sqrt(np.outer(D, D))
    with np.errstate(divide='ignore', invalid='ignore'):
        return E / np.sqrt(np.outer(Cd, Cd)) + (np.diagonal(E) / Cd)[:, None] + (np.diagonal(E) / Cd)[None, :]


def _check_corr(d, v, shift, what):
    with np.errstate(divide='ignore', invalid='ignore'):
        ref = np.corrcoef(v, rowvar=False)
    const = v.var(axis=0) == 0
    assert np.isnan(d['corr'][const]).all() and np.isnan(d['corr'][:, const]).all()      # reference variance 0: NaN
    ok = ~const
    got, want, bar = d['corr'][np.ix_(ok, ok)], ref[np.ix_(ok, ok)], _r_bar(v, shift)[np.ix_(ok, ok)]
    assert np.isfinite(got).all() and np.array_equal(got, got.T) and (np.diagonal(got) == 1.0).all()
    err = np.abs(got - want)
    print('%s: worst |r - corrcoef| %.3g, worst error / bar %.3f' % (what, err.max(), (err / bar).max()))
    assert (err <= bar).all(), float((err / bar).max())


def test_gene_correlation_against_corrcoef_of_predict(trained):
    ad, net, x = trained
    n, G = x.shape
    before = np.array(ad.X, copy=True)
    assert net.gene_correlation(ad) is None
    np.testing.assert_array_equal(ad.X, before)
    d = ad.uns['dca_gene_corr']
    assert list(d['genes']) == list(ad.var_names) and d['n_cells'] == n and d['corr'].dtype == np.float64
    v = x.astype(np.float64)
    chunk = net._chunk(n)
    shift = v[:chunk].mean(axis=0)                                   # what Engine.gene_gram fixes from its first chunk
    _check_corr(d, v, shift, 'all cells')
    np.testing.assert_allclose(d['mean'], v.mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(d['var'], v.var(axis=0, ddof=1), rtol=1e-9)
    # genes=: their order is the order of the result
    order = ['g31', 'g2', 'g17', 'g0', 'g8']
    idx = [31, 2, 17, 0, 8]
    net.gene_correlation(ad, genes=order, key_added='five')
    assert list(ad.uns['five']['genes']) == order
    _check_corr(ad.uns['five'], v[:, idx], shift[idx], 'five genes')
    # one group's cells on log1p of the mean without size factors
    lab = np.array(['abc'[i % 3] if i % 10 else None for i in range(n)], dtype=object)
    ad.obs['cluster'] = pd.Categorical(lab)
    net.gene_correlation(ad, groupby='cluster', group='b', value='denoised')
    rows = lab == 'b'
    dg = ad.uns['dca_gene_corr']
    assert dg['n_cells'] == rows.sum() and dg['group'] == 'b' and dg['groupby'] == 'cluster'
    _check_corr(dg, v[rows], v[:chunk][rows[:chunk]].mean(axis=0), "group 'b'")
    net.gene_correlation(ad, groupby='cluster', group='b', value='normalized', log1p=True, key_added='lg')
    sf = ad.obs['size_factors'].values.astype(np.float32).astype(np.float64)[:, None]
    np.testing.assert_allclose(ad.uns['lg']['corr'], np.corrcoef(np.log1p(v / sf)[rows], rowvar=False), atol=1e-4)
    # top_partners
    from dca_amd.genecorr import top_partners
    net.gene_correlation(ad)
    names, r = top_partners(ad, 'g5', n=7)
    row = ad.uns['dca_gene_corr']['corr'][5]
    want = [j for j in np.argsort(-np.abs(row), kind='stable') if j != 5 and np.isfinite(row[j])][:7]
    assert list(names) == ['g%d' % j for j in want] and np.array_equal(r, row[want])


def test_gene_correlation_of_a_gene_subset_network():
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G = 120, 30
    np.random.seed(0)
    ad = AnnData(synth_counts(n, G, 6).astype(np.float32), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    ad = io.normalize(ad)
    cols = [17, 2, 9, 11, 0, 25]
    subset = ['g%d' % i for i in cols]
    net = AE_types['zinb-conddisp'](input_size=G, output_size=len(cols), hidden_size=(16, 8, 16))
    net.build()
    train(ad, net, epochs=2, early_stop=0, reduce_lr=0, output_subset=subset, verbose=False)
    with pytest.raises(ValueError, match='output_subset'):
        net.gene_correlation(ad)
    net.gene_correlation(ad, output_subset=subset)
    d = ad.uns['dca_gene_corr']
    assert list(d['genes']) == subset and d['corr'].shape == (6, 6)
    v = np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float32).astype(np.float64)
    _check_corr(d, v, v.mean(axis=0), 'gene subset')


def test_cli_genecorr_file(tmp_path):
    from dca_amd.train import train_with_args
    from dca_amd.__main__ import parse_args
    n, g = 64, 18
    y = synth_counts(n, g, 5)
    genes = ['g%d' % i for i in range(g)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=['c%d' % i for i in range(n)]).to_csv(f, sep='\t')
    gl = str(tmp_path / 'genes.txt')
    with open(gl, 'w') as fh:
        fh.write('g11\ng3\ng7\ng0\n')
    out = str(tmp_path / 'res')
    train_with_args(parse_args([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '16,4,16', '--genecorr', gl]))
    t = pd.read_csv(os.path.join(out, 'gene_corr.tsv'), sep='\t', index_col=0)
    order = ['g0', 'g3', 'g7', 'g11']
    assert list(t.index) == list(t.columns) == order and (np.diagonal(t.values) == 1.0).all()
    mean = pd.read_csv(os.path.join(out, 'mean.tsv'), sep='\t', index_col=0)        # genes x cells, six decimals
    v = mean.loc[order].values.astype(np.float64)
    ref = np.corrcoef(v)
    # the comparison is of the files, to the digits they carry: mean.tsv rounds every value to six decimals, a perturbation e
    # of a gene's n values with |e| <= 5e-7 each, ||e|| <= 5e-7 sqrt(n); to first order r_ij moves by at most
    # ||e_i|| / ||c_i|| + ||e_j|| / ||c_j|| (c the centred values), held with a factor two to spare; gene_corr.tsv rounds r
    # itself to six decimals
    norm = np.sqrt(((v - v.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
    bar = 2 * 5e-7 * np.sqrt(n) * (1 / norm[:, None] + 1 / norm[None, :]) + 5e-7
    err = np.abs(t.values - ref)
    print('gene_corr.tsv against corrcoef of mean.tsv: worst error / bar %.3f' % (err / bar).max())
    assert (err <= bar).all()
    assert np.array_equal(t.values, t.values.T)
