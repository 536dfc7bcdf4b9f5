"""Molecular cross-validation, the layers that run without a GPU: the numpy restatement of K-SPLIT's draw (dca_amd/mcv.py
thin_counts_host: what tests/test_mcv_gpu.py holds dcahip_csr_thin to, bit for bit), split_counts, mcv() on the CPU oracle ops,
the hyper-parameter objective and the command line.

The statistical bars are caps, not measurements: |z| <= 4 for 15 + 45 z-scores (a numpy prototype of the same definition on
the same problem and seeds gave 2.01 at worst)."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _mcv_cases as C
from conftest import synth_counts
from _score_ref import ScoreRefOps
from dca_amd import hyper, io, mcv
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.network import override_ops, AE_types
from oracle import net_np as N


def test_philox_is_the_oracles():
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, size=(4, 1000), dtype=np.uint64)
    for k0, k1 in ((0, 0), (0xa4093822, 0x299f31d0), (2 ** 32 - 1, 7)):
        got = mcv.philox4x32_10(*ctr, k0, k1)
        ref = N.philox4x32_10(*ctr, k0, k1)
        for g, r in zip(got, ref):
            assert g.dtype == np.uint32 and np.array_equal(g, r)
    # Random123's known answer for the counter and key of pi digits
    got = mcv.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert tuple(int(x) for x in got) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_problem_has_the_planted_shapes():
    M = C.dense()
    ip, ix, v = C.csr()
    assert (M[7, 11], M[0, 0], M[1, 1], M[2, 2]) == (100000, 65, 64, 5)
    assert len(v) == 86043 and int(M.sum()) == int(v.sum()) and (v == 0).sum() == len(C.ZERO_ROWS)
    assert {1, 4, 5, 64, 65, 100000} <= set(np.unique(v).astype(int).tolist())
    assert np.diff(ip).max() >= 290


@pytest.mark.parametrize('seed', [0, 2 ** 40 + 3])
@pytest.mark.parametrize('threshold', C.THRESHOLDS)
def test_host_split_adds_up_and_keeps_the_order(threshold, seed):
    M = C.dense()
    pa, ia, va, pb, ib, vb = C.host_split(threshold, seed)
    assert pa.dtype == pb.dtype == np.int64 and ia.dtype == ib.dtype == np.int32 and va.dtype == vb.dtype == np.float32
    A, B = C.to_dense(pa, ia, va), C.to_dense(pb, ib, vb)
    assert np.array_equal(A + B, M)
    for ptr, idx, val in ((pa, ia, va), (pb, ib, vb)):
        assert ptr[0] == 0 and ptr[-1] == len(idx) == len(val) and (val >= 1).all()         # no stored zero survives
        inner = np.ones(len(idx), bool)
        inner[ptr[1:-1][ptr[1:-1] < len(idx)]] = False
        assert (np.diff(idx.astype(np.int64))[inner[1:]] > 0).all()                         # column order inside every row
        assert ptr[4] == ptr[3] and ptr[300] == ptr[299]                                    # rows 3 and 299 stay empty
    if threshold == 0:
        assert len(va) == 0 and np.array_equal(B, M)
    if threshold == 2 ** 32:
        assert len(vb) == 0 and np.array_equal(A, M)
    if threshold == 1:
        assert A.sum() <= 3                                # 411 019 molecules at p = 2^-32
    if threshold == 2 ** 32 - 1:
        assert B.sum() <= 3


def test_host_split_depends_on_the_cell_not_on_the_row():
    thr, seed = C.THRESHOLDS[3], 0
    full = C.host_split(thr, seed)
    A, B = C.to_dense(*full[:3]), C.to_dense(*full[3:])
    rows = np.random.RandomState(1).permutation(C.N)[:97].tolist() + [7, 0]
    rows = list(dict.fromkeys(rows))
    sub = C.host_split(thr, seed, rows=rows)
    assert np.array_equal(C.to_dense(*sub[:3]), A[rows]) and np.array_equal(C.to_dense(*sub[3:]), B[rows])
    # the same rows WITHOUT their ids are other cells: another draw
    ip, ix, v = C.take_rows(rows)
    other = mcv.thin_counts_host(ip, ix, v, None, thr, seed)
    assert not np.array_equal(C.to_dense(*other[:3]), A[rows])
    # seeds
    again = mcv.thin_counts_host(*C.csr(), None, thr, seed)
    assert all(np.array_equal(x, y) for x, y in zip(again, full))
    assert not np.array_equal(C.to_dense(*C.host_split(thr, 1)[:3]), A)
    assert not np.array_equal(C.to_dense(*C.host_split(thr, 2 ** 32)[:3]), A)            # the key's high word counts


def test_host_split_does_not_depend_on_where_large_counts_start(monkeypatch):
    """Counts above mcv._ONE_BY_ONE are drawn one entry at a time: the same bits wherever that line is."""
    thr = C.THRESHOLDS[3]
    rows = [0, 1, 2, 4, 5, 6, 8, 9]                     # counts of 65, 64 and 5 among them (the 100 000 of row 7 stays out: one
    ref = C.host_split(thr, 0, rows=rows)               # Philox block per pass would take 25 000 passes)
    for cut in (2, 64, 70):
        monkeypatch.setattr(mcv, '_ONE_BY_ONE', cut)
        got = mcv.thin_counts_host(*C.take_rows(rows), np.asarray(rows), thr, 0)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), cut


@pytest.mark.parametrize('f', [0.5, 0.8, 0.1])
def test_split_statistics(f):
    M = C.dense()
    thr = mcv.threshold_of(f)
    p = thr / 2.0 ** 32
    total = int(M.sum())
    two = M == 2
    n2 = int(two.sum())
    assert n2 == 16404
    cells = np.array([(1 - p) ** 2, 2 * p * (1 - p), p * p])
    for seed in range(5):
        A = C.to_dense(*C.host_split(thr, seed)[:3])
        z = (A.sum() - total * p) / np.sqrt(total * p * (1 - p))
        got = np.bincount(A[two], minlength=3)
        z2 = (got - n2 * cells) / np.sqrt(n2 * cells * (1 - cells))
        print('f %.1f seed %d: z %.2f, y = 2 cells z %s' % (f, seed, z, np.round(z2, 2)))
        assert abs(z) <= 4 and (np.abs(z2) <= 4).all()


# ---------------------------------------------------------------------------------------------------- split_counts
def _adata(X, n, G):
    return AnnData(X, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]), var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


def test_split_counts_dense_and_sparse():
    ip, ix, v = C.csr()
    S = sp.csr_matrix((v.copy(), ix.copy(), ip.copy()), shape=(C.N, C.G))
    state = np.random.get_state()[1].copy()
    fs, hs = mcv.split_counts(_adata(S, C.N, C.G), 0.8, seed=0)
    fd, hd = mcv.split_counts(_adata(C.dense().astype(np.float32), C.N, C.G), 0.8, seed=0)
    assert np.array_equal(np.random.get_state()[1], state)                  # numpy's global stream is not consumed
    assert sp.issparse(fs.X) and fs.X.format == 'csr' and fs.X.dtype == np.float32 and isinstance(fd.X, np.ndarray)
    assert np.array_equal(fs.X.toarray(), fd.X) and np.array_equal(hs.X.toarray(), hd.X)
    assert np.array_equal(fd.X + hd.X, C.dense())
    ref = C.host_split(C.THRESHOLDS[3], 0)
    assert np.array_equal(fs.X.indptr, ref[0]) and np.array_equal(fs.X.indices, ref[1]) and np.array_equal(fs.X.data, ref[2])
    assert np.array_equal(hs.X.indptr, ref[3]) and np.array_equal(hs.X.indices, ref[4]) and np.array_equal(hs.X.data, ref[5])
    for part in (fs, hs, fd, hd):
        assert list(part.obs_names) == ['c%d' % i for i in range(C.N)] and list(part.var_names) == ['g%d' % i for i in range(C.G)]


@pytest.mark.parametrize('bad', [0.5, -1.0, float(2 ** 25)])
def test_split_counts_refuses_what_is_not_a_count(bad):
    X = C.dense()[:20, :30].astype(np.float32)
    X[4, 7] = bad
    for form in (X, sp.csr_matrix(X)):
        with pytest.raises(ValueError, match='not counts'):
            mcv.split_counts(_adata(form, 20, 30), 0.5)


def test_split_counts_takes_the_largest_count():
    X = C.dense()[:20, :30].astype(np.float32)
    X[4, 7] = float(2 ** 24)                                                 # the largest count fp32 carries exactly
    f, h = mcv.split_counts(_adata(X, 20, 30), 0.5)
    assert f.X[4, 7] + h.X[4, 7] == 2 ** 24 and abs(f.X[4, 7] - 2 ** 23) <= 4 * 2 ** 11


@pytest.mark.parametrize('fraction', [0, 1, 0.0, 1.0, -0.1, 1.5])
def test_split_counts_refuses_a_fraction_outside_the_open_interval(fraction):
    with pytest.raises(ValueError, match='fraction'):
        mcv.split_counts(_adata(C.dense()[:5, :5].astype(np.float32), 5, 5), fraction)


# ---------------------------------------------------------------------------------------------------- mcv()
HS = (16, 8, 16)
N_CELLS, N_GENES, F, SEED = 200, 120, 0.8, 3
LONELY = 57                      # a gene made to hold one molecule only, in a cell whose draw sends it to the held-out part


def _counts():
    y = synth_counts(N_CELLS, N_GENES, 8).astype(np.float32)
    y[:, LONELY] = 0
    thr = mcv.threshold_of(F)
    for i in range(N_CELLS):
        one = mcv.thin_counts_host(np.array([0, 1]), np.array([LONELY]), np.array([1.0]), np.array([i]), thr, SEED)
        if len(one[2]) == 0:
            y[i, LONELY] = 1
            return y, i
    raise AssertionError('no cell sends the molecule to the held-out part')


@pytest.fixture(scope='module')
def fitted():
    y, cell = _counts()
    ad = _adata(y, N_CELLS, N_GENES)
    before = y.copy()
    with override_ops(ScoreRefOps):
        res = mcv.mcv(ad, fraction=F, seed=SEED, return_model=True, ae_type='zinb-conddisp', hidden_size=HS, epochs=2,
                      verbose=False)
    assert np.array_equal(ad.X, before) and 'dca_split' not in ad.obs.columns          # the caller's data is untouched
    return ad, res, cell


def _by_hand(ad, net, scale):
    """The evaluation set rebuilt from split_counts and the documented recipe, scored by the fitted network."""
    work = io.read_dataset(ad, copy=True)
    fit, held = mcv.split_counts(work, F, SEED)
    genes = np.asarray(fit.X.sum(axis=0)).reshape(-1) > 0
    fit, held = fit[:, genes].copy(), held[:, genes].copy()
    cells = np.asarray(fit.X.sum(axis=1)).reshape(-1) > 0
    fit, held = fit[cells].copy(), held[cells].copy()
    fit = io.normalize(fit, filter_min_counts=False, device=False)
    ev = _adata(fit.X, fit.n_obs, fit.n_vars)
    ev.raw = held
    ev.obs['size_factors'] = fit.obs['size_factors'].values * scale
    with override_ops(ScoreRefOps):
        net.score(ev)
    return ev, genes, cells


def test_mcv_scores_the_held_out_part_with_scaled_size_factors(fitted):
    ad, res, cell = fitted
    ev, genes, cells = _by_hand(ad, res['model'], (1 - F) / F)
    assert abs(res['mcv_loss'] - ev.uns['dca_nll']) <= 1e-12 * abs(ev.uns['dca_nll'])
    np.testing.assert_allclose(res['gene_nll'], ev.var['dca_nll'].values, rtol=1e-12)
    np.testing.assert_allclose(res['cell_nll'], ev.obs['dca_nll'].values, rtol=1e-12)
    assert res['cell_nll'].shape == (res['n_cells'],) and res['gene_nll'].shape == (res['n_genes'],)      # ALL cells
    assert abs(res['mcv_loss'] - res['cell_nll'].mean()) <= 1e-12 * abs(res['mcv_loss'])
    plain, _, _ = _by_hand(ad, res['model'], 1.0)                            # a forgotten (1 - f) / f
    assert abs(plain.uns['dca_nll'] - res['mcv_loss']) > 1e-3 * abs(res['mcv_loss'])
    assert set(res) >= {'mcv_loss', 'gene_nll', 'cell_nll', 'history', 'fraction', 'seed', 'n_cells', 'n_genes', 'model'}
    assert res['fraction'] == F and res['seed'] == SEED and len(res['history']['loss']) == 2
    assert np.isfinite(res['mcv_loss']) and np.isfinite(res['gene_nll']).all() and np.isfinite(res['cell_nll']).all()


def test_mcv_drops_what_the_fit_part_does_not_hold(fitted):
    ad, res, cell = fitted
    _, genes, cells = _by_hand(ad, res['model'], 1.0)
    assert not genes[LONELY] and ad.X[cell, LONELY] == 1                    # its one molecule went to the held-out part
    assert res['genes_dropped'] == int((~genes).sum()) >= 1 and res['cells_dropped'] == int((~cells).sum())
    assert res['n_genes'] == N_GENES - res['genes_dropped'] and res['n_cells'] == N_CELLS - res['cells_dropped']
    assert 'g%d' % LONELY not in set(res['gene_names'])


def test_mcv_without_the_model_and_with_unknown_arguments(fitted):
    ad = fitted[0]
    with pytest.raises(TypeError, match='mode'):
        mcv.mcv(ad, mode='latent')
    with pytest.raises(ValueError, match='fraction'):
        mcv.mcv(ad, fraction=1.0)


# ---------------------------------------------------------------------------------------------------- hyper, command line
def _params():
    return {'data': {'norm_input_log': True, 'norm_input_zeromean': True, 'norm_input_sf': True},
            'model': {'lr': 1e-3, 'ridge': 1e-3, 'l1_enc_coef': 1e-6, 'hidden_size': (16,), 'activation': 'relu',
                      'aetype': 'zinb-conddisp', 'batchnorm': True, 'dropout': 0.0, 'input_dropout': 0.0}}


def test_hyper_objective(monkeypatch):
    ad = io.read_dataset(_adata(synth_counts(90, 40, 2).astype(np.float32), 90, 40), copy=True)
    scored = []
    real = AE_types['zinb-conddisp'].score

    def spy(self, adata, **kw):
        r = real(self, adata, **kw)
        scored.append((adata.uns['dca_nll'], adata.n_obs, np.asarray(adata.obs['size_factors'].values).copy()))
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'score', spy)
    with override_ops(ScoreRefOps):
        np.random.seed(1)
        today = hyper.evaluate(ad, _params(), 2)
        np.random.seed(1)
        none = hyper.evaluate(ad, _params(), 2, mcv=None)
        assert not scored                                                   # mcv=None: today's objective, nothing scored
        np.random.seed(1)
        loss, hist = hyper.evaluate(ad, _params(), 2, mcv=0.5)
        np.random.seed(1)
        again, _ = hyper.evaluate(ad, _params(), 2, mcv=0.5, _parts=hyper.mcv_parts(ad, 0.5))
    assert today[0] == none[0] == min(today[1]['val_loss']) and today[1] == none[1]
    assert len(scored) == 2 and loss == scored[0][0] and scored[0][1] == 90                 # every cell is scored
    assert loss != min(hist['val_loss'])
    assert again == loss                                                     # seed 42: the same split for every trial


def _write_counts(tmp_path, n=64, G=18, seed=5):
    y = synth_counts(n, G, seed)
    genes, cells = ['g%d' % i for i in range(G)], ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


def test_cli_mcv_files(tmp_path, capsys):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    with override_ops(ScoreRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8', '--mcv', '0.8'])
    assert sorted(os.listdir(out)) == ['cell_mcv_nll.tsv', 'gene_mcv_nll.tsv', 'mcv.json']          # no denoising run
    js = json.load(open(os.path.join(out, 'mcv.json')))
    assert js['fraction'] == 0.8 and js['seed'] == 42 and np.isfinite(js['mcv_loss'])
    assert all(isinstance(v, (int, float, str)) for v in js.values())
    gene = pd.read_csv(os.path.join(out, 'gene_mcv_nll.tsv'), sep='\t', index_col=0)
    cell = pd.read_csv(os.path.join(out, 'cell_mcv_nll.tsv'), sep='\t', index_col=0)
    assert list(gene.columns) == ['nll'] and list(cell.columns) == ['nll']
    assert len(gene) == js['n_genes'] and len(cell) == js['n_cells'] and set(gene.index) <= set(genes) and set(cell.index) <= set(cells)
    assert abs(cell['nll'].mean() - js['mcv_loss']) <= 1e-5
    assert ('%.6f' % js['mcv_loss']) in capsys.readouterr().out


def test_cli_hypermcv_marks_the_objective(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    outs = {}
    for name, extra in (('plain', []), ('mcv', ['--hypermcv', '0.5'])):
        out = str(tmp_path / name)
        with override_ops(ScoreRefOps):
            main([f, out, '-t', '--hyper', '--hypern', '1', '--hyperepoch', '1'] + extra)
        outs[name] = json.load(open(os.path.join(out, 'hyperopt_results', 'best.json')))
    assert 'objective' not in outs['plain'] and outs['mcv']['objective'] == 'mcv'
    assert outs['plain']['model'] == outs['mcv']['model'] and outs['plain']['loss'] != outs['mcv']['loss']
