"""Scoring a fitted model, the Python layers (Autoencoder.score, Engine.score, `dca --score`) on the CPU oracle extended with
nll_marginals (tests/_score_ref.ScoreRefOps), against the fp64 oracle network on the same parameters."""
import os

import numpy as np
import pandas as pd
import pytest

from conftest import synth_counts
from helpers import make_problem, make_engine
from _score_ref import ScoreRefOps, oracle_score, assert_marginals_close
from dca_amd import io
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle import net_np as N
from oracle.cpu_ops import CpuRefOps

HS = (8, 3, 8)


def _adata(n=90, G=21, seed=3):
    ad = AnnData(synth_counts(n, G, seed).astype(np.float32),
                 obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    return io.normalize(ad, device=False)


def _fitted(ae_type, ad, subset=None, ridge=0.05, **kw):
    G = ad.n_vars
    net = AE_types[ae_type](input_size=G, output_size=len(subset) if subset else G, hidden_size=HS, ridge=ridge)
    net.build()
    train(ad, net, epochs=2, batch_size=32, output_subset=subset, verbose=False, **kw)
    return net


def _oracle(net):
    p = {k: np.asarray(v, np.float64) for k, v in net.engine.get_params().items()}
    return N.OracleAE(net.ae_type, p, HS, True, net.ridge)


@pytest.mark.parametrize('ae_type', ['zinb-conddisp', 'nb', 'normal'])
def test_autoencoder_score_columns_dtypes_and_values(ae_type):
    ad = _adata()
    n, G = ad.shape
    with override_ops(ScoreRefOps):
        net = _fitted(ae_type, ad)
        before = (ad.X.copy(), list(ad.obs.columns), list(ad.var.columns), dict(ad.uns))
        res = net.score(ad, copy=True)
        assert res is not ad and 'dca_nll' not in ad.obs.columns and 'dca_nll' not in ad.var.columns \
            and 'dca_nll' not in ad.uns
        np.testing.assert_array_equal(ad.X, before[0])
        assert (list(ad.obs.columns), list(ad.var.columns), dict(ad.uns)) == before[1:]
        assert net.score(ad) is None                               # in place, like predict
    for a in (res, ad):
        assert a.obs['dca_nll'].dtype == np.float64 and a.var['dca_nll'].dtype == np.float64
        assert isinstance(a.uns['dca_nll'], float)
        assert a.obs['dca_nll'].shape == (n,) and a.var['dca_nll'].shape == (G,)
    np.testing.assert_array_equal(res.obs['dca_nll'].values, ad.obs['dca_nll'].values)
    cell_ref, gene_ref = oracle_score(_oracle(net), ad.X, ad.raw.X, ad.obs['size_factors'].values)
    assert_marginals_close(ad.obs['dca_nll'].values * G, ad.var['dca_nll'].values * n, cell_ref, gene_ref, ae_type)
    assert abs(ad.uns['dca_nll'] - cell_ref.sum() / (n * G)) <= 1e-5 * abs(cell_ref.sum() / (n * G))
    assert abs(ad.uns['dca_nll'] - ad.obs['dca_nll'].mean()) <= 1e-12 * abs(ad.uns['dca_nll'])
    assert abs(ad.uns['dca_nll'] - ad.var['dca_nll'].mean()) <= 1e-12 * abs(ad.uns['dca_nll'])


def test_autoencoder_score_of_a_gene_subset_network():
    ad = _adata()
    n, G = ad.shape
    subset = ['g%d' % i for i in (17, 2, 9, 11, 0)]
    cols = [17, 2, 9, 11, 0]
    with override_ops(ScoreRefOps):
        net = _fitted('zinb-conddisp', ad, subset=subset)
        net.score(ad, output_subset=subset)
    v = ad.var['dca_nll'].values
    outside = np.setdiff1d(np.arange(G), cols)
    assert np.isnan(v[outside]).all() and np.isfinite(v[cols]).all()
    cell_ref, gene_ref = oracle_score(_oracle(net), ad.X, ad.raw.X[:, cols], ad.obs['size_factors'].values)
    assert_marginals_close(ad.obs['dca_nll'].values * len(cols), v[cols] * n, cell_ref, gene_ref, 'subset')
    assert abs(ad.uns['dca_nll'] - cell_ref.sum() / (n * len(cols))) <= 1e-5 * ad.uns['dca_nll']


def test_autoencoder_score_with_the_normalised_matrix_as_target():
    """use_raw_as_output=False (train.py:87): the targets are adata.X itself."""
    ad = _adata()
    n, G = ad.shape
    with override_ops(ScoreRefOps):
        net = _fitted('normal', ad, use_raw_as_output=False)
        net.score(ad, use_raw_as_output=False)
    cell_ref, gene_ref = oracle_score(_oracle(net), ad.X, ad.X, ad.obs['size_factors'].values)
    assert_marginals_close(ad.obs['dca_nll'].values * G, ad.var['dca_nll'].values * n, cell_ref, gene_ref, 'normal on X')
    with override_ops(ScoreRefOps):
        net.score(ad)                                              # the raw counts as targets: another number
    assert abs(ad.obs['dca_nll'].values * G - cell_ref).max() > 1e-3 * abs(cell_ref).max()


def test_engine_score_refusals():
    n, G = 40, 9
    X, Y, sf, p = make_problem(n, G, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.score()
    eng = make_engine(ScoreRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    eng.load_data(X, None, sf)
    with pytest.raises(ValueError, match='needs the targets Y'):
        eng.score()
    eng.load_data(X, Y, sf)
    with pytest.raises(ValueError, match='rows'):
        eng.score(0, n + 1)
    res = eng.score(5, 29, chunk=7)                                # a row range, ragged chunks
    cell_ref, _ = oracle_score(N.OracleAE('zinb-conddisp', {k: np.asarray(v, np.float64) for k, v in p.items()}, HS, True, 0.05),
                               X, Y, sf)
    assert res['cell'].shape == (24,) and res['gene'].shape == (G,)
    np.testing.assert_allclose(res['cell'].numpy(), cell_ref[5:29], rtol=2e-5)

    class TwoRanks:
        rank, world, dp = 0, 2, False
    eng.comm = TwoRanks()
    with pytest.raises(ValueError, match='data-parallel'):
        eng.score()


def _write_counts(tmp_path, n=64, G=18, seed=5):
    y = synth_counts(n, G, seed)
    genes = ['g%d' % i for i in range(G)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


def test_cli_score_files(tmp_path, capsys, monkeypatch):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    scored = {}
    real = AE_types['zinb-conddisp'].score

    def spy(self, adata, **kw):
        r = real(self, adata, **kw)
        scored['obs'], scored['var'], scored['uns'] = adata.obs['dca_nll'].copy(), adata.var['dca_nll'].copy(), adata.uns['dca_nll']
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'score', spy)
    with override_ops(ScoreRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8', '--score', '--testsplit'])
    assert os.path.exists(os.path.join(out, 'cell_nll.tsv')) and os.path.exists(os.path.join(out, 'gene_nll.tsv'))
    mean = pd.read_csv(os.path.join(out, 'mean.tsv'), sep='\t', index_col=0)
    cell = pd.read_csv(os.path.join(out, 'cell_nll.tsv'), sep='\t', index_col=0)
    gene = pd.read_csv(os.path.join(out, 'gene_nll.tsv'), sep='\t', index_col=0)
    assert list(cell.columns) == ['nll', 'split'] and list(gene.columns) == ['nll']
    assert list(cell.index) == list(mean.columns) == cells and list(gene.index) == list(mean.index) == genes
    assert set(cell['split']) == {'train', 'test'}
    np.testing.assert_array_equal(cell['nll'].values, np.array(['%.6f' % v for v in scored['obs'].values], dtype=np.float64))
    np.testing.assert_array_equal(gene['nll'].values, np.array(['%.6f' % v for v in scored['var'].values], dtype=np.float64))
    # every figure of the files has six decimals
    for name in ('cell_nll.tsv', 'gene_nll.tsv'):
        for line in open(os.path.join(out, name)).read().splitlines()[1:]:
            assert len(line.split('\t')[1].split('.')[1]) == 6, line
    line = [l for l in capsys.readouterr().out.splitlines() if 'mean NLL' in l]
    assert len(line) == 1 and 'train' in line[0] and 'test' in line[0]
    for k in ('train', 'test'):
        assert ('%s: %.6f' % (k, cell['nll'][cell['split'] == k].mean())) in line[0] or \
            ('%s: %.6f' % (k, scored['obs'].values[(cell['split'] == k).values].mean())) in line[0]


def test_cli_without_score_writes_todays_files(tmp_path, capsys):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    with override_ops(ScoreRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8', '--testsplit'])
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'latent.tsv', 'mean.tsv', 'model.pickle']
    assert 'NLL' not in capsys.readouterr().out
