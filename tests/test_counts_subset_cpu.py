"""Counts-resident training for a gene subset (train(output_subset=...)) without a GPU: the engine gathering all input
genes and the fitted genes' counts from the CSR on the CPU oracle -- bit for bit the dense engine on Y = raw[:, cols] --
the residency decision's keyword, and train()'s routing."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from oracle.cpu_ops import CpuRefOps

from helpers import make_problem

from dca_amd import prep as P
from dca_amd._anndata import AnnData
from dca_amd.engine import Engine
from dca_amd.train import fit_engine


class CsrColsOps(CpuRefOps):
    """The CPU oracle with the resident-CSR entries of include/dcahip.h (numpy, fp32 arithmetic as the kernels)."""

    def _rows(self, csr, rows):
        ip, ix, v = csr.indptr.numpy(), csr.indices.numpy(), csr.values.numpy()
        Yr = np.zeros((len(rows), csr.G), np.float32)
        for k, r in enumerate(rows):
            a, b = ip[r], ip[r + 1]
            Yr[k, ix[a:b]] = v[a:b]
        return Yr

    def _tiles(self, csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, X, ldx, sf_out):
        if perm is not None:
            c = int(cursor.item())
            rows = perm[c:c + B].numpy().astype(np.int64)
        else:
            rows = np.arange(row0, row0 + B)
        G = csr.G
        y = self._rows(csr, rows)
        if X is not None:
            x = np.zeros((B, ldx), np.float32)
            x[:, :G] = y
            if fac is not None:
                x = (x / fac.numpy()[rows][:, None]).astype(np.float32)
            if do_log:
                x = np.log1p(x).astype(np.float32)
            if mean is not None:
                x[:, :G] = ((x[:, :G] - mean.numpy()[:G]) / std.numpy()[:G]).astype(np.float32)
            torch.as_strided(X, (B, ldx), (ldx, 1)).numpy()[:] = x
        if sf_out is not None:
            sf_out[:B] = sf[torch.as_tensor(rows)]
        return y

    def csr_gather(self, csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, Y, ldy, X, ldx, sf_out, status):
        y = self._tiles(csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, X, ldx, sf_out)
        Yv = torch.as_strided(Y, (B, ldy), (ldy, 1)).numpy()
        Yv[:] = 0.0
        Yv[:, :csr.G] = y

    def csr_gather_cols(self, csr, col_out, G_out, perm, cursor, row0, B, sf, fac, do_log, mean, std, Y, ldy, X, ldx, sf_out,
                        status):
        y = self._tiles(csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, X, ldx, sf_out)
        co = col_out.numpy()
        assert co.dtype == np.int32 and co.shape == (csr.G,) and co.min() >= -1 and co.max() < G_out <= ldy
        Yv = torch.as_strided(Y, (B, ldy), (ldy, 1)).numpy()
        Yv[:] = 0.0
        Yv[:, co[co >= 0]] = y[:, co >= 0]

    def csr_row_sums(self, csr, out, status):
        out[:] = torch.as_tensor(self._rows(csr, range(csr.n)).astype(np.float64).sum(axis=1).astype(np.float32))

    def csr_col_pass(self, csr, fac, do_log, col_part, status):
        Y = torch.as_tensor(self._rows(csr, range(csr.n)))
        self.prep_col_pass(Y, csr.G, csr.n, csr.G, fac, do_log, None, 0, col_part)


N_CELLS, N_GENES = 75, 18
SUBSETS = {
    'five_shuffled': [11, 2, 17, 0, 6],
    'one': [9],
    'all_reversed': list(range(N_GENES - 1, -1, -1)),
}


def _problem(seed=3):
    _, Y, sf, _ = make_problem(N_CELLS, N_GENES, (6, 3, 6), 'zinb-conddisp', True, seed=seed)
    Y[5] = 0.0                                               # an empty row
    return sp.csr_matrix(Y), sf


def _engines(ae_type, hs, cols):
    ops = CsrColsOps()
    Ys, sf = _problem()
    n, G = Ys.shape
    k = len(cols)
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    fac = torch.as_tensor(np.linspace(0.5, 1.5, n).astype(np.float32))
    norm = P.csr_norm(ops, csr, fac, True, True)
    # the dense engine's matrices: the plain gather over every row (what K-PREP writes densely), Y cut to the subset
    Xd = torch.zeros(n, P._r4(G))
    Yd = torch.zeros(n, P._r4(G))
    ops.csr_gather(csr, None, None, 0, n, None, norm['fac'], True, norm['mean'], norm['std'], Yd, Yd.shape[1], Xd,
                   Xd.shape[1], None, None)
    Ysub = torch.zeros(n, P._r4(k))
    Ysub[:, :k] = Yd[:, cols]
    sf_t = torch.as_tensor(sf)
    engs = []
    for form in ('dense', 'counts'):
        eng = Engine(ae_type, G, k, hs, True, 0.0, ops=ops)
        eng.init_params(seed=7)
        if form == 'dense':
            eng.attach_device_data(Xd, Ysub, sf_t, norm=norm)
        else:
            eng.attach_counts(csr, sf_t, norm, out_cols=cols)
        engs.append(eng)
    return engs, n


def _fit(eng, n, B):
    n_train = int(n * 0.8)
    return fit_engine(eng, n_train, n - n_train, n_train, n - n_train, 0, epochs=3, batch_size=B,
                      shuffle_rng=np.random.RandomState(11), reduce_lr=1, early_stop=0, use_graph=False)


@pytest.mark.parametrize('subset', sorted(SUBSETS))
@pytest.mark.parametrize('ae_type, hs', [('zinb-conddisp', (8, 4, 8)), ('nb', (8, 4, 8)), ('zinb', ())])
def test_subset_fit_and_predict_equal_dense_bit_for_bit(ae_type, hs, subset):
    cols = SUBSETS[subset]
    (dense, counts), n = _engines(ae_type, hs, cols)
    B = 16                                                  # 60 training rows: steps of 16, 16, 16, 12
    hd, hc = _fit(dense, n, B), _fit(counts, n, B)
    assert hd.history['loss'] == hc.history['loss']
    assert hd.history['val_loss'] == hc.history['val_loss']
    assert torch.equal(dense.w, counts.w)
    assert torch.equal(dense.ms, counts.ms)
    for x, y in zip(dense.mm + dense.mv, counts.mm + counts.mv):
        assert torch.equal(x, y)
    assert counts.X.shape == (counts.Bmax, P._r4(N_GENES))  # tiles, not [n, .]: all input genes ...
    assert counts.Y.shape == (counts.Bmax, P._r4(len(cols)))  # ... and the fitted ones
    assert list(counts.out_cols) == list(cols)
    for eng in (dense, counts):
        eng.reserve(32)
    want = {'mean'} | ({'dropout'} if ae_type.startswith('zinb') else set()) | \
        ({'dispersion'} if ae_type == 'zinb-conddisp' else set()) | ({'latent'} if hs else set())
    for r0 in range(0, n, 32):
        b = min(32, n - r0)
        od = {k: v.clone() for k, v in dense.predict_chunk(r0, b, want).items()}
        oc = counts.predict_chunk(r0, b, want)
        for k in want:
            assert torch.equal(od[k], oc[k]), k


def test_the_map_is_checked_and_the_plain_form_keeps_its_refusal():
    ops = CsrColsOps()
    Ys, sf = _problem()
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    norm = P.csr_norm(ops, csr, None, True, True)
    sf_t = torch.as_tensor(sf)
    eng = Engine('zinb-conddisp', N_GENES, 3, (8, 4, 8), True, 0.0, ops=ops)
    with pytest.raises(ValueError, match='input genes = output genes'):
        eng.attach_counts(csr, sf_t, norm)
    for bad in ([1, 1, 2], [0, 1], [0, 1, N_GENES], [-1, 0, 1]):
        with pytest.raises(ValueError):
            eng.attach_counts(csr, sf_t, norm, out_cols=bad)
    eng.attach_counts(csr, sf_t, norm, out_cols=[4, 1, 2], compact=True)
    assert eng.cc_csr is None                               # no byte tile with a map, whatever `compact` says
    assert eng.col_out.tolist() == [-1, 1, 2, -1, 0] + [-1] * (N_GENES - 5)
    with pytest.raises(ValueError, match='csr_gather_cols'):
        Engine('zinb-conddisp', N_GENES, 3, (8, 4, 8), True, 0.0, ops=_NoColsOps()).attach_counts(csr, sf_t, norm,
                                                                                                  out_cols=[4, 1, 2])


class _NoColsOps(CsrColsOps):
    csr_gather_cols = property()                            # hasattr() is False: ops from before the kernel


# ---------------------------------------------------------------------------------------------------- the decision
def test_the_keyword_lets_an_output_subset_through():
    assert P.choose_residency('counts', 10 ** 15, 10, 0, output_subset=True, subset_gather=True) == 'counts'
    assert P.choose_residency('auto', 10 ** 15, 10, 0, output_subset=True, subset_gather=True) == 'counts'
    assert P.choose_residency('auto', 10, 10, 100, output_subset=True, subset_gather=True) == 'dense'
    # off by default, and it lifts nothing else
    assert P.choose_residency('auto', 10 ** 15, 10, 0, output_subset=True) == 'dense'
    with pytest.raises(ValueError, match='output_subset'):
        P.choose_residency('counts', 10 ** 15, 10, 0, output_subset=True)
    with pytest.raises(ValueError, match='use_raw_as_output'):
        P.choose_residency('counts', 10 ** 15, 10, 0, output_subset=True, subset_gather=True, use_raw_as_output=False)
    with pytest.raises(ValueError, match='data-parallel'):
        P.choose_residency('counts', 10 ** 15, 10, 0, output_subset=True, subset_gather=True, world=2)


# ---------------------------------------------------------------------------------------------------- train()
def _adata_with_resident_counts(ops):
    """What normalize() leaves behind in counts-resident mode, made by hand on the CPU: the normalised host X, the raw
    counts in .raw, the size factors, and the DeviceData holding the CSR."""
    Ys, sf = _problem()
    n, G = Ys.shape
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    norm = P.csr_norm(ops, csr, None, True, True)
    X = P.download_csr(ops, csr, norm)
    names = ['g%d' % i for i in range(G)]
    ad = AnnData(X, obs=pd.DataFrame({'size_factors': sf}, index=['c%d' % i for i in range(n)]), var=pd.DataFrame(index=names))
    ad.raw = AnnData(Ys, obs=ad.obs, var=ad.var)
    ad._dca_device = P.DeviceData(None, None, torch.as_tensor(sf), n, G, norm=norm, csr=csr)
    return ad


def _train(ops, genes, monkeypatch, mode, **kw):
    from dca_amd.network import AE_types, override_ops
    from dca_amd.train import train
    monkeypatch.setenv('DCA_AMD_RESIDENT', mode)
    ad = _adata_with_resident_counts(ops)
    with override_ops(lambda: ops):
        net = AE_types['zinb-conddisp'](input_size=N_GENES, output_size=len(genes), hidden_size=(8, 4, 8))
        net.seed = 0
        net.build()
    np.random.seed(0)
    h = train(ad, net, epochs=2, batch_size=16, output_subset=genes, verbose=False, use_graph=False, **kw)
    return net, ad, h


@pytest.mark.parametrize('mode', ['counts', 'auto'])
def test_train_gathers_the_subset_from_the_resident_counts(monkeypatch, tmp_path, mode):
    ops = CsrColsOps()
    genes = ['g11', 'g2', 'g17', 'g0', 'g6']
    net, ad, h = _train(ops, genes, monkeypatch, mode)
    eng = net.engine
    assert eng.csr is ad._dca_device.csr and list(eng.out_cols) == [11, 2, 17, 0, 6]
    assert eng.X.shape[0] == eng.Bmax < N_CELLS
    # the same run from the host matrices (no resident counts: Engine.load_data of X and raw[:, genes])
    from dca_amd.network import AE_types, override_ops
    from dca_amd.train import train
    ref_ad = _adata_with_resident_counts(ops)
    del ref_ad._dca_device
    with override_ops(lambda: ops):
        ref_net = AE_types['zinb-conddisp'](input_size=N_GENES, output_size=len(genes), hidden_size=(8, 4, 8))
        ref_net.seed = 0
        ref_net.build()
    np.random.seed(0)
    ref_h = train(ref_ad, ref_net, epochs=2, batch_size=16, output_subset=genes, verbose=False, use_graph=False)
    assert ref_net.engine.csr is None
    assert h.history == ref_h.history
    assert torch.equal(eng.w, ref_net.engine.w)
    # inference re-attaches through the device data and hands the map back
    # the command line's last step: the fitted genes' results go to the files, adata.X keeps all genes
    cols = np.asarray(genes)
    net.predict_write(ad, str(tmp_path / 'counts'), mode='full', colnames=cols)
    ref_net.predict_write(ref_ad, str(tmp_path / 'host'), mode='full', colnames=cols)
    files = sorted(os.listdir(str(tmp_path / 'host')))
    assert {'mean.tsv', 'dispersion.tsv', 'dropout.tsv', 'latent.tsv'} <= set(files)
    assert files == sorted(os.listdir(str(tmp_path / 'counts')))
    for f in files:
        assert (tmp_path / 'host' / f).read_bytes() == (tmp_path / 'counts' / f).read_bytes(), f
    assert open(str(tmp_path / 'counts' / 'mean.tsv')).readline().count('\t') == N_CELLS
    assert ad.X.shape == (N_CELLS, N_GENES)
    net.predict(ad, mode='latent')
    ref_net.predict(ref_ad, mode='latent')
    assert net.engine.csr is not None and list(net.engine.out_cols) == [11, 2, 17, 0, 6]
    assert (np.asarray(ad.obsm['X_dca']) == np.asarray(ref_ad.obsm['X_dca'])).all()


def test_a_gene_named_twice_keeps_the_dense_route(monkeypatch):
    ops = CsrColsOps()
    genes = ['g3', 'g8', 'g3']
    net, _, h = _train(ops, genes, monkeypatch, 'auto')
    assert net.engine.csr is None and np.isfinite(h.history['loss']).all()
    with pytest.raises(ValueError, match='twice'):
        _train(ops, genes, monkeypatch, 'counts')


def test_forced_counts_mode_still_names_the_other_reasons(monkeypatch):
    ops = CsrColsOps()
    with pytest.raises(ValueError, match='use_raw_as_output'):
        _train(ops, ['g3', 'g8'], monkeypatch, 'counts', use_raw_as_output=False)
    with pytest.raises(ValueError, match='output_subset'):
        _train(_NoColsOps(), ['g3', 'g8'], monkeypatch, 'counts')
