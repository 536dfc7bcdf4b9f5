"""Counts-resident mode without a GPU: the residency decision, its environment variable, and the engine gathering each
minibatch from CSR counts on the CPU oracle -- bit for bit the dense engine."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle.cpu_ops import CpuRefOps

from helpers import make_problem

from dca_amd import config as C
from dca_amd import prep as P
from dca_amd.engine import Engine
from dca_amd.train import fit_engine


# ---------------------------------------------------------------------------------------------------- the decision
def test_dense_whenever_its_estimate_fits():
    assert P.choose_residency('auto', 100, 10, 100) == 'dense'
    assert P.choose_residency('auto', 101, 10, 100) == 'counts'
    assert P.choose_residency('dense', 10 ** 15, 10, 0) == 'dense'
    assert P.choose_residency('counts', 10, 10, 10 ** 15) == 'counts'


@pytest.mark.parametrize('kw, why', [(dict(world=2), 'data-parallel'), (dict(output_subset=['g1']), 'output_subset'),
                                     (dict(use_raw_as_output=False), 'use_raw_as_output'),
                                     (dict(has_norm=False), 'not a known function')])
def test_auto_stays_dense_and_counts_refuses_where_the_mode_cannot_apply(kw, why):
    assert P.choose_residency('auto', 10 ** 15, 10, 0, **kw) == 'dense'
    with pytest.raises(ValueError, match=why):
        P.choose_residency('counts', 10 ** 15, 10, 0, **kw)


def test_unknown_mode_is_refused():
    with pytest.raises(ValueError):
        P.choose_residency('csr', 1, 1, 1)


def test_memory_estimates():
    # the benchmark shape: 68 579 x 20 000 at 96 M non-zeros -> ~12.4 GB dense, ~0.77 GB as CSR
    assert abs(P.dense_bytes(68579, 20000) / 1e9 - 12.4) < 0.1
    assert abs(P.counts_bytes(68579, 96_000_000) / 1e9 - 0.77) < 0.01


def test_environment_variable(monkeypatch):
    monkeypatch.delenv('DCA_AMD_RESIDENT', raising=False)
    assert C.current().resident == 'auto'
    for v in ('counts', 'dense', 'auto'):
        monkeypatch.setenv('DCA_AMD_RESIDENT', v)
        assert C.current().resident == v
    monkeypatch.setenv('DCA_AMD_RESIDENT', 'sparse')
    with pytest.raises(ValueError, match='DCA_AMD_RESIDENT'):
        C.current()


def test_residency_without_the_csr_kernels():
    X = sp.random(10, 8, density=0.3, format='csr', dtype=np.float32, random_state=0)
    assert P.residency(X, torch.device('cpu'), CpuRefOps(), mode='auto') == 'dense'
    with pytest.raises(ValueError, match='csr_gather'):
        P.residency(X, torch.device('cpu'), CpuRefOps(), mode='counts')


# ---------------------------------------------------------------------------------------------------- the engine
class CsrOps(CpuRefOps):
    """The CPU oracle with the resident-CSR entries of include/dcahip.h (numpy, fp32 arithmetic as the kernels)."""

    def _rows(self, csr, rows):
        ip, ix, v = csr.indptr.numpy(), csr.indices.numpy(), csr.values.numpy()
        Yr = np.zeros((len(rows), csr.G), np.float32)
        for k, r in enumerate(rows):
            a, b = ip[r], ip[r + 1]
            Yr[k, ix[a:b]] = v[a:b]
        return Yr

    def csr_gather(self, csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, Y, ldy, X, ldx, sf_out, status):
        if perm is not None:
            c = int(cursor.item())
            rows = perm[c:c + B].numpy().astype(np.int64)
        else:
            rows = np.arange(row0, row0 + B)
        G = csr.G
        y = self._rows(csr, rows)
        Yv = torch.as_strided(Y, (B, ldy), (ldy, 1)).numpy()
        Yv[:] = 0.0
        Yv[:, :G] = y
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

    def csr_row_sums(self, csr, out, status):
        out[:] = torch.as_tensor(self._rows(csr, range(csr.n)).astype(np.float64).sum(axis=1).astype(np.float32))

    def csr_col_pass(self, csr, fac, do_log, col_part, status):
        Y = torch.as_tensor(self._rows(csr, range(csr.n)))
        self.prep_col_pass(Y, csr.G, csr.n, csr.G, fac, do_log, None, 0, col_part)


def _problem(n=75, G=18, seed=3):
    _, Y, sf, _ = make_problem(n, G, (6, 3, 6), 'zinb-conddisp', True, seed=seed)
    Y[5] = 0.0                                               # an empty row
    return sp.csr_matrix(Y), sf


def _engines(ae_type, hs, seed=3, **kw):
    ops = CsrOps()
    Ys, sf = _problem(seed=seed)
    n, G = Ys.shape
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    fac = torch.as_tensor(np.linspace(0.5, 1.5, n).astype(np.float32))
    norm = P.csr_norm(ops, csr, fac, True, True)
    # the dense engine's matrices are the same gather over every row (what K-PREP writes densely)
    Xd = torch.zeros(n, P._r4(G))
    Yd = torch.zeros(n, P._r4(G))
    ops.csr_gather(csr, None, None, 0, n, None, norm['fac'], True, norm['mean'], norm['std'], Yd, Yd.shape[1], Xd,
                   Xd.shape[1], None, None)
    sf_t = torch.as_tensor(sf)
    engs = []
    for form in ('dense', 'counts'):
        eng = Engine(ae_type, G, G, hs, True, 0.0, ops=ops, **kw)
        eng.init_params(seed=7)
        if form == 'dense':
            eng.attach_device_data(Xd, Yd, sf_t, norm=norm)
        else:
            eng.attach_counts(csr, sf_t, norm)
        engs.append(eng)
    return engs, n


def _fit(eng, n, B):
    n_train = int(n * 0.8)
    return fit_engine(eng, n_train, n - n_train, n_train, n - n_train, 0, epochs=3, batch_size=B,
                      shuffle_rng=np.random.RandomState(11), reduce_lr=1, early_stop=0, use_graph=False)


def _same_state(a, b):
    assert torch.equal(a.w, b.w)
    assert torch.equal(a.ms, b.ms)
    for x, y in zip(a.mm + a.mv, b.mm + b.mv):
        assert torch.equal(x, y)


@pytest.mark.parametrize('ae_type, hs, kw', [
    ('zinb-conddisp', (8, 4, 8), {}),
    ('nb', (8, 4, 8), {}),
    ('zinb-conddisp', (8, 4, 8), dict(hidden_dropout=0.25, input_dropout=0.2, dropout_seed=5)),
    ('zinb', (), {}),
])
def test_counts_resident_fit_equals_dense_bit_for_bit(ae_type, hs, kw):
    (dense, counts), n = _engines(ae_type, hs, **kw)
    B = 16                                                  # 60 training rows: steps of 16, 16, 16, 12
    hd, hc = _fit(dense, n, B), _fit(counts, n, B)
    assert hd.history['loss'] == hc.history['loss']
    assert hd.history['val_loss'] == hc.history['val_loss']
    _same_state(dense, counts)
    assert counts.X.shape[0] == counts.Bmax                 # the input is a tile, not [n, G]


@pytest.mark.parametrize('hs', [(8, 4, 8), ()])
def test_counts_resident_predict_equals_dense_bit_for_bit(hs):
    (dense, counts), n = _engines('zinb-conddisp', hs)
    for eng in (dense, counts):
        eng.reserve(32)
    want = {'mean', 'dispersion', 'dropout'} | ({'latent'} if hs else set())
    for r0 in range(0, n, 32):
        b = min(32, n - r0)
        od = {k: v.clone() for k, v in dense.predict_chunk(r0, b, want).items()}
        oc = counts.predict_chunk(r0, b, want)
        for k in want:
            assert torch.equal(od[k], oc[k]), k
