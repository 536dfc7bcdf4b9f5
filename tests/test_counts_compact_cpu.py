"""EngineConfig.counts_compact without a GPU: the field and its environment variable, the fallback of ops that lack
csr_gather_compact (the CPU oracle: counts mode keeps the fp32 gather), the once-per-dataset verdict taken from the CSR,
and the tile format restated in numpy against compact.py."""
import numpy as np
import scipy.sparse as sp
import torch

from test_counts_resident_cpu import CsrOps, _fit, _problem, _same_state

from dca_amd import compact
from dca_amd import config as C
from dca_amd import prep as P
from dca_amd.engine import Engine


def test_field_defaults_to_off_and_parses(monkeypatch):
    monkeypatch.delenv('DCA_AMD_COUNTS_COMPACT', raising=False)
    assert C.EngineConfig().counts_compact is False
    assert C.current().counts_compact is False
    assert C.EngineConfig._ENV['counts_compact'] == 'DCA_AMD_COUNTS_COMPACT'
    monkeypatch.setenv('DCA_AMD_COUNTS_COMPACT', '1')
    assert C.current().counts_compact is True
    monkeypatch.setenv('DCA_AMD_COUNTS_COMPACT', '0')
    assert C.current().counts_compact is False


def _counts_engine(compact_arg, monkeypatch=None, env=None):
    if monkeypatch is not None:
        monkeypatch.setenv('DCA_AMD_COUNTS_COMPACT', env)
    ops = CsrOps()
    assert not hasattr(ops, 'csr_gather_compact')
    Ys, sf = _problem()
    n, G = Ys.shape
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    fac = torch.as_tensor(np.linspace(0.5, 1.5, n).astype(np.float32))
    norm = P.csr_norm(ops, csr, fac, True, True)
    eng = Engine('zinb-conddisp', G, G, (8, 4, 8), True, 0.0, ops=ops)
    eng.init_params(seed=7)
    eng.attach_counts(csr, torch.as_tensor(sf), norm, compact=compact_arg)
    return eng, n


def test_ops_without_the_entry_keep_the_fp32_gather(monkeypatch):
    monkeypatch.delenv('DCA_AMD_COUNTS_COMPACT', raising=False)
    off, n = _counts_engine(False)
    on, _ = _counts_engine(True)
    env, _ = _counts_engine(None, monkeypatch, '1')
    h = [_fit(e, n, 16) for e in (off, on, env)]
    for e, hk in zip((on, env), h[1:]):
        assert e.cc is None and e.cc_in is None and e.cc_csr is None
        assert hk.history['loss'] == h[0].history['loss'] and hk.history['val_loss'] == h[0].history['val_loss']
        _same_state(off, e)


def _np_tile(Ys, rows):
    """The tile format (include/dcahip.h, dcahip_csr_gather_compact) restated: bytes, pad columns, the overflow list."""
    n, G = Ys.shape
    ldc = (G + 15) // 16 * 16
    Yc = np.zeros((len(rows), ldc), np.uint8)
    ptr, col, val = [0], [], []
    for k, r in enumerate(rows):
        a, b = Ys.indptr[r], Ys.indptr[r + 1]
        for c, v in zip(Ys.indices[a:b], Ys.data[a:b]):      # canonical rows: ascending columns
            Yc[k, c] = 255 if v >= 255 else int(v)
            if v >= 255:
                col.append(c)
                val.append(v)
        ptr.append(len(col))
    return Yc, ldc, np.asarray(ptr, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float32)


class _CompactOps:
    """counts_compact of include/dcahip.h in numpy (what compact.build needs from its ops)."""

    def counts_compact_ld(self, G):
        return (G + 15) // 16 * 16

    def counts_compact(self, Y, ldy, n, G, Yc, ldc, status):
        y = Y.numpy()[:n, :G]
        bad = ~(y >= 0) | (y != np.floor(y)) | (y > 16777216.0)
        y = np.where(bad, 0.0, y)
        code = np.where(y >= 255, 255, y).astype(np.uint8)
        Yc.numpy()[:n, :G] = code
        status[0] += int(bad.sum())
        status[1] += int((code == 255).sum())


def test_numpy_restatement_of_the_tile_agrees_with_compact_py():
    rng = np.random.default_rng(4)
    n, G = 23, 37
    Y = rng.integers(0, 6, (n, G)).astype(np.float32) * (rng.random((n, G)) < 0.3)
    for r, c, v in ((2, 0, 255.), (2, 36, 70000.), (2, 9, 256.), (11, 5, 5000.), (22, 36, 254.)):
        Y[r, c] = v
    Y[4] = 0
    Ys = sp.csr_matrix(Y)
    Ys.sort_indices()
    rows = [2, 22, 4, 11, 0, 2]
    Yc, ldc, ptr, col, val = _np_tile(Ys, rows)
    cc = compact.build(_CompactOps(), torch.as_tensor(Y[rows]), len(rows), G)
    assert cc.ldc == ldc and (cc.Yc.numpy() == Yc).all() and (Yc[:, G:] == 0).all()
    assert (cc.ovf_ptr.numpy() == ptr).all() and (cc.ovf_col.numpy() == col).all() and (cc.ovf_val.numpy() == val).all()
    assert ptr.tolist() == [0, 3, 3, 3, 4, 4, 7] and col[:3].tolist() == [0, 9, 36]


def test_verdict_from_the_csr_equals_what_the_dense_pass_finds():
    rng = np.random.default_rng(5)
    n, G = 40, 30
    Y = rng.integers(0, 4, (n, G)).astype(np.float32)
    Y[1, 1] = 1.0
    for r, k in ((3, 5), (17, 2), (30, 1)):
        Y[r, :k] = 300.0
    csr = P.upload_csr(sp.csr_matrix(Y), torch.device('cpu'), CsrOps())
    v = compact.csr_verdict(csr)
    assert not v.bad and v.n_esc == 8 and v.row_esc.tolist() == [5, 2, 1]
    assert [v.capacity(b) for b in (1, 2, 3, 40)] == [5, 7, 8, 8]      # no tile of b rows holds more escapes
    assert compact.csr_verdict(csr) is v                                   # once per dataset
    for bad in (2.5, -1.0, float('nan'), float('inf')):
        cb = P.upload_csr(sp.csr_matrix(Y), torch.device('cpu'), CsrOps())
        lo, hi = int(cb.indptr[1]), int(cb.indptr[2])
        cb.values[lo + int((cb.indices[lo:hi] == 1).nonzero()[0])] = bad
        assert compact.csr_verdict(cb).bad
    empty = P.upload_csr(sp.csr_matrix((5, G), dtype=np.float32), torch.device('cpu'), CsrOps())
    ve = compact.csr_verdict(empty)
    assert not ve.bad and ve.n_esc == 0 and ve.capacity(4) == 0
