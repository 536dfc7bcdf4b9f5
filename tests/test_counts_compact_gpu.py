"""Counts-resident training from a per-batch byte tile on the MI355X (EngineConfig.counts_compact): dcahip_csr_gather_compact
against dcahip_counts_compact + compact.build on the fp32 tile of dcahip_csr_gather, what it refuses, the engine against the
dense engine WITH its byte store, the path a throughput step takes, dca() and predict_write -- all bit for bit."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from dca_amd import compact, io, prep
from dca_amd._anndata import AnnData

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _counts(n, G, density, seed, empty=(), big=(), last=None):
    """Random counts; the rows of `empty` (those the matrix has) store nothing, row `last` stores the last column."""
    rng = np.random.default_rng(seed)
    Y = sp.random(n, G, density=density, format='csr', dtype=np.float32, random_state=seed,
                  data_rvs=lambda k: rng.integers(1, 40, k).astype(np.float32))
    Y = Y.tolil()
    if last is not None:
        Y[last, G - 1] = 7
    for k, v in enumerate(big):                               # escapes: several in one row, first / last column included
        Y[(3 * k) % n if k % 2 else 1, (k * 7919) % G if k else G - 1] = v
    if big:
        Y[1, 0] = big[0]
    for r in empty:
        if r < n:
            Y[r, :] = 0
    Y = Y.tocsr()
    Y.eliminate_zeros()
    return Y


class _Tile:
    """Every output of csr_gather_compact between guard elements (bytes GUARD, words -7, floats NaN)."""

    def __init__(self, ops, B, G, cap, with_x, ldx):
        dev = torch.device('cuda')
        self.B, self.cap, self.ldc, self.ldx = B, cap, ops.counts_compact_ld(G), ldx
        self.Yc = torch.full((B + 2, self.ldc), GUARD, dtype=torch.uint8, device=dev)
        self.ptr = torch.full((B + 3,), -7, dtype=torch.int32, device=dev)
        self.col = torch.full((cap + 2,), -7, dtype=torch.int32, device=dev)
        self.val = torch.full((cap + 2,), float('nan'), device=dev)
        self.X = torch.full((B + 2, ldx), float('nan'), device=dev) if with_x else None
        self.sf = torch.full((B + 2,), float('nan'), device=dev)
        self.fac = torch.full((B + 2,), float('nan'), device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(self, ops, csr, perm, cur, row0, sf, fac, do_log, mean, std):
        B, cap = self.B, self.cap
        lst = (self.ptr[1:B + 2], self.col[1:cap + 1], self.val[1:cap + 1]) if cap else (None, None, None)
        ops.csr_gather_compact(csr, perm, cur, row0, B, sf, fac, do_log, mean, std, self.Yc[1:], self.ldc, *lst,
                               self.X[1:] if self.X is not None else None, self.ldx, self.sf[1:],
                               self.fac[1:] if fac is not None else None, self.status)

    def check_guards(self):
        B, cap = self.B, self.cap
        assert (self.Yc[0] == GUARD).all() and (self.Yc[B + 1] == GUARD).all()
        if cap:
            assert self.ptr[0].item() == -7 and self.ptr[B + 2].item() == -7
        else:
            assert (self.ptr == -7).all()
        assert self.col[0].item() == -7 and self.col[cap + 1].item() == -7
        assert torch.isnan(self.val[0]) and torch.isnan(self.val[cap + 1])
        if self.X is not None:
            assert torch.isnan(self.X[0]).all() and torch.isnan(self.X[B + 1]).all()
        assert torch.isnan(self.sf[0]) and torch.isnan(self.sf[B + 1])
        assert torch.isnan(self.fac[0]) and torch.isnan(self.fac[B + 1])


def _reference(ops, csr, rows, sf, fac, do_log, mean, std, ld):
    """The fp32 tile of csr_gather for these storage rows -> counts_compact + compact.py's list."""
    dev = torch.device('cuda')
    B = len(rows)
    perm = torch.as_tensor(np.asarray(rows, np.int32), device=dev)
    cur = torch.zeros(1, dtype=torch.int64, device=dev)
    Y = torch.empty(B, ld, device=dev)
    X = torch.empty(B, ld, device=dev)
    so = torch.empty(B, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_gather(csr, perm, cur, 0, B, sf, fac, do_log, mean, std, Y, ld, X, ld, so, st)
    assert int(st.item()) == 0
    cc = compact.build(ops, Y, B, csr.G)
    assert cc is not None
    return cc, X, so


def _equal(t, cc, X, so, fac_rows):
    B = t.B
    torch.cuda.synchronize()
    assert int(t.status.item()) == 0
    t.check_guards()
    assert torch.equal(t.Yc[1:B + 1], cc.Yc)
    if cc.ovf_ptr is None:
        if t.cap:
            assert (t.ptr[1:B + 2] == 0).all()
    else:
        assert torch.equal(t.ptr[1:B + 2], cc.ovf_ptr)
        k = cc.ovf_col.numel()
        assert k <= t.cap
        assert torch.equal(t.col[1:k + 1], cc.ovf_col)
        assert (_bits(t.val[1:k + 1]) == _bits(cc.ovf_val)).all()
        assert (t.col[k + 1:] == -7).all()                    # nothing written behind the list's end
    if t.X is not None:
        assert (_bits(t.X[1:B + 1]) == _bits(X)).all()
    assert (_bits(t.sf[1:B + 1]) == _bits(so)).all()
    if fac_rows is not None:
        assert (_bits(t.fac[1:B + 1]) == _bits(fac_rows)).all()


BIG = (255., 256., 5000., 70000., 254., 300.)


# G = 8065: one fp32 LDS segment and a 4-float tail; 32256: exactly one byte segment; 32257: one and a 16-byte tail
@pytest.mark.parametrize('n, G, big', [(60, 1001, ()), (40, 9001, ()), (60, 1001, BIG), (40, 9001, BIG), (24, 33001, BIG),
                                       (30, 1024, BIG), (5, 8065, BIG), (5, 32256, ()), (5, 32257, BIG)])
@pytest.mark.parametrize('use_fac, do_log, scale', [(f, l, s) for f in (0, 1) for l in (0, 1) for s in (0, 1)])
def test_tile_equals_the_dense_stores_rows(ops, n, G, big, use_fac, do_log, scale):
    dev = torch.device('cuda')
    Ys = _counts(n, G, 0.05, seed=G + n, empty=(0, 7, n - 1), big=big, last=2)
    assert Ys[2, G - 1] != 0 and Ys[0].nnz == 0
    csr = prep.upload_csr(Ys, dev, ops)
    ld = prep._r4(G)
    rng = np.random.default_rng(1)
    fac = torch.as_tensor(rng.uniform(0.3, 2.0, n).astype(np.float32), device=dev) if use_fac else None
    mean = std = None
    if scale:
        mean = torch.zeros(ld, device=dev)
        std = torch.ones(ld, device=dev)
        mean[:G] = torch.as_tensor(rng.normal(0, 1, G).astype(np.float32))
        mean[:8] = 0.0
        std[:G] = torch.as_tensor(rng.uniform(0.5, 3, G).astype(np.float32))
    sf = torch.as_tensor(rng.uniform(0.1, 9, n).astype(np.float32), device=dev)
    v = compact.csr_verdict(csr)
    assert not v.bad and v.n_esc == int((Ys.data >= 255).sum())
    perm = rng.permutation(n)
    for rows, perm_mode in ((perm, True), (perm[:1], True), (np.arange(min(5, n - 2), n), False),
                            (np.arange(n - 1, n), False)):
        B = len(rows)
        cap = v.capacity(B)
        idx = torch.as_tensor(rows, device=dev)
        cc, X, so = _reference(ops, csr, rows, sf, fac, do_log, mean, std, ld)
        assert (0 if cc.ovf_col is None else cc.ovf_col.numel()) <= cap
        for with_x in (False, True):
            t = _Tile(ops, B, G, cap, with_x, ld)
            if perm_mode:
                p = torch.as_tensor(np.r_[np.zeros(3, np.int64), rows].astype(np.int32), device=dev)
                t.run(ops, csr, p, torch.full((1,), 3, dtype=torch.int64, device=dev), 0, sf, fac, do_log, mean, std)
            else:
                t.run(ops, csr, None, None, int(rows[0]), sf, fac, do_log, mean, std)
            _equal(t, cc, X, so, fac[idx] if use_fac else None)


def test_tile_from_a_replayed_graph_follows_the_cursor_word(ops):
    dev = torch.device('cuda')
    n, G, B = 90, 9001, 16
    Ys = _counts(n, G, 0.05, seed=3, big=BIG)
    csr = prep.upload_csr(Ys, dev, ops)
    ld = prep._r4(G)
    rng = np.random.default_rng(2)
    fac = torch.as_tensor(rng.uniform(0.3, 2.0, n).astype(np.float32), device=dev)
    sf = torch.as_tensor(rng.uniform(0.1, 9, n).astype(np.float32), device=dev)
    order = rng.permutation(n)
    perm = torch.as_tensor(order.astype(np.int32), device=dev)
    cur = torch.zeros(1, dtype=torch.int64, device=dev)
    cap = compact.csr_verdict(csr).capacity(B)
    for with_x in (False, True):
        t = _Tile(ops, B, G, cap, with_x, ld)
        cur.zero_()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            t.run(ops, csr, perm, cur, 0, sf, fac, True, None, None)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            t.run(ops, csr, perm, cur, 0, sf, fac, True, None, None)
        for at in (0, 16, 61, 74):                            # (61: rows 1 and the escapes' rows move through the tile)
            cur.fill_(at)
            graph.replay()
            rows = order[at:at + B]
            cc, X, so = _reference(ops, csr, rows, sf, fac, True, None, None, ld)
            _equal(t, cc, X, so, fac[torch.as_tensor(rows, device=dev)])


def _finite_inside(t):
    torch.cuda.synchronize()
    t.check_guards()
    B = t.B
    if t.X is not None:
        assert torch.isfinite(t.X[1:B + 1]).all()
    if t.cap:
        p = t.ptr[1:B + 2].cpu().numpy()
        assert p[0] == 0 and (np.diff(p) >= 0).all() and p[-1] <= t.cap


def test_malformed_csr_is_counted_and_stays_inside_the_tile(ops):
    dev = torch.device('cuda')
    G, ld = 30, 32
    indptr = torch.as_tensor([0, 3, 2, 6, 6], dtype=torch.int64, device=dev)     # row 1 decreases
    indices = torch.as_tensor([1, 40, 5, -2, 7, 29], dtype=torch.int32, device=dev)
    values = torch.as_tensor([1, 2, 3, 4, 300, 6], dtype=torch.float32, device=dev)
    csr = prep.CsrCounts(indptr, indices, values, 4, G)
    sf = torch.ones(4, device=dev)
    perm = torch.as_tensor(np.array([0, 1, 2, 3, 9], np.int32), device=dev)      # storage row 9 does not exist
    cur = torch.zeros(1, dtype=torch.int64, device=dev)
    for with_x in (False, True):
        t = _Tile(ops, 5, G, 2, with_x, ld)
        t.run(ops, csr, perm, cur, 0, sf, None, True, None, None)
        _finite_inside(t)
        assert int(t.status.item()) == 4                      # column 40, column -2, the decreasing row, the missing row
        Yc = t.Yc[1:6].cpu().numpy()
        assert Yc[0, 1] == 1 and Yc[2, 7] == 255 and Yc[2, 29] == 6 and Yc[4].sum() == 0 and Yc[:, 30:].sum() == 0
        assert t.col[1].item() == 7 and t.val[1].item() == 300.0


def test_unsorted_and_duplicate_columns_stay_inside_the_tile_and_the_list(ops):
    """Rows that are not canonical may give wrong values, never a write outside: every escape is listed at most once per
    stored entry, inside the row's share of the list."""
    dev = torch.device('cuda')
    G, ld = 30, 32
    indptr = torch.as_tensor([0, 3, 7], dtype=torch.int64, device=dev)
    indices = torch.as_tensor([5, 5, 3, 29, 0, 0, 29], dtype=torch.int32, device=dev)
    values = torch.as_tensor([300, 400, 256, 1000, 2, 255, 7], dtype=torch.float32, device=dev)
    csr = prep.CsrCounts(indptr, indices, values, 2, G)
    sf = torch.ones(2, device=dev)
    for with_x in (False, True):
        for cap in (5, 4):
            t = _Tile(ops, 2, G, cap, with_x, ld)
            t.run(ops, csr, None, None, 0, sf, None, True, None, None)
            _finite_inside(t)
            assert int(t.status.item()) == 5 - cap            # five escapes stored; what does not fit is counted
            assert t.ptr[1:4].tolist() == [0, 3, cap]
            assert t.col[1:4].tolist() == [5, 5, 3] and t.val[1:4].tolist() == [300.0, 400.0, 256.0]
            Yc = t.Yc[1:3].cpu().numpy()
            assert Yc[0, 5] == 255 and Yc[0, 3] == 255 and Yc[1, 29] in (7, 255) and Yc[1, 0] in (2, 255)


def test_values_that_are_not_counts_are_stored_as_zero_and_counted(ops):
    dev = torch.device('cuda')
    G, ld = 40, 40
    indptr = torch.as_tensor([0, 4, 6], dtype=torch.int64, device=dev)
    indices = torch.as_tensor([0, 3, 9, 39, 2, 5], dtype=torch.int32, device=dev)
    values = torch.as_tensor([2.5, -1.0, 7.0, float('nan'), float('inf'), 300.5], dtype=torch.float32, device=dev)
    csr = prep.CsrCounts(indptr, indices, values, 2, G)
    assert compact.csr_verdict(csr).bad
    sf = torch.ones(2, device=dev)
    for with_x in (False, True):
        t = _Tile(ops, 2, G, 1, with_x, ld)
        t.run(ops, csr, None, None, 0, sf, None, False, None, None)
        torch.cuda.synchronize()
        t.check_guards()
        assert int(t.status.item()) == 5
        Yc = t.Yc[1:3].cpu().numpy()
        assert Yc[0, 9] == 7 and Yc.sum() == 7
        assert (t.ptr[1:4] == 0).all() and t.col[1].item() == -7


def test_a_list_one_entry_too_small_is_counted_and_not_overrun(ops):
    dev = torch.device('cuda')
    n, G = 30, 1024
    Ys = _counts(n, G, 0.05, seed=9, big=BIG)
    csr = prep.upload_csr(Ys, dev, ops)
    sf = torch.ones(n, device=dev)
    total = int((Ys.data >= 255).sum())
    assert total >= 4
    for with_x in (False, True):
        t = _Tile(ops, n, G, total - 1, with_x, G)
        t.run(ops, csr, None, None, 0, sf, None, True, None, None)
        _finite_inside(t)
        assert int(t.status.item()) == 1
        assert t.ptr[n + 1].item() == total - 1
        # without a list at all every escape is counted
        t0 = _Tile(ops, n, G, 0, with_x, G)
        t0.run(ops, csr, None, None, 0, sf, None, True, None, None)
        torch.cuda.synchronize()
        t0.check_guards()
        assert int(t0.status.item()) == total
        assert torch.equal(t0.Yc[1:n + 1], t.Yc[1:n + 1])


# ---------------------------------------------------------------------------------------------------- the engine
def _device_data(ops, n, G, seed, monkeypatch, n_big=0):
    """The same counts normalised by K-PREP in both forms: every count below 255 but n_big of them."""
    out = {}
    for form in ('dense', 'counts'):
        monkeypatch.setenv('DCA_AMD_RESIDENT', form)
        Y = np.minimum(synth_counts(n, G, seed), 254.0).astype(np.float32)
        if n_big:
            rng = np.random.default_rng(seed)
            at = rng.choice(n * G, n_big, replace=False)
            Y.reshape(-1)[at] = rng.choice([255., 256., 300., 1000., 5000.], n_big).astype(np.float32)
        ad = AnnData(sp.csr_matrix(Y), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                     var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
        ad, dd = prep.normalize_device(ad, filter_min_counts=False, ops=ops)
        assert (dd.csr is not None) == (form == 'counts')
        out[form] = (ad, dd)
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    assert (out['dense'][0].X == out['counts'][0].X).all()
    return out


def _engine(ops, ae, G, hs, dd, form, **kw):
    from dca_amd.engine import Engine
    eng = Engine(ae, G, G, hs, True, 0.0, ops=ops, **kw)
    eng.init_params(seed=3)
    if form == 'dense':
        eng.attach_device_data(dd.X, dd.Y, dd.sf, norm=dd.norm)          # the default form: byte store on
    else:
        eng.attach_counts(dd.csr, dd.sf, dd.norm, compact=True)
    return eng


@pytest.mark.parametrize('ae, hs, n, G, B, n_big, kw', [
    ('zinb-conddisp', (64, 32, 64), 700, 1000, 32, 0, {}),
    ('zinb-conddisp', (64, 32, 64), 9000, 1000, 4096, 0, {}),
    ('nb', (64, 32, 64), 700, 1000, 32, 0, {}),
    ('zinb', (64, 32, 64), 700, 1000, 64, 0, {}),
    ('zinb-conddisp', (128, 64, 128), 1500, 1000, 512, 0, {}),
    ('zinb-conddisp', (64, 32, 64), 700, 1000, 32, 0, dict(hidden_dropout=0.2, input_dropout=0.1, dropout_seed=4)),
    ('zinb-conddisp', (64, 32, 64), 9000, 1000, 4096, 40, {}),          # 4e-6: targets and first layer from the tile's list
    ('zinb-conddisp', (64, 32, 64), 2000, 1000, 512, 200, {}),          # 1e-4: targets from the tile, dense first layer
    ('zinb-conddisp', (64, 32, 64), 700, 1000, 64, 1500, {}),           # 2e-3, above the rate: fp32 targets
])
def test_counts_compact_engine_equals_the_dense_engine_with_its_byte_store(ops, ae, hs, n, G, B, n_big, kw, monkeypatch):
    from dca_amd.train import fit_engine
    data = _device_data(ops, n, G, seed=n + G, monkeypatch=monkeypatch, n_big=n_big)
    engs = {f: _engine(ops, ae, G, hs, data[f][1], f, **kw) for f in ('dense', 'counts')}
    d, c = engs['dense'], engs['counts']
    hist = {}
    for f, eng in engs.items():
        n_train = int(n * 0.9)
        hist[f] = fit_engine(eng, n_train, n - n_train, n_train, n - n_train, 0, epochs=2, batch_size=B,
                             shuffle_rng=np.random.RandomState(5), reduce_lr=1, early_stop=0, use_graph=True).history
    # the decisions are the dense engine's
    assert (d.cc is None) == (c.cc is None) and (d.cc_in is None) == (c.cc_in is None)
    assert (d.cc is None) == (n_big == 1500) and (d.cc_in is None) == (n_big >= 200)
    if d.cc is not None:
        assert (d.cc.ovf_ptr is None) == (c.cc.ovf_ptr is None) == (n_big == 0)
    assert hist['dense'] == hist['counts']
    assert torch.equal(d.w, c.w) and torch.equal(d.ms, c.ms)
    out_d = {k: v.clone() for k, v in d.predict_chunk(0, min(n, d.Bmax), {'mean', 'latent'}).items()}
    out_c = c.predict_chunk(0, min(n, c.Bmax), {'mean', 'latent'})
    for k in out_d:
        assert torch.equal(out_d[k], out_c[k]), k
    assert int(c.gather_status.item()) == 0


def test_a_throughput_step_reads_neither_fp32_tile(ops, monkeypatch):
    n, G, B = 4500, 1000, 4096
    data = _device_data(ops, n, G, seed=11, monkeypatch=monkeypatch)
    engs = {f: _engine(ops, 'zinb-conddisp', G, (64, 32, 64), data[f][1], f) for f in ('dense', 'counts')}
    loss = {}
    for f, eng in engs.items():
        eng.reserve(B)
        eng.perm = torch.as_tensor(np.random.RandomState(2).permutation(n).astype(np.int32), device=eng.dev)
        eng.hist = torch.zeros(4, dtype=torch.float32, device=eng.dev)
        eng.cursor.zero_(); eng.acc.zero_()
        eng.set_lr(1e-3)
        if f == 'counts':
            assert eng.cc is not None and eng.cc_in is not None
            eng.X.fill_(float('nan'))
            eng.Y.fill_(float('nan'))
        eng.train_step(B, rows_per_slot=B)
        torch.cuda.synchronize()
        loss[f] = float(eng.hist[0].item())
    c = engs['counts']
    assert torch.isnan(c.X).all() and torch.isnan(c.Y).all()
    assert np.isfinite(loss['counts']) and loss['counts'] == loss['dense']
    assert torch.equal(engs['dense'].w, c.w)
    assert int(c.gather_status.item()) == 0


def _sparse_adata(n, G, seed):
    Ys = sp.csr_matrix(synth_counts(n, G, seed).astype(np.float32))
    return AnnData(Ys, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                   var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


def _runs(form, tmp, monkeypatch):
    """dca() in place, then the command line's sequence: read_dataset -> normalize -> train -> predict_write."""
    from dca_amd.api import dca
    from dca_amd.network import AE_types
    from dca_amd.train import train
    if form == 'tile':
        monkeypatch.setenv('DCA_AMD_RESIDENT', 'counts')
        monkeypatch.setenv('DCA_AMD_COUNTS_COMPACT', '1')
    ad = _sparse_adata(400, 600, 12)
    dca(ad, mode='denoise', epochs=3, return_info=True, random_state=1, verbose=False)
    b = io.read_dataset(_sparse_adata(333, 530, 4), transpose=False, test_split=False, copy=False)
    b = io.normalize(b, size_factors=True, logtrans_input=True, normalize_input=True)
    assert (b._dca_device.csr is not None) == (form == 'tile')
    net = AE_types['zinb-conddisp'](input_size=b.n_vars, hidden_size=(64, 32, 64), file_path=str(tmp))
    net.seed = 0
    net.build()
    train(b, net, epochs=2, batch_size=32, verbose=False, early_stop=0, reduce_lr=0)
    assert (net.engine.cc_csr is not None) == (form == 'tile') and net.engine.cc is not None
    path = os.path.join(str(tmp), form)
    net.predict_write(b, path, mode='full')
    if form == 'tile':
        monkeypatch.delenv('DCA_AMD_RESIDENT')
        monkeypatch.delenv('DCA_AMD_COUNTS_COMPACT')
    return ad, path


def test_dca_and_predict_write_from_the_byte_tile_equal_the_default_dense_run(tmp_path, monkeypatch):
    monkeypatch.delenv('DCA_AMD_RESIDENT', raising=False)
    monkeypatch.delenv('DCA_AMD_COUNTS_COMPACT', raising=False)
    rd, pd_ = _runs('dense', tmp_path, monkeypatch)
    rc, pc = _runs('tile', tmp_path, monkeypatch)
    assert (np.asarray(rd.X) == np.asarray(rc.X)).all()
    assert sorted(rd.obsm) == sorted(rc.obsm)
    for k in rd.obsm:
        assert (np.asarray(rd.obsm[k]) == np.asarray(rc.obsm[k])).all(), k
    assert rd.uns['dca_loss_history'] == rc.uns['dca_loss_history']
    files = sorted(os.listdir(pd_))
    assert files == sorted(os.listdir(pc)) and 'mean.tsv' in files
    for f in files:
        assert open(os.path.join(pd_, f), 'rb').read() == open(os.path.join(pc, f), 'rb').read(), f
