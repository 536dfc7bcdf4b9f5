"""Counts-resident mode on the MI355X: dcahip_csr_gather and the CSR statistics against the dense kernels (csr_expand +
prep_col_pass + prep_scale + index_select, gene_counts / cell_counts / prep_col_finish), the engine gathering its
minibatch against the dense engine without the byte store, dca() and predict_write in both forms -- all bit for bit --
and a dataset whose dense form does not fit the memory the allocator may use."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from dca_amd import io, prep
from dca_amd._anndata import AnnData

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _counts(n, G, density, seed, empty=(), last=None):
    """Random counts; the rows of `empty` (those the matrix has) store nothing, row `last` stores the last column."""
    rng = np.random.default_rng(seed)
    Y = sp.random(n, G, density=density, format='csr', dtype=np.float32, random_state=seed,
                  data_rvs=lambda k: rng.integers(1, 40, k).astype(np.float32))
    Y = Y.tolil()
    if last is not None:
        Y[last, G - 1] = 7
    for r in empty:
        if r < n:
            Y[r, :] = 0
    Y = Y.tocsr()
    Y.eliminate_zeros()
    return Y


def _dense_reference(ops, Ys, fac, do_log, mean, std, rows):
    """What the dense form holds for these storage rows: csr_expand -> prep_col_pass -> prep_scale, then index_select."""
    dev = torch.device('cuda')
    n, G = Ys.shape
    ld = prep._r4(G)
    Y = prep.upload_sparse(Ys, dev, ops, ld)
    X = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    R = ops.prep_chunks(n)
    part = torch.zeros(R * 2 * ld, dtype=torch.float64, device=dev)
    ops.prep_col_pass(Y, ld, n, G, fac, do_log, X, ld, part)
    if mean is not None:
        ops.prep_scale(X, ld, n, G, mean, std)
    idx = torch.as_tensor(rows, device=dev)
    return Y.index_select(0, idx), X.index_select(0, idx)


def _gather(ops, csr, rows_or_perm, B, sf, fac, do_log, mean, std, ld, perm_mode, cursor_at=3):
    """csr_gather into a NaN-filled tile with a guard row above and below."""
    dev = torch.device('cuda')
    Yt = torch.full((B + 2, ld), float('nan'), device=dev)
    Xt = torch.full((B + 2, ld), float('nan'), device=dev)
    so = torch.full((B + 2,), float('nan'), device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    if perm_mode:
        perm = torch.as_tensor(np.r_[np.zeros(cursor_at, np.int64), rows_or_perm].astype(np.int32), device=dev)
        cur = torch.full((1,), cursor_at, dtype=torch.int64, device=dev)
        ops.csr_gather(csr, perm, cur, 0, B, sf, fac, do_log, mean, std, Yt[1:], ld, Xt[1:], ld, so[1:], st)
    else:
        ops.csr_gather(csr, None, None, rows_or_perm, B, sf, fac, do_log, mean, std, Yt[1:], ld, Xt[1:], ld, so[1:], st)
    torch.cuda.synchronize()
    for t in (Yt, Xt):
        assert torch.isnan(t[0]).all() and torch.isnan(t[B + 1]).all()
    assert torch.isnan(so[0]) and torch.isnan(so[B + 1])
    return Yt[1:B + 1], Xt[1:B + 1], so[1:B + 1], int(st.item())


# G = 8064: exactly one LDS segment of the gather kernels; 8065: one segment and a 4-float tail; 16129: two and a tail
@pytest.mark.parametrize('n, G', [(60, 1001), (40, 9001), (5, 8064), (5, 8065), (5, 16129)])
@pytest.mark.parametrize('use_fac, do_log, scale', [(f, l, s) for f in (0, 1) for l in (0, 1) for s in (0, 1)])
def test_csr_gather_equals_the_dense_preprocessing(ops, n, G, use_fac, do_log, scale):
    dev = torch.device('cuda')
    Ys = _counts(n, G, 0.05, seed=G + n, empty=(0, 7, n - 1), last=2)
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
        mean[:8] = 0.0                                        # zero counts over a zero mean: 0 - 0 keeps its sign rule
        std[:G] = torch.as_tensor(rng.uniform(0.5, 3, G).astype(np.float32))
    sf = torch.as_tensor(rng.uniform(0.1, 9, n).astype(np.float32), device=dev)
    perm = rng.permutation(n)
    for rows, perm_mode in ((perm, True), (perm[:1], True), (np.arange(min(5, n - 2), n), False),
                            (np.arange(n - 1, n), False)):
        B = len(rows)
        Yg, Xg, sg, bad = _gather(ops, csr, rows if perm_mode else int(rows[0]), B, sf, fac, do_log, mean, std, ld, perm_mode)
        assert bad == 0
        Yd, Xd = _dense_reference(ops, Ys, fac, do_log, mean, std, rows)
        assert (_bits(Yg) == _bits(Yd)).all()
        assert (_bits(Xg) == _bits(Xd)).all()
        assert (_bits(sg) == _bits(sf[torch.as_tensor(rows, device=dev)])).all()


def test_malformed_csr_is_counted_and_stays_inside_the_tile(ops):
    dev = torch.device('cuda')
    G, ld = 30, 32
    indptr = torch.as_tensor([0, 3, 2, 6, 6], dtype=torch.int64, device=dev)     # row 1 decreases
    indices = torch.as_tensor([1, 40, 5, -2, 7, 29], dtype=torch.int32, device=dev)
    values = torch.arange(1, 7, dtype=torch.float32, device=dev)
    csr = prep.CsrCounts(indptr, indices, values, 4, G)
    sf = torch.ones(4, device=dev)
    rows = np.array([0, 1, 2, 3, 9])                          # storage row 9 does not exist
    Yg, Xg, sg, bad = _gather(ops, csr, rows, 5, sf, None, True, None, None, ld, True)
    assert bad >= 4                                           # column 40, column -2, the decreasing row, the missing row
    assert torch.isfinite(Yg).all() and torch.isfinite(Xg).all()
    assert Yg[0, 1].item() == 1.0 and Yg[4].abs().sum().item() == 0.0


def test_csr_gather_beyond_two_to_the_31_entries(ops):
    """nnz > 2^31 (about 17 GB on the device): the last rows' entries sit beyond INT32_MAX."""
    dev = torch.device('cuda')
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip('needs about 24 GB of free device memory (%d GB free)' % (free >> 30))
    G = 8192
    n = (2 ** 31) // G + 3
    nnz = n * G
    indptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * G
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    values = torch.empty(nnz, dtype=torch.float32, device=dev)
    step = 1 << 27
    for s in range(0, nnz, step):
        e = min(nnz, s + step)
        a = torch.arange(s, e, dtype=torch.int64, device=dev)
        indices[s:e] = (a % G).to(torch.int32)
        values[s:e] = ((a // G) % 97 + (a % G) % 5 + 1).to(torch.float32)
        del a
    csr = prep.CsrCounts(indptr, indices, values, n, G)
    rows = np.array([n - 1, 0, n - 2, n // 2])
    sf = torch.ones(n, device=dev)
    Yg, Xg, _, bad = _gather(ops, csr, rows, 4, sf, None, False, None, None, G, True)
    assert bad == 0
    g = np.arange(G)
    want = np.stack([((r % 97) + g % 5 + 1).astype(np.float32) for r in rows])
    assert (Yg.cpu().numpy() == want).all() and (Xg.cpu().numpy() == want).all()
    del csr, indices, values, indptr
    torch.cuda.empty_cache()


def test_csr_statistics_equal_the_dense_ones(ops):
    dev = torch.device('cuda')
    n, G = 700, 2003
    Ys = _counts(n, G, 0.07, seed=5, empty=(3,))
    csr = prep.upload_csr(Ys, dev, ops)
    Y = prep._upload(Ys, dev, ops=ops)
    assert (_bits(prep.csr_gene_counts(ops, csr)) == _bits(prep.gene_counts(ops, Y, n, G))).all()
    assert (_bits(prep.csr_cell_counts(ops, csr)) == _bits(prep.cell_counts(ops, Y, n, G))).all()
    fac = torch.as_tensor(np.random.default_rng(2).uniform(0.5, 2, n).astype(np.float32), device=dev)
    for f, lg in ((fac, True), (None, True), (fac, False)):
        _, nd = prep.transform(ops, Y, n, G, f, lg, True, return_norm=True)
        nc = prep.csr_norm(ops, csr, f, lg, True)
        assert (_bits(nd['mean']) == _bits(nc['mean'])).all()
        assert (_bits(nd['std']) == _bits(nc['std'])).all()


# ---------------------------------------------------------------------------------------------------- the engine
def _device_data(ops, n, G, seed, monkeypatch):
    """The same counts normalised by K-PREP in both forms."""
    out = {}
    for form in ('dense', 'counts'):
        monkeypatch.setenv('DCA_AMD_RESIDENT', form)
        Ys = sp.csr_matrix(synth_counts(n, G, seed).astype(np.float32))
        ad = AnnData(Ys, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
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
        eng.attach_device_data(dd.X, dd.Y, dd.sf, norm=dd.norm, compact=False)
    else:
        eng.attach_counts(dd.csr, dd.sf, dd.norm)
    return eng


@pytest.mark.parametrize('ae, hs, n, G, B, kw', [
    ('zinb-conddisp', (64, 32, 64), 700, 1000, 32, {}),
    ('zinb-conddisp', (64, 32, 64), 9000, 1000, 4096, {}),
    ('nb', (64, 32, 64), 700, 1000, 32, {}),
    ('zinb', (64, 32, 64), 700, 1000, 64, {}),
    ('zinb-conddisp', (128, 64, 128), 1500, 1000, 512, {}),
    ('zinb-conddisp', (64, 32, 64), 700, 1000, 32, dict(hidden_dropout=0.2, input_dropout=0.1, dropout_seed=4)),
])
def test_counts_resident_engine_equals_dense_bit_for_bit(ops, ae, hs, n, G, B, kw, monkeypatch):
    from dca_amd.train import fit_engine
    data = _device_data(ops, n, G, seed=n + G, monkeypatch=monkeypatch)
    engs = {f: _engine(ops, ae, G, hs, data[f][1], f, **kw) for f in ('dense', 'counts')}
    d, c = engs['dense'], engs['counts']
    for k in ('heads_d_exp', 'd_exp'):
        assert getattr(d, k) == getattr(c, k), k
    assert (d.tile_order is None) == (c.tile_order is None)
    if d.tile_order is not None:
        assert torch.equal(d.tile_order, c.tile_order)
    assert (d.x_exp is None) == (c.x_exp is None)
    if d.x_exp is not None:
        assert torch.equal(d.x_exp, c.x_exp)
    if hs[-1] > 64:
        assert c.x_exp is not None                            # the wide network's plane path reads it
    hist = {}
    for f, eng in engs.items():
        n_train = int(n * 0.9)
        hist[f] = fit_engine(eng, n_train, n - n_train, n_train, n - n_train, 0, epochs=2, batch_size=B,
                             shuffle_rng=np.random.RandomState(5), reduce_lr=1, early_stop=0, use_graph=True).history
    assert hist['dense'] == hist['counts']
    assert torch.equal(d.w, c.w) and torch.equal(d.ms, c.ms)
    out_d = {k: v.clone() for k, v in d.predict_chunk(0, min(n, d.Bmax), {'mean', 'latent'}).items()}
    out_c = c.predict_chunk(0, min(n, c.Bmax), {'mean', 'latent'})
    for k in out_d:
        assert torch.equal(out_d[k], out_c[k]), k
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
    monkeypatch.setenv('DCA_AMD_RESIDENT', form)
    ad = _sparse_adata(400, 600, 12)
    dca(ad, mode='denoise', epochs=3, return_info=True, random_state=1, verbose=False)
    b = io.read_dataset(_sparse_adata(333, 530, 4), transpose=False, test_split=False, copy=False)
    b = io.normalize(b, size_factors=True, logtrans_input=True, normalize_input=True)
    assert (b._dca_device.csr is not None) == (form == 'counts')
    net = AE_types['zinb-conddisp'](input_size=b.n_vars, hidden_size=(64, 32, 64), file_path=str(tmp))
    net.seed = 0
    net.build()
    train(b, net, epochs=2, batch_size=32, verbose=False, early_stop=0, reduce_lr=0)
    path = os.path.join(str(tmp), form)
    net.predict_write(b, path, mode='full')
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    return ad, path


def test_dca_and_predict_write_in_counts_mode_equal_the_dense_run(tmp_path, monkeypatch):
    rd, pd_ = _runs('dense', tmp_path, monkeypatch)
    rc, pc = _runs('counts', tmp_path, monkeypatch)
    assert (np.asarray(rd.X) == np.asarray(rc.X)).all()
    assert sorted(rd.obsm) == sorted(rc.obsm)
    for k in rd.obsm:
        assert (np.asarray(rd.obsm[k]) == np.asarray(rc.obsm[k])).all(), k
    assert rd.uns['dca_loss_history'] == rc.uns['dca_loss_history']
    files = sorted(os.listdir(pd_))
    assert files == sorted(os.listdir(pc)) and 'mean.tsv' in files
    for f in files:
        assert open(os.path.join(pd_, f), 'rb').read() == open(os.path.join(pc, f), 'rb').read(), f


CAPACITY = r'''
import sys, numpy as np, pandas as pd, scipy.sparse as sp, torch
sys.path.insert(0, %(root)r)
n, G, per_row, cap = %(n)d, %(G)d, %(per_row)d, %(cap)d
total = torch.cuda.mem_get_info()[1]
torch.cuda.set_per_process_memory_fraction(cap / total, 0)
from dca_amd import io, prep
from dca_amd._anndata import AnnData
from dca_amd.network import AE_types
from dca_amd.train import train
rng = np.random.default_rng(0)
stride = G // per_row
cols = (np.arange(per_row) * stride + rng.integers(0, stride, (n, per_row))).astype(np.int32).reshape(-1)
vals = rng.integers(1, 12, n * per_row).astype(np.float32)
X = sp.csr_matrix((vals, cols, np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, G))
ad = AnnData(X, obs=pd.DataFrame(index=['c%%d' %% i for i in range(n)]), var=pd.DataFrame(index=['g%%d' %% i for i in range(G)]))
ad = io.read_dataset(ad, transpose=False, test_split=False, copy=False)
ad = io.normalize(ad, size_factors=True, logtrans_input=True, normalize_input=True)
assert ad._dca_device.csr is not None, 'auto did not choose counts mode'
net = AE_types['zinb-conddisp'](input_size=ad.n_vars, hidden_size=(64, 32, 64))
net.seed = 0
net.build()
h = train(ad, net, epochs=1, batch_size=4096, verbose=False, early_stop=0, reduce_lr=0)
assert np.isfinite(h.history['loss']).all() and np.isfinite(h.history['val_loss']).all()
net.predict(ad, mode='latent')
assert np.isfinite(ad.obsm['X_dca']).all()
print('peak %%.2f GB of %%.2f GB' %% (torch.cuda.max_memory_allocated() / 1e9, cap / 1e9))
'''


def test_a_dataset_beyond_the_dense_budget_trains_in_counts_mode():
    """Capped allocator: below the dense estimate of 60 000 x 20 000 at 5 %, above the counts-resident need."""
    n, G, per_row = 60000, 20000, 1000
    cap = 8 * 10 ** 9
    dense, counts = prep.dense_bytes(n, G), prep.counts_bytes(n, n * per_row)
    tiles = 4096 * prep._r4(G) * 4 * (2 + 2 * 3)             # X, Y and the heads' activation / gradient planes at B = 4096
    assert counts + tiles < cap < dense, (counts, tiles, cap, dense)
    try:
        avail = os.sysconf('SC_AVPHYS_PAGES') * os.sysconf('SC_PAGE_SIZE')
    except (ValueError, OSError):
        avail = None
    if avail is not None and avail < 24 * 2 ** 30:
        pytest.skip('needs about 24 GB of free host memory for the dense normalised adata.X (%d GB free)' % (avail >> 30))
    env = dict(os.environ)
    env.pop('DCA_AMD_RESIDENT', None)
    script = CAPACITY % dict(root=ROOT, n=n, G=G, per_row=per_row, cap=cap)
    r = subprocess.run(['timeout', '-k', '10', '900', sys.executable, '-c', script], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert 'peak' in r.stdout
