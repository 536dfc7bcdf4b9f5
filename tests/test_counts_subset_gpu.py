"""Counts-resident training for a gene subset on the MI355X: dcahip_csr_gather_cols against dcahip_csr_gather (the X tile
bit for bit, the Y tile = its columns selected), a malformed column map, the engine against the dense engine on
Y = counts[:, cols], and train(output_subset=...) -> predict_write in both residencies -- all bit for bit."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from dca_amd import io, prep
from dca_amd._anndata import AnnData

pytestmark = pytest.mark.gpu


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


def _tile(rows, ld, offset):
    """A NaN-filled [rows, ld] tile; offset = 1: it starts one float behind a 16-byte boundary (the scalar-store form)."""
    buf = torch.full((rows * ld + 4,), float('nan'), device='cuda')
    return buf[offset:offset + rows * ld].view(rows, ld)


def _gather(ops, csr, col_out, G_out, rows_or_perm, B, sf, fac, do_log, mean, std, ldx, ldy, perm_mode, offset=0,
            cursor_at=3):
    """csr_gather (col_out None) or csr_gather_cols into NaN-filled tiles with a guard row above and below."""
    dev = torch.device('cuda')
    Yt, Xt = _tile(B + 2, ldy, offset), _tile(B + 2, ldx, offset)
    so = torch.full((B + 2,), float('nan'), device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    if perm_mode:
        perm = torch.as_tensor(np.r_[np.zeros(cursor_at, np.int64), rows_or_perm].astype(np.int32), device=dev)
        cur = torch.full((1,), cursor_at, dtype=torch.int64, device=dev)
        sel = (perm, cur, 0)
    else:
        sel = (None, None, rows_or_perm)
    tail = (B, sf, fac, do_log, mean, std, Yt[1:], ldy, Xt[1:], ldx, so[1:], st)
    if col_out is None:
        ops.csr_gather(csr, *sel, *tail)
    else:
        ops.csr_gather_cols(csr, col_out, G_out, *sel, *tail)
    torch.cuda.synchronize()
    for t in (Yt, Xt):
        assert torch.isnan(t[0]).all() and torch.isnan(t[B + 1]).all()
    assert torch.isnan(so[0]) and torch.isnan(so[B + 1])
    return Yt[1:B + 1], Xt[1:B + 1], so[1:B + 1], int(st.item())


_PROBLEMS = {}


def _problem(ops, n, G):
    """The counts, their CSR on the device, the normalisation operands and the gathers' row sets -- made once per shape."""
    if (n, G) not in _PROBLEMS:
        dev = torch.device('cuda')
        Ys = _counts(n, G, 0.05, seed=G + n, empty=(0, 7, n - 1), last=2)
        assert Ys[2, G - 1] != 0 and Ys[0].nnz == 0
        csr = prep.upload_csr(Ys, dev, ops)
        ld = prep._r4(G)
        rng = np.random.default_rng(1)
        fac = torch.as_tensor(rng.uniform(0.3, 2.0, n).astype(np.float32), device=dev)
        mean = torch.zeros(ld, device=dev)
        std = torch.ones(ld, device=dev)
        mean[:G] = torch.as_tensor(rng.normal(0, 1, G).astype(np.float32))
        mean[:8] = 0.0
        std[:G] = torch.as_tensor(rng.uniform(0.5, 3, G).astype(np.float32))
        sf = torch.as_tensor(rng.uniform(0.1, 9, n).astype(np.float32), device=dev)
        perm = rng.permutation(n)
        per_gene = np.asarray(Ys.getnnz(axis=0))
        unstored = int(np.flatnonzero(per_gene == 0)[0])            # a gene without a stored entry
        stored = int(np.argmax(per_gene))
        others = np.setdiff1d(np.arange(G), [unstored, stored])
        srng = np.random.default_rng(7)

        def shuffled(k):
            c = np.r_[unstored, stored, srng.choice(others, k - 2, replace=False)]
            return srng.permutation(c)
        subsets = {'one': np.array([unstored]), 'one_stored': np.array([stored]), 'k37': shuffled(37),
                   'identity': np.arange(G)}
        if G > 8500:
            subsets['k8500'] = shuffled(8500)                       # more output columns than one LDS segment holds
        row_sets = {'perm': (perm, True), 'one_row': (perm[:1], True), 'range': (np.arange(min(5, n - 2), n), False)}
        _PROBLEMS[(n, G)] = dict(Ys=Ys, csr=csr, ld=ld, fac=fac, mean=mean, std=std, sf=sf, subsets=subsets,
                                 row_sets=row_sets, plain={})
    return _PROBLEMS[(n, G)]


def _col_map(G, cols):
    inv = np.full(G, -1, np.int32)
    inv[cols] = np.arange(len(cols), dtype=np.int32)
    return torch.as_tensor(inv, device='cuda')


def _plain(ops, pr, opt, rs):
    """csr_gather's tiles for these options and rows: the reference, computed once and left unchanged."""
    if (opt, rs) not in pr['plain']:
        use_fac, do_log, scale = opt
        rows, perm_mode = pr['row_sets'][rs]
        Y, X, s, bad = _gather(ops, pr['csr'], None, 0, rows if perm_mode else int(rows[0]), len(rows), pr['sf'],
                               pr['fac'] if use_fac else None, do_log, pr['mean'] if scale else None,
                               pr['std'] if scale else None, pr['ld'], pr['ld'], perm_mode)
        assert bad == 0
        pr['plain'][(opt, rs)] = (Y.clone(), X.clone(), s.clone())
    return pr['plain'][(opt, rs)]


def _check_against_plain(ops, pr, G, subset, opt, rs, offset=0):
    use_fac, do_log, scale = opt
    cols = pr['subsets'][subset]
    k = len(cols)
    ldy = prep._r4(k)
    rows, perm_mode = pr['row_sets'][rs]
    Yp, Xp, sp_ = _plain(ops, pr, opt, rs)
    Yg, Xg, sg, bad = _gather(ops, pr['csr'], _col_map(G, cols), k, rows if perm_mode else int(rows[0]), len(rows), pr['sf'],
                              pr['fac'] if use_fac else None, do_log, pr['mean'] if scale else None,
                              pr['std'] if scale else None, pr['ld'], ldy, perm_mode, offset=offset)
    assert bad == 0
    assert (_bits(Xg) == _bits(Xp)).all()
    want = torch.zeros(len(rows), ldy, device='cuda')
    want[:, :k] = Yp.index_select(1, torch.as_tensor(cols, device='cuda'))
    assert (_bits(Yg) == _bits(want)).all()                       # (the pad columns k .. ldy: +0.0)
    assert (_bits(sg) == _bits(sp_)).all()


ALL_OPTIONS = [(f, l, s) for f in (0, 1) for l in (0, 1) for s in (0, 1)]


# G = 8064: exactly one LDS segment of the gather kernels; 8065: one segment and a 4-float tail; 16129: two and a tail
@pytest.mark.parametrize('n, G', [(60, 1001), (40, 9001), (5, 8064), (5, 8065), (5, 16129)])
@pytest.mark.parametrize('opt', ALL_OPTIONS)
def test_gather_cols_equals_csr_gather_on_37_shuffled_genes(ops, n, G, opt):
    pr = _problem(ops, n, G)
    assert prep._r4(37) == 40                                     # three pad columns
    for rs in pr['row_sets']:
        _check_against_plain(ops, pr, G, 'k37', opt, rs)


@pytest.mark.parametrize('n, G, subset', [(60, 1001, 'one'), (60, 1001, 'one_stored'), (60, 1001, 'identity'),
                                          (40, 9001, 'one'), (40, 9001, 'one_stored'), (40, 9001, 'k8500'),
                                          (40, 9001, 'identity')])
def test_gather_cols_equals_csr_gather_on_the_other_subsets(ops, n, G, subset):
    pr = _problem(ops, n, G)
    for rs in pr['row_sets']:
        _check_against_plain(ops, pr, G, subset, (1, 1, 1), rs)


@pytest.mark.parametrize('n, G, subset', [(60, 1001, 'k37'), (40, 9001, 'k8500')])
def test_gather_cols_with_unaligned_tiles_takes_the_scalar_stores(ops, n, G, subset):
    pr = _problem(ops, n, G)
    _check_against_plain(ops, pr, G, subset, (1, 1, 1), 'perm', offset=1)


def test_b_zero_launches_nothing(ops):
    pr = _problem(ops, 60, 1001)
    cols = pr['subsets']['k37']
    Y = torch.full((2, 40), float('nan'), device='cuda')
    X = torch.full((2, pr['ld']), float('nan'), device='cuda')
    st = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.csr_gather_cols(pr['csr'], _col_map(1001, cols), 37, None, None, 0, 0, pr['sf'], None, True, None, None, Y, 40, X,
                        pr['ld'], None, st)
    torch.cuda.synchronize()
    assert torch.isnan(Y).all() and torch.isnan(X).all() and int(st.item()) == 0


def test_a_malformed_column_map_is_counted_and_stays_inside_the_tile(ops):
    n, G = 60, 1001
    pr = _problem(ops, n, G)
    cols = pr['subsets']['k37']
    k, ldy = 37, 40
    per_gene = np.asarray(pr['Ys'].getnnz(axis=0))
    free = np.setdiff1d(np.flatnonzero(per_gene > 0), cols)[:3]   # three genes with stored entries outside the subset
    cm = _col_map(G, cols)
    for g, v in zip(free, (k, k + 7, -5)):                        # the first pad column, the next tile row, below -1
        cm[int(g)] = v
    Yp, Xp, sp_ = _plain(ops, pr, (1, 1, 1), 'range')
    rows, _ = pr['row_sets']['range']
    Yg, Xg, sg, bad = _gather(ops, pr['csr'], cm, k, int(rows[0]), len(rows), pr['sf'], pr['fac'], True, pr['mean'], pr['std'],
                              pr['ld'], ldy, False)                # (the guard rows are checked in there)
    assert bad == int(pr['Ys'][rows][:, free].getnnz())
    assert bad > 0
    want = torch.zeros(len(rows), ldy, device='cuda')
    want[:, :k] = Yp.index_select(1, torch.as_tensor(cols, device='cuda'))
    assert (_bits(Yg) == _bits(want)).all()                       # every valid column, and the pad still +0.0
    assert (_bits(Xg) == _bits(Xp)).all()


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
    return out


def _engine(ops, ae, G, cols, hs, dd, form):
    from dca_amd.engine import Engine
    k = len(cols)
    eng = Engine(ae, G, k, hs, True, 0.0, ops=ops)
    eng.init_params(seed=3)
    if form == 'dense':
        Ysub = torch.zeros(dd.n, prep._r4(k), device='cuda')
        Ysub[:, :k] = dd.Y.index_select(1, torch.as_tensor(cols, device='cuda'))
        eng.attach_device_data(dd.X, Ysub, dd.sf, norm=dd.norm, compact=False)
    else:
        eng.attach_counts(dd.csr, dd.sf, dd.norm, out_cols=cols)
    return eng


@pytest.mark.parametrize('ae, hs, n, G, B', [
    ('zinb-conddisp', (64, 32, 64), 700, 1000, 32),
    ('zinb-conddisp', (64, 32, 64), 9000, 1000, 4096),
    ('nb', (64, 32, 64), 700, 1000, 32),
    ('zinb-conddisp', (128, 64, 128), 1500, 1000, 512),
])
def test_subset_engine_equals_dense_bit_for_bit(ops, ae, hs, n, G, B, monkeypatch):
    from dca_amd.train import fit_engine
    data = _device_data(ops, n, G, seed=n + G, monkeypatch=monkeypatch)
    cols = np.random.default_rng(3).permutation(G)[:100]
    engs = {f: _engine(ops, ae, G, cols, hs, data[f][1], f) for f in ('dense', 'counts')}
    d, c = engs['dense'], engs['counts']
    for k in ('heads_d_exp', 'd_exp'):
        assert getattr(d, k) == getattr(c, k), k
    assert (d.tile_order is None) == (c.tile_order is None)
    if d.tile_order is not None:
        assert torch.equal(d.tile_order, c.tile_order)
    assert (d.x_exp is None) == (c.x_exp is None)
    if d.x_exp is not None:
        assert torch.equal(d.x_exp, c.x_exp)
    hist = {}
    for f, eng in engs.items():
        n_train = int(n * 0.9)
        hist[f] = fit_engine(eng, n_train, n - n_train, n_train, n - n_train, 0, epochs=2, batch_size=B,
                             shuffle_rng=np.random.RandomState(5), reduce_lr=1, early_stop=0, use_graph=True).history
    assert hist['dense'] == hist['counts']
    assert torch.equal(d.w, c.w) and torch.equal(d.ms, c.ms)
    assert c.X.shape == (c.Bmax, prep._r4(G)) and c.Y.shape == (c.Bmax, 100)
    out_d = {k: v.clone() for k, v in d.predict_chunk(0, min(n, d.Bmax), {'mean', 'latent'}).items()}
    out_c = c.predict_chunk(0, min(n, c.Bmax), {'mean', 'latent'})
    for k in out_d:
        assert torch.equal(out_d[k], out_c[k]), k
    assert int(c.gather_status.item()) == 0


# ---------------------------------------------------------------------------------------------------- the surface
def _sparse_adata(n, G, seed):
    Ys = sp.csr_matrix(synth_counts(n, G, seed).astype(np.float32))
    return AnnData(Ys, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                   var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


def _run(form, tmp, monkeypatch):
    """The command line's sequence with a gene list: read_dataset -> normalize -> train(output_subset) -> predict_write."""
    from dca_amd.network import AE_types
    from dca_amd.train import train
    monkeypatch.setenv('DCA_AMD_RESIDENT', form)
    np.random.seed(0)                                        # the per-epoch shuffles draw from numpy's global stream
    b = io.read_dataset(_sparse_adata(333, 530, 4), transpose=False, test_split=False, copy=False)
    b = io.normalize(b, size_factors=True, logtrans_input=True, normalize_input=True)
    dd = b._dca_device
    assert (dd.csr is not None) == (form == 'counts')
    genes = list(np.random.default_rng(2).permutation(np.asarray(b.var_names))[:40])
    net = AE_types['zinb-conddisp'](input_size=b.n_vars, output_size=len(genes), hidden_size=(64, 32, 64), file_path=str(tmp))
    net.seed = 0
    net.build()
    h = train(b, net, epochs=2, batch_size=32, verbose=False, early_stop=0, reduce_lr=0, output_subset=genes)
    eng = net.engine
    if form == 'counts':
        assert eng.csr is dd.csr and eng.X.shape[0] == eng.Bmax < b.n_obs
        assert list(b.var_names[eng.out_cols]) == genes
    else:
        assert eng.csr is None and eng.X.shape[0] == b.n_obs
    path = os.path.join(str(tmp), form)
    net.predict_write(b, path, mode='full', colnames=np.asarray(genes))
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    return h.history, path


def test_train_with_a_gene_list_in_counts_mode_equals_the_dense_run(tmp_path, monkeypatch):
    hd, pd_ = _run('dense', tmp_path, monkeypatch)
    hc, pc = _run('counts', tmp_path, monkeypatch)
    assert hd == hc
    files = sorted(os.listdir(pd_))
    assert files == sorted(os.listdir(pc)) and {'mean.tsv', 'dispersion.tsv', 'dropout.tsv', 'latent.tsv'} <= set(files)
    for f in files:
        assert open(os.path.join(pd_, f), 'rb').read() == open(os.path.join(pc, f), 'rb').read(), f
