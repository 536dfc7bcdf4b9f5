"""Scoring a fitted model on the MI355X: dcahip_nll_marginals alone, Engine.score for every network type and both
residency modes, Autoencoder.score end to end -- against the fp64 oracle (tests/_score_ref.py).

Bars (taken from the project, not from what the kernel gives): the total to 1e-5 relative (every single-step loss test);
every per-cell / per-gene value to 2e-5 |ref| + 2e-5 max|ref| (helpers.assert_grads_close's atol_scale; the absolute term
covers the cancellation in (mean - y)^2 of 'normal' and rows / columns much smaller than the largest)."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine, oracle_net, run_single_step
from _score_ref import kernel_elements, oracle_score, assert_marginals_close
from oracle import net_np as N

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


# ---------------------------------------------------------------------------------------------------- the kernel alone
# (B, G, lda = ldy): one element on the scalar path; tail lanes on the scalar path (lda % 4 != 0); two 1024-gene segments
# with two pad columns and 37 rows (below the 64 row slices: one row per slice); the vector path with a ragged last quad,
# three segments and more rows than slices (70: six slices get two rows)
SHAPES = [(1, 1, 1), (3, 5, 5), (37, 1030, 1032), (70, 2051, 2052)]
FLAGS = [0, 1, 2, 3, 4, 8]          # every combination the engine uses (AE_HEADS / AE_LOSS_FLAG)
RIDGE = 0.05
_cases = {}


def _case(flags, shape):
    """Operands of one kernel call (host, fp32, with the pad columns poisoned) and the fp64 marginals -- made once."""
    key = (flags, shape)
    if key not in _cases:
        B, G, ld = shape
        rng = np.random.default_rng(100 * flags + B)
        pre = lambda: rng.uniform(-4.0, 4.0, size=(B, G)).astype(np.float32)
        am, ad, ap = pre(), pre(), pre()
        tw = rng.uniform(-4.0, 4.0, size=G).astype(np.float32)
        y = synth_counts(B, G, seed=B + G).astype(np.float32)
        for _ in range(min(5, B * G)):
            y[rng.integers(0, B), rng.integers(0, G)] = 5000.0
        sf = rng.uniform(0.3, 3.0, size=B).astype(np.float32)
        el = kernel_elements(flags, am, ad, ap, tw, y, sf, RIDGE)
        assert np.isfinite(el).all() and (el >= 0).all()
        _cases[key] = dict(am=am, ad=ad, ap=ap, tw=tw, y=y, sf=sf, cell=el.sum(axis=1), gene=el.sum(axis=0))
    return _cases[key]


def _padded(a, ld):
    """[B, ld] device tensor holding a in its first columns, NaN in the pad."""
    t = torch.full((a.shape[0], ld), float('nan'), dtype=torch.float32)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t.cuda()


def _call(ops, c, flags, shape, gene0=None):
    B, G, ld = shape
    am, ad, ap, y = (_padded(c[k], ld) for k in ('am', 'ad', 'ap', 'y'))
    tw = torch.full(((G + 3) // 4 * 4,), float('nan'))
    tw[:G] = torch.from_numpy(c['tw'])
    tw = tw.cuda()
    sf = torch.from_numpy(c['sf']).cuda()
    cell = torch.full((B,), float('nan'), dtype=torch.float64, device='cuda')          # overwritten
    gene = torch.zeros(G, dtype=torch.float64, device='cuda') if gene0 is None else gene0.clone()
    ws = torch.full((ops.nll_marginals_workspace_doubles(B, G),), float('nan'), dtype=torch.float64, device='cuda')
    loss_only = bool(flags & 12)
    ops.nll_marginals(am, None if (flags & 2 or loss_only) else ad, ap if flags & 1 else None, ld,
                      tw if flags & 2 else None, y, ld, sf, B, G, RIDGE, flags, cell, gene, ws)
    torch.cuda.synchronize()
    return cell, gene


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_ld%d' % s)
@pytest.mark.parametrize('flags', FLAGS)
def test_kernel_against_the_oracle(ops, flags, shape):
    B, G, ld = shape
    c = _case(flags, shape)
    base = torch.linspace(-3.0, 7.0, G, dtype=torch.float64, device='cuda') * 1e3       # gene_acc is added to
    cell, gene = _call(ops, c, flags, shape, gene0=base)
    cell, gene = cell.cpu().numpy(), (gene - base).cpu().numpy()
    assert np.isfinite(cell).all() and np.isfinite(gene).all()          # the NaN pad columns / workspace reached nothing
    what = 'flags %d %dx%d' % (flags, B, G)
    # (gene - base) carries one double rounding of base (1e4 * 2^-53 ~ 1e-12): far inside the bars
    total_rtol = 1e-5
    if (flags, shape) == (2, (1, 1, 1)):
        # the one case where fp32 arithmetic cannot meet the bar on the total: its only element is a count of 5 000 under an
        # NB with mean ~ 5 000, the two terms of NB.loss (dca/loss.py:87-88) are ~1e4 each and cancel to 94.04 -- one fp32
        # rounding of a term is 6e-6 of the result.  The fp32 oracle misses the fp64 value by 1.35e-5, the kernel (log-gamma
        # differences taken analytically, zinb_math.hpp nb_t1_large) by 1.00e-5: held to twice the fp32 oracle's own error,
        # as tests/test_activations_keras_gpu.py holds its one such case.  (The per-value bar is met: 0.25 of it.)
        e32 = kernel_elements(flags, c['am'], c['ad'], c['ap'], c['tw'], c['y'], c['sf'], RIDGE, dtype=np.float32)
        rel32 = abs(float(e32.astype(np.float64).sum()) / c['cell'].sum() - 1)
        assert 1e-5 < rel32 < 2e-5, rel32
        total_rtol = 2 * rel32
    assert_marginals_close(cell, gene, c['cell'], c['gene'], what, total_rtol=total_rtol)


@pytest.mark.parametrize('flags', [1, 2, 8])
def test_kernel_is_deterministic(ops, flags):
    shape = SHAPES[2]
    c = _case(flags, shape)
    c1, g1 = _call(ops, c, flags, shape)
    c2, g2 = _call(ops, c, flags, shape)
    assert torch.equal(c1, c2) and torch.equal(g1, g2)


def test_kernel_argument_errors_launch_nothing(ops):
    from dca_amd import hip
    L, p = hip.lib(), hip.ptr
    B, G = 3, 8
    f32 = dict(dtype=torch.float32, device='cuda')
    am, ad, ap, y = (torch.zeros(B, G, **f32) for _ in range(4))
    sf = torch.ones(B, **f32)
    cell = torch.full((B,), 7.0, dtype=torch.float64, device='cuda')
    gene = torch.full((G,), 9.0, dtype=torch.float64, device='cuda')
    ws = torch.zeros(ops.nll_marginals_workspace_doubles(B, G), dtype=torch.float64, device='cuda')

    def call(B=B, G=G, cell_=cell, gene_=gene, ws_=ws, a_pi=ap, flags=1):
        return L.dcahip_nll_marginals(p(am), p(ad), p(a_pi), G, None, p(y), G, p(sf), B, G, 0.0, flags,
                                      p(cell_), p(gene_), p(ws_), hip.stream())
    assert call(G=0) == EINVAL and call(B=0) == EINVAL
    assert call(cell_=None) == EINVAL and call(gene_=None) == EINVAL and call(ws_=None) == EINVAL
    assert call(a_pi=None) == EINVAL                                    # HAS_PI without the plane
    assert L.dcahip_nll_marginals_workspace_doubles(0, G) == 0 and L.dcahip_nll_marginals_workspace_doubles(B, 0) == 0
    torch.cuda.synchronize()
    assert (cell == 7.0).all() and (gene == 9.0).all()
    assert call() == 0                                                   # the same operands, complete: runs
    torch.cuda.synchronize()
    assert not (cell == 7.0).any() and not (gene == 9.0).any()


# ---------------------------------------------------------------------------------------------------- Engine.score
HS = (12, 5, 12)
AE_ALL = ['normal', 'poisson', 'nb', 'nb-conddisp', 'nb-shared', 'nb-fork', 'zinb', 'zinb-conddisp', 'zinb-shared',
          'zinb-fork', 'zinb-elempi']


def _ridge(ae):
    return 0.05 if ae.startswith('zinb') else 0.0


def _val_sum(eng, r0, r1, chunk=None):
    eng.acc.zero_()
    eng.eval_loss_sum(r0, r1, 1.0, chunk)
    torch.cuda.synchronize()
    return float(eng.acc[1].item())


def _check_engine(ops, ae, n, G, hs, chunks):
    X, Y, sf, p = make_problem(n, G, hs, ae, seed=6)
    ridge = _ridge(ae)
    eng = make_engine(ops, ae, G, hs, True, ridge, p, X, Y, sf)
    cell_ref, gene_ref = oracle_score(oracle_net(ae, p, hs, True, ridge), X, Y, sf)
    genes = []
    for chunk in chunks:
        res = eng.score(chunk=chunk)
        torch.cuda.synchronize()
        assert res['cell'].dtype == res['gene'].dtype == torch.float64 and res['cell'].is_cuda
        assert res['cell'].shape == (n,) and res['gene'].shape == (G,)
        cell, gene = res['cell'].cpu().numpy(), res['gene'].cpu().numpy()
        assert_marginals_close(cell, gene, cell_ref, gene_ref, '%s chunk %d' % (ae, chunk))
        genes.append(gene)
        # the validation pass over the same rows (it may take the split kernels: agreement, not equality); its fp32 scalar
        # accumulates chunk by chunk
        val = _val_sum(eng, 0, n, chunk)
        print('%s chunk %d: eval_loss_sum rel %.2e' % (ae, chunk, abs(val / cell.sum() - 1)))
        assert abs(val - cell.sum()) <= 1e-5 * abs(cell.sum())
        assert abs(gene.sum() - cell.sum()) <= 1e-5 * abs(cell.sum())
    for g in genes[1:]:
        assert (np.abs(g - genes[0]) <= 1e-12 * np.abs(genes[0])).all()
    return eng


@pytest.mark.parametrize('ae', AE_ALL)
def test_engine_score_against_the_oracle(ops, ae):
    assert set(AE_ALL) == set(N.AE_TYPES)
    _check_engine(ops, ae, 150, 33, HS, (64, 150))          # three chunks with a ragged last one | one chunk


def test_engine_score_wide_network(ops):
    _check_engine(ops, 'zinb-conddisp', 320, 600, (512, 256, 128, 256, 512), (320,))


def test_engine_score_row_range(ops):
    n, G, ae = 150, 33, 'zinb-conddisp'
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    eng = make_engine(ops, ae, G, HS, True, 0.05, p, X, Y, sf)
    full = eng.score(chunk=64)
    part = eng.score(40, 131, chunk=32)
    torch.cuda.synchronize()
    cell_ref, _ = oracle_score(oracle_net(ae, p, HS, True, 0.05), X, Y, sf)
    assert part['cell'].shape == (91,)
    tol = 2e-5 * np.abs(cell_ref[40:131]) + 2e-5 * np.abs(cell_ref).max()
    assert (np.abs(part['cell'].cpu().numpy() - cell_ref[40:131]) <= tol).all()
    assert (part['gene'] < full['gene']).all()


@pytest.mark.parametrize('ae', ['zinb-conddisp', 'nb'])
def test_score_leaves_the_training_state_untouched(ops, ae):
    n, G = 150, 33
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    rows = np.random.RandomState(1).permutation(n)[:32]
    out = []
    for scored in (False, True):
        eng = make_engine(ops, ae, G, HS, True, _ridge(ae), p, X, Y, sf)
        eng.set_optimizer('rmsprop')
        if scored:
            before = (eng.w.clone(), eng.ms.clone(), eng.acc.clone(), eng.cursor.clone(), [m.clone() for m in eng.mm],
                      [m.clone() for m in eng.mv])
            eng.score(chunk=64)
            torch.cuda.synchronize()
            after = (eng.w, eng.ms, eng.acc, eng.cursor, eng.mm, eng.mv)
            for a, b in zip(before, after):
                if isinstance(a, list):
                    assert all(torch.equal(x, y) for x, y in zip(a, b))
                else:
                    assert torch.equal(a, b)
        out.append(run_single_step(eng, rows))
    (l0, g0, p0), (l1, g1, p1) = out
    assert l0 == l1
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k


# ---------------------------------------------------------------------------------------------------- counts-resident
def _device_data(ops, n, G, seed, monkeypatch):
    """The same counts normalised by K-PREP, resident dense and as CSR."""
    import scipy.sparse as sp
    from dca_amd import prep
    from dca_amd._anndata import AnnData
    out = {}
    for form in ('dense', 'counts'):
        monkeypatch.setenv('DCA_AMD_RESIDENT', form)
        Ys = sp.csr_matrix(synth_counts(n, G, seed).astype(np.float32))
        ad = AnnData(Ys, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                     var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
        ad, dd = prep.normalize_device(ad, filter_min_counts=False, ops=ops)
        assert (dd.csr is not None) == (form == 'counts')
        out[form] = dd
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    return out


def test_counts_resident_score_equals_the_dense_one(ops, monkeypatch):
    from dca_amd.engine import Engine
    n, G, ae = 150, 33, 'zinb-conddisp'
    data = _device_data(ops, n, G, 11, monkeypatch)
    p = {k: np.asarray(v, np.float32) for k, v in N.init_params(ae, G, HS, batchnorm=True, seed=4).items()}
    res = {}
    for form, dd in data.items():
        eng = Engine(ae, G, G, HS, True, 0.05, ops=ops)
        eng.set_params(p)
        if form == 'dense':
            eng.attach_device_data(dd.X, dd.Y, dd.sf, norm=dd.norm, compact=False)
        else:
            eng.attach_counts(dd.csr, dd.sf, dd.norm)
        res[form] = eng.score(chunk=64)
        torch.cuda.synchronize()
        if form == 'counts':
            assert int(eng.gather_status.item()) == 0 and eng.Y.shape[0] == 64      # tiles, not the matrix
    assert torch.equal(res['dense']['cell'], res['counts']['cell'])
    assert torch.equal(res['dense']['gene'], res['counts']['gene'])
    dd = data['dense']
    cell_ref, gene_ref = oracle_score(oracle_net(ae, p, HS, True, 0.05), dd.X[:, :G].cpu().numpy(), dd.Y[:, :G].cpu().numpy(),
                                      dd.sf.cpu().numpy())
    assert_marginals_close(res['counts']['cell'].cpu().numpy(), res['counts']['gene'].cpu().numpy(), cell_ref, gene_ref,
                           'counts-resident')


def test_counts_resident_score_of_a_gene_subset(ops, monkeypatch):
    from dca_amd.engine import Engine
    n, G, ae = 150, 33, 'zinb-conddisp'
    dd_c, dd_d = (_device_data(ops, n, G, 11, monkeypatch)[k] for k in ('counts', 'dense'))
    cols = np.random.default_rng(3).permutation(G)[:11]             # 11 of 33 genes, shuffled order
    p = {k: np.asarray(v, np.float32) for k, v in N.init_params(ae, G, HS, output_size=11, batchnorm=True, seed=4).items()}
    eng = Engine(ae, G, 11, HS, True, 0.05, ops=ops)
    eng.set_params(p)
    eng.attach_counts(dd_c.csr, dd_c.sf, dd_c.norm, out_cols=cols)
    res = eng.score(chunk=64)
    torch.cuda.synchronize()
    assert int(eng.gather_status.item()) == 0 and res['gene'].shape == (11,)
    cell_ref, gene_ref = oracle_score(oracle_net(ae, p, HS, True, 0.05), dd_d.X[:, :G].cpu().numpy(),
                                      dd_d.Y[:, :G].cpu().numpy()[:, cols], dd_d.sf.cpu().numpy())
    assert_marginals_close(res['cell'].cpu().numpy(), res['gene'].cpu().numpy(), cell_ref, gene_ref, 'counts-resident subset')


# ---------------------------------------------------------------------------------------------------- end to end
def test_autoencoder_score_reproduces_val_loss():
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G = 333, 530
    np.random.seed(0)
    ad = AnnData(synth_counts(n, G, 4).astype(np.float32), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    ad = io.normalize(ad)
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
    net.build()
    h = train(ad, net, epochs=2, early_stop=0, reduce_lr=0, verbose=False)
    x_before = np.array(ad.X, copy=True)
    assert net.score(ad) is None
    np.testing.assert_array_equal(ad.X, x_before)
    n_val = n - int(0.9 * n)
    val = float(ad.obs['dca_nll'].values[-n_val:].mean())
    print('val_loss %.8f, scored %.8f, rel %.2e' % (h.history['val_loss'][-1], val, abs(val / h.history['val_loss'][-1] - 1)))
    assert abs(val - h.history['val_loss'][-1]) <= 1e-5 * abs(val)
    u = ad.uns['dca_nll']
    assert isinstance(u, float) and ad.obs['dca_nll'].dtype == np.float64 and ad.var['dca_nll'].dtype == np.float64
    assert abs(u - ad.obs['dca_nll'].mean()) <= 1e-12 * abs(u) and abs(u - ad.var['dca_nll'].mean()) <= 1e-12 * abs(u)
