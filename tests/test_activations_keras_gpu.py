"""hard_sigmoid, exponential, swish and gelu on the MI355X: one training step of every form of the hidden stack the engine
selects against the fp64 oracle (tests/_keras_acts.py extends oracle/net_np.py with the four names), with the bar of
test_engine_gpu.py::test_activations_single_step_matches_oracle -- loss 1e-5 relative, helpers.assert_grads_close, the
inference pass (predict_chunk) mean / latent to 2e-3 after the update.

The pre-activations are shifted down (_keras_acts.shift_biases): a share lies below the minimum of swish and gelu, where a
backward that derived the slope from the output h would miss the gradients by more than the tolerance
(test_activations_keras_cpu.py::test_slopes_from_the_output_would_fail_these_cases)."""
import os

import numpy as np
import pytest
import torch

import _keras_acts as KA
from helpers import assert_grads_close, make_engine, make_problem, oracle_net, run_single_step
from oracle import net_np as N

pytestmark = pytest.mark.gpu

NAMES = list(KA.NEW)
DROP = dict(hidden_dropout=[0.2, 0.0, 0.35], input_dropout=0.15, dropout_seed=0x1234567890abcdef)

# form: (ae_type, n, G, hidden, B, extra engine arguments, engine stack mode)
FORMS = {
    'small': ('zinb-conddisp', 90, 33, (12, 5, 12), 40, {}, None),               # the problem of test_activations_...
    'batch32': ('zinb-conddisp', 200, 150, (64, 32, 64), 32, {}, None),          # batch-32 chains / one-launch backward
    'throughput': ('zinb-conddisp', 1200, 120, (64, 32, 64), 1024, {}, None),    # K-STACK one-step launches
    'throughput_coop': ('zinb-conddisp', 1200, 120, (64, 32, 64), 1024, {}, 'coop'),  # K-STACK cooperative launches
    'wide': ('zinb-conddisp', 320, 600, (512, 256, 128, 256, 512), 256, {}, None),     # the plane path, layers > 64 units
    'fork': ('zinb-fork', 200, 150, (64, 32, 64), 96, {}, None),                 # per-head last layers side by side
    'dropout': ('zinb-conddisp', 200, 150, (64, 32, 64), 96, DROP, None),        # hidden (and input) dropout
}


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _params(name, ae, n, G, hs, batchnorm):
    X, Y, sf, p = make_problem(n, G, hs, ae, batchnorm, seed=6)
    p = KA.shift_biases(p, hs, batchnorm)
    if name == 'exponential':
        # exp of exp: with glorot layers behind the first, fp32 itself misses the fp64 loss of these problems by more than the
        # bar (the fp32 oracle by up to 4e-4: an outlier row normalises to ~sqrt(B) and is exponentiated), or overflows.
        # Those layers scaled down -- with batch norm below its eps, so that they stay close to the linear range -- keep
        # the problems inside fp32 (the fp32 oracle within 1e-7 of the fp64 loss)
        s = np.float32(0.005 if batchnorm else 0.05)
        p = {k: v * s if k[0] in 'Wb' and k[1:].isdigit() and k[1:] != '0' else v for k, v in p.items()}
    return X, Y, sf, p


def _check_path(eng, form, B, batchnorm):
    """The form really takes the kernels it is named after."""
    if form == 'batch32':
        assert eng._bn_small(B) and (eng._stack_chain(B) if batchnorm else eng._layer_small(B, 1))
    elif form.startswith('throughput'):
        assert eng._stack_coop(B) == batchnorm
    elif form == 'wide':
        assert eng.ws_heads is None and eng._wide_planes(B)


@pytest.mark.parametrize('batchnorm', [True, False])
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('form', list(FORMS))
def test_keras_activation_step_matches_oracle(ops, monkeypatch, form, name, batchnorm):
    KA.extend_oracle(monkeypatch)
    ae, n, G, hs, B, extra, stack = FORMS[form]
    X, Y, sf, p = _params(name, ae, n, G, hs, batchnorm)
    rows = np.random.RandomState(1).permutation(n)[:B]
    ref = oracle_net(ae, p, hs, batchnorm, activation=name, **extra)
    if form == 'wide':
        ref.row_threads = max(1, min(16, os.cpu_count() or 1))
    args = (X[rows].astype(np.float64), Y[rows].astype(np.float64), sf[rows].astype(np.float64))
    rl, rg = ref.loss_and_grads(*args)
    eng = make_engine(ops, ae, G, hs, batchnorm, 0.0, p, X, Y, sf, activation=name, **extra)
    if stack is not None:
        eng.stack_mode = stack
    loss, g, newp = run_single_step(eng, rows)
    _check_path(eng, form, B, batchnorm)
    assert abs(loss - rl) < 1e-5 * abs(rl), (loss, rl)
    if form == 'wide' and name == 'exponential' and batchnorm:
        # the one case where fp32 arithmetic cannot meet the gradient bar: the fp32 oracle misses the fp64 gradients of the
        # small weight gradients behind the scaled layers by more than it -- held to the fp32 oracle's own error instead
        _, g32 = oracle_net(ae, p, hs, batchnorm, activation=name, dtype=np.float32, **extra).loss_and_grads(
            *[a.astype(np.float32) for a in args])
        gscale = max(float(np.abs(np.asarray(v)).max()) for v in rg.values())
        for k, r in rg.items():
            r = np.asarray(r, np.float64)
            if np.abs(r).max() < 1e-9 * gscale:               # Dense bias feeding batch norm: identically 0
                assert np.abs(g[k]).max() < 1e-5 * gscale, k
                continue
            e, e32 = np.abs(g[k] - r).max(), np.abs(np.asarray(g32[k], np.float64) - r).max()
            assert e <= max(2 * e32, 2e-5 * np.abs(r).max()), (k, e, e32)
    else:
        assert_grads_close(g, rg)
    # the inference pass on the parameters and moving statistics the step left (RMSprop's first step is sign-like: a
    # gradient at the fp32 noise floor moves its parameter by a full step either way, which the exponential amplifies)
    out_ref = oracle_net(ae, newp, hs, batchnorm, activation=name).predict(X[:16].astype(np.float64),
                                                                           sf[:16].astype(np.float64))
    out = eng.predict_chunk(0, 16, {'mean', 'latent'})
    np.testing.assert_allclose(out['mean'].cpu().numpy()[:, :G], out_ref['mean'], rtol=2e-3, atol=2e-4, err_msg='mean')
    np.testing.assert_allclose(out['latent'].cpu().numpy(), out_ref['latent'], rtol=2e-3, atol=2e-4, err_msg='latent')


@pytest.mark.parametrize('name', NAMES)
def test_hidden_all_uses_the_same_forward(ops, monkeypatch, name):
    """hidden_all (the fused writer's hidden stack over every cell) applies the activation of predict_chunk."""
    KA.extend_oracle(monkeypatch)
    ae, n, G, hs = 'zinb-conddisp', 200, 150, (64, 32, 64)
    X, Y, sf, p = _params(name, ae, n, G, hs, True)
    eng = make_engine(ops, ae, G, hs, True, 0.0, p, X, Y, sf, activation=name)
    want = oracle_net(ae, p, hs, True, activation=name).forward(X.astype(np.float64), sf.astype(np.float64), training=False)
    latent = eng.hidden_all(128)                              # two chunks
    np.testing.assert_allclose(latent.cpu().numpy(), want['Z'][1], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(eng.HL_all[:, :hs[-1]].cpu().numpy(), want['H'][-1], rtol=2e-3, atol=2e-4)


def test_gelu_dca_end_to_end_and_fused_writer(tmp_path):
    """dca(activation='gelu', epochs=2) on the GPU, then predict_write's files against predict + write, byte for byte."""
    import pandas as pd
    from conftest import synth_counts
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.api import dca
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G = 333, 530
    raw = AnnData(synth_counts(n, G, 4).astype(np.float32), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                  var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ret = dca(raw, ae_type='zinb-conddisp', activation='gelu', epochs=2, copy=True, return_info=True)
    assert np.isfinite(ret.X).all() and np.isfinite(ret.obsm['X_dca_dropout']).all()
    ad = io.read_dataset(raw.copy(), transpose=False, test_split=False, copy=False)
    ad = io.normalize(ad, size_factors=True, logtrans_input=True, normalize_input=True)
    net = AE_types['zinb-conddisp'](input_size=ad.n_vars, hidden_size=(64, 32, 64), activation='gelu',
                                    file_path=str(tmp_path))
    net.seed = 0
    net.build()
    train(ad, net, epochs=2, batch_size=32, verbose=False, early_stop=0, reduce_lr=0)
    a, b = str(tmp_path / 'fused'), str(tmp_path / 'plain')
    net.predict_write(ad, a, mode='full', gene_block=140)
    net.predict(ad, mode='full', return_info=True)
    net.write(ad, b, mode='full')
    files = sorted(os.listdir(b))
    assert 'mean.tsv' in files and 'latent.tsv' in files and sorted(os.listdir(a)) == files
    for f in files:
        assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), f
