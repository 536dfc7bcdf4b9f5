"""hard_sigmoid, exponential, swish and gelu: Activation(self.activation) of dca/network.py:132-135 with every name
keras.activations knows under the pinned TF 2.4.  The fp64 formulas (tests/_keras_acts.py), the engine's operands of the
pre-activation contract on the CPU oracle, the Python surface (dca(), the command line) and the names that stay refused."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import _keras_acts as KA
from conftest import synth_counts
from helpers import assert_grads_close, make_engine, make_problem, oracle_net, run_single_step
from oracle import net_np as N

NAMES = list(KA.NEW)


@pytest.mark.parametrize('name', NAMES)
def test_fp64_slopes_match_central_differences(name):
    code = KA.NEW[name]
    x = np.linspace(-6.0, 6.0, 2401)
    if code == 10:
        x = x[np.abs(np.abs(x) - 2.5) > 1e-3]                 # hard_sigmoid's two kinks
    eps = 1e-6
    fd = (KA.fwd(code, x + eps) - KA.fwd(code, x - eps)) / (2 * eps)
    np.testing.assert_allclose(KA.grad(code, x), fd, rtol=1e-6, atol=1e-8)
    if code < KA.PRE:                                         # monotonic: the slope is a function of the output too
        np.testing.assert_allclose(KA.grad_from_out(code, KA.fwd(code, x)), KA.grad(code, x), rtol=1e-12, atol=0)


def test_fp64_forms_match_torch():
    x = torch.linspace(-9.0, 9.0, 1001, dtype=torch.float64)
    xn = x.numpy()
    np.testing.assert_allclose(KA.fwd(12, xn), torch.nn.functional.silu(x).numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(KA.fwd(13, xn), torch.nn.functional.gelu(x).numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(KA.fwd(11, xn), torch.exp(x).numpy(), rtol=1e-15)
    np.testing.assert_allclose(KA.fwd(10, xn), torch.clamp(0.2 * x + 0.5, 0, 1).numpy(), rtol=1e-15)
    assert np.isinf(KA.fwd(11, np.float32(89.0)))                 # no clamp: overflows as TensorFlow's exp
    assert abs(KA.minimum(12) + 1.2785) < 1e-3 and abs(KA.minimum(13) + 0.7518) < 1e-3


@pytest.mark.parametrize('batchnorm', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_engine_step_on_the_cpu_oracle(monkeypatch, name, batchnorm):
    """The engine hands the kernels the operands of the pre-activation contract (beta with batch norm, Z without) --
    on KerasActOps, which restates the contract in fp64 -- and matches the fp64 network."""
    KA.extend_oracle(monkeypatch)
    n, G, hs, B = 90, 33, (12, 5, 12), 40
    X, Y, sf, p = make_problem(n, G, hs, 'zinb-conddisp', batchnorm, seed=6)
    p = KA.shift_biases(p, hs, batchnorm)
    rows = np.random.RandomState(1).permutation(n)[:B]
    ref = oracle_net('zinb-conddisp', p, hs, batchnorm, activation=name)
    rl, rg = ref.loss_and_grads(X[rows].astype(np.float64), Y[rows].astype(np.float64), sf[rows].astype(np.float64))
    eng = make_engine(KA.KerasActOps(), 'zinb-conddisp', G, hs, batchnorm, 0.0, p, X, Y, sf, activation=name)
    assert eng.act == KA.NEW[name] and eng.act_pre == (KA.NEW[name] >= KA.PRE)
    loss, g, _ = run_single_step(eng, rows)
    assert abs(loss - rl) < 1e-5 * abs(rl), (loss, rl)
    assert_grads_close(g, rg)


@pytest.mark.parametrize('batchnorm', [True, False])
@pytest.mark.parametrize('name', ['swish', 'gelu'])
def test_slopes_from_the_output_would_fail_these_cases(monkeypatch, name, batchnorm):
    """The GPU cases (tests/test_activations_keras_gpu.py) shift the pre-activations so that a share lies below the
    minimum.  A backward that took the slope from h -- inverting h on the increasing branch -- misses the fp64 gradients
    there by more than the tolerance those cases hold the kernels to: the cases can catch it."""
    KA.extend_oracle(monkeypatch)
    code = KA.NEW[name]
    n, G, hs, B = 90, 33, (12, 5, 12), 40
    X, Y, sf, p = make_problem(n, G, hs, 'zinb-conddisp', batchnorm, seed=6)
    p = KA.shift_biases(p, hs, batchnorm)
    rows = np.random.RandomState(1).permutation(n)[:B]
    args = (X[rows].astype(np.float64), Y[rows].astype(np.float64), sf[rows].astype(np.float64))
    ref = oracle_net('zinb-conddisp', p, hs, batchnorm, activation=name)
    _, rg = ref.loss_and_grads(*args)
    below = np.mean(np.concatenate([ref.cache['Yb'][i].ravel() for i in range(len(hs))]) < KA.minimum(code))
    assert below > 0.1, below
    good = N.act_grad
    monkeypatch.setattr(N, 'act_grad', lambda c, x: KA.slope_from_out_upper_branch(c, KA.fwd(c, x)) if c == code
                        else good(c, x))
    _, wrong = oracle_net('zinb-conddisp', p, hs, batchnorm, activation=name).loss_and_grads(*args)
    with pytest.raises(AssertionError):
        assert_grads_close(wrong, rg)


def _adata(n=120, G=50, seed=0):
    from dca_amd._anndata import AnnData
    return AnnData(synth_counts(n, G, seed).astype(np.float32),
                   obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                   var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


@pytest.mark.parametrize('name', NAMES)
def test_dca_and_the_command_line_take_the_names(monkeypatch, tmp_path, name):
    from dca_amd.__main__ import main
    from dca_amd.api import dca
    from dca_amd.network import override_ops
    KA.extend_oracle(monkeypatch)
    with override_ops(KA.KerasActOps):
        ret = dca(_adata(), activation=name, epochs=1, copy=True, hidden_size=(8, 2, 8))
        # (exponential is not clamped, as in TensorFlow: on this problem its training overflows within the epoch)
        assert ret.X.shape == (120, 50) and (name == 'exponential' or np.isfinite(ret.X).all())
        n, G = 70, 24
        y = synth_counts(n, G, 5)
        f = str(tmp_path / 'counts.tsv')
        pd.DataFrame(y.T.astype(int), index=['g%d' % i for i in range(G)],
                     columns=['c%d' % i for i in range(n)]).to_csv(f, sep='\t')
        out = str(tmp_path / 'res')
        main([f, out, '--type', 'zinb-conddisp', '-e', '1', '-s', '8,2,8', '--activation', name])
    mean = pd.read_csv(os.path.join(out, 'mean.tsv'), sep='\t', index_col=0)
    assert mean.shape == (G, n)


def test_softmax_and_unknown_names_stay_refused():
    from dca_amd.api import dca
    from dca_amd.engine import ACT_CODES, Engine
    from dca_amd.network import override_ops
    from oracle.cpu_ops import CpuRefOps
    assert {'hard_sigmoid': 10, 'exponential': 11, 'swish': 12, 'gelu': 13}.items() <= ACT_CODES.items()
    with override_ops(CpuRefOps):
        with pytest.raises(NotImplementedError, match='row reduction'):
            dca(_adata(), activation='softmax', epochs=1)
        with pytest.raises(NotImplementedError, match='no_such_activation'):
            dca(_adata(), activation='no_such_activation', epochs=1)
    with pytest.raises(NotImplementedError, match='row reduction'):
        Engine('zinb', 10, 10, (4,), True, 0.0, ops=CpuRefOps(), activation='softmax')


def test_hyper_search_space_is_unchanged():
    from dca_amd import hyper
    assert not set(KA.NEW) & set(hyper.ACTIVATIONS)
