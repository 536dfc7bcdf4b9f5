"""K-OPT (dcahip_optimizer_step, dcahip_nadam_step, dcahip_counter_add, dcahip_l1l2_apply) and the fused step end
(dcahip_rmsprop_clip without and with its step-end arguments), each kernel on its own against the fp64 oracle at the sizes where the
grid-stride loops run: the cases of tests/_opt_kernel_cases.py on HipOps, and the entry points' argument checks."""
import ctypes

import pytest
import torch

import _opt_kernel_cases as C

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


@pytest.mark.parametrize('kind', C.KINDS)
def test_optimizer_three_steps(ops, kind):
    ew, es = C.optimizer_three_steps(ops, kind)
    print(kind, 'worst update error %.3g, slot error %.3g, TOL %.3g' % (ew, es, C.TOL))


def test_counter_add(ops):
    C.counter_add_cases(ops)


def test_rmsprop_stride_and_fused_end(ops):
    ew, es = C.rmsprop_stride(ops)
    print('rmsprop worst update error %.3g, slot error %.3g, TOL %.3g' % (ew, es, C.TOL))


def test_rmsprop_end_null_words(ops):
    C.rmsprop_end_null_words(ops)


def test_l1l2_apply(ops):
    C.l1l2_cases(ops)


def test_argument_checks(ops):
    """Return codes only: every refused call returns before a launch, and the same call with the argument put right
    is accepted (so the refusal is that argument's)."""
    from dca_amd import hip
    L, p, s = ops.L, hip.ptr, hip.stream()
    n = 1024
    w, g, s1, s2 = (torch.zeros(n + 4, device='cuda') for _ in range(4))
    lr = torch.tensor([1e-3], device='cuda')
    it = torch.zeros(1, dtype=torch.int64, device='cuda')
    msch = torch.ones(1, device='cuda')
    K = hip.OPT_KINDS

    def step(kind, slot1=s1, slot2=s2, iter_=it, n_=n, w_=w, g_=g, lr_=lr):
        return L.dcahip_optimizer_step(kind, p(w_), p(g_), p(slot1), p(slot2), n_, p(lr_), p(iter_), 5.0, s)
    for kind in ('sgd', 'adagrad', 'adadelta', 'adam', 'adamax'):
        assert step(K[kind]) == 0, kind
    assert step(K['sgd'], None, None, None) == 0 and step(K['adagrad'], s1, None, None) == 0
    assert step(K['adadelta'], s1, s2, None) == 0
    assert step(K['rmsprop']) == EINVAL                  # kind 1 is dcahip_rmsprop_clip's
    assert step(-1) == EINVAL and step(6) == EINVAL
    for kind in ('adagrad', 'adadelta', 'adam', 'adamax'):
        assert step(K[kind], slot1=None) == EINVAL, kind
    for kind in ('adadelta', 'adam', 'adamax'):
        assert step(K[kind], slot2=None) == EINVAL, kind
    for kind in ('adam', 'adamax'):
        assert step(K[kind], iter_=None) == EINVAL, kind
    assert step(K['sgd'], n_=0) == EINVAL and step(K['sgd'], n_=-5) == EINVAL
    assert step(K['sgd'], w_=None) == EINVAL and step(K['sgd'], g_=None) == EINVAL and step(K['sgd'], lr_=None) == EINVAL

    def nadam(**kw):
        a = dict(w=w, g=g, m=s1, v=s2, lr=lr, it=it, msch=msch)
        a.update(kw)
        return L.dcahip_nadam_step(p(a['w']), p(a['g']), p(a['m']), p(a['v']), kw.get('n', n), p(a['lr']), p(a['it']),
                                   p(a['msch']), 5.0, s)
    assert nadam() == 0
    for k in ('w', 'g', 'm', 'v', 'lr', 'it', 'msch'):
        assert nadam(**{k: None}) == EINVAL, k
    assert nadam(n=0) == EINVAL

    def rms(fn, w_=w, g_=g, ms_=s1, n_=n):
        if fn == 'plain':
            return L.dcahip_rmsprop_clip(p(w_), p(g_), p(ms_), n_, p(lr), 0.9, 1e-7, 5.0, None, 0.0, None, 0, None, None, 0, s)
        return L.dcahip_rmsprop_clip(p(w_), p(g_), p(ms_), n_, p(lr), 0.9, 1e-7, 5.0, p(msch), 1.0, None, 0, None, p(it), 0, s)   # a loss word, the cursor + 0
    for fn in ('plain', 'end'):
        assert rms(fn) == 0
        assert rms(fn, w_=w[1:]) == EINVAL and rms(fn, g_=g[2:]) == EINVAL and rms(fn, ms_=s1[3:]) == EINVAL   # 4, 8, 12 bytes off
        assert rms(fn, w_=w[4:]) == 0                                                                            # 16: aligned again
        assert rms(fn, n_=0) == EINVAL and rms(fn, w_=None) == EINVAL

    assert L.dcahip_counter_add(None, 1, s) == EINVAL
    assert L.dcahip_counter_add(p(it), 0, s) == 0

    # 16 segments are legal (the shared cases run them), 17 are not; a negative count neither
    d = hip.RegDesc()
    ws = torch.zeros(ops.l1l2_workspace_doubles(), dtype=torch.float64, device='cuda')
    loss = torch.zeros(1, device='cuda')
    d.nseg = 16                                          # all empty: nothing to launch
    assert L.dcahip_l1l2_apply(ctypes.byref(d), p(w), p(g), p(loss), p(ws), s) == 0
    for bad in (17, -1):
        d.nseg = bad
        assert L.dcahip_l1l2_apply(ctypes.byref(d), p(w), p(g), p(loss), p(ws), s) == EINVAL
    d.nseg = 1
    assert L.dcahip_l1l2_apply(ctypes.byref(d), None, p(g), p(loss), p(ws), s) == EINVAL
    assert L.dcahip_l1l2_apply(ctypes.byref(d), p(w), p(g), p(loss), None, s) == EINVAL
    assert L.dcahip_l1l2_apply(None, p(w), p(g), p(loss), p(ws), s) == EINVAL
    torch.cuda.synchronize()
    assert loss.item() == 0.0 and it.item() == 0
