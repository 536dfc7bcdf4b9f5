"""The `beta` argument of the four batch-norm backward entries (dcahip_bn_bwd_sums, dcahip_bn_bwd_apply, dcahip_bn_bwd_small,
dcahip_dense_bn_bwd_small; include/dcahip.h, conventions), through HipOps, at the smallest shapes that reach both template
instances of the small-batch kernels (B = 32 and 33) and a ragged 64-column strip (H = 20, H = 12):

  (a) code 12 (swish) without beta is refused before any launch: the call raises, every output keeps its sentinel;
  (b) code 1 (relu) does not read beta: beta=None and a beta of NaN give bit-identical outputs (that the numbers are right
      is the job of the parity tests that run these kernels through the engine);
  (c) code 12 with a real beta against the fp64 reference tests/_stack_ref.py, evaluated on the fp32 operands the kernel
      reads.  Tolerance: the class tests/test_stack_kernels_gpu.py uses for the same quantities (sums, dbeta, dZ, gW with
      its bias row, the input gradient) -- |err| <= 1e-6 * sum |terms| + the allowance for what enters already rounded
      (slope_tolerance: one ulp of xhat + beta times the slope's sensitivity), both from _stack_ref; none derived from a
      kernel's output.
Every case prints its worst error / bound before it asserts."""
import functools

import numpy as np
import pytest
import torch

import _stack_ref as SR

pytestmark = pytest.mark.gpu

SENT = 7.0
SWISH, RELU = 12, 1


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _ld(h):
    return h + (-h) % 4 + 4                  # at least four pad columns, which must keep the sentinel


def dev(a, ld=None):
    """fp32 device copy; a matrix gets rows of ld floats whose pad columns hold the sentinel."""
    a = np.asarray(a, np.float32)
    if ld is None:
        return torch.as_tensor(np.ascontiguousarray(a)).cuda()
    t = torch.full((a.shape[0], ld), SENT, dtype=torch.float32, device='cuda')
    t[:, :a.shape[1]] = torch.as_tensor(a).cuda()
    return t


def host(t):
    return t.detach().cpu().double().numpy()


def sent(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device='cuda')


@functools.lru_cache(maxsize=None)
def problem(B, H, K=0):
    """The fp32 operands of one layer's backward (widened to fp64 for the reference) and the fp64 results for swish:
    sums over the row chunks of dcahip_bn_bwd_sums and over the batch, then the step that consumes the batch's."""
    rng = np.random.RandomState(1000 * B + 10 * H + K)
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    p = dict(B=B, H=H, K=K, dH=f(rng.normal(0, 1, (B, H))), xhat=f(rng.normal(0, 1, (B, H))), beta=f(rng.normal(0, .5, H)),
             inv_std=f(rng.uniform(.5, 2., H)))
    x = p['xhat'] + p['beta']
    p['Hact'] = {SWISH: f(SR.act_fwd(SWISH, x)), RELU: f(SR.act_fwd(RELU, x))}
    if K:
        p['Hp'], p['W'] = f(rng.normal(0, 1, (B, K))), f(rng.normal(0, .3, (K, H)))
    args = (p['dH'], p['Hact'][SWISH], p['xhat'])
    p['chunks'] = SR.bwd_step(0, *args, beta=p['beta'], act=SWISH, ranges=SR.block_ranges(B, 64))
    o0 = SR.bwd_step(0, *args, beta=p['beta'], act=SWISH)
    tol = SR.REL * o0['sums_mag'][0] + o0['sums_in'][0]
    p['step'] = SR.bwd_step(1, *args, p['inv_std'], p['beta'], o0['sums'][0, 0], o0['sums'][0, 1], float(B),
                            p.get('Hp'), p.get('W'), None, SWISH, None, 0.0, (tol[0], tol[1]))
    return p


class Judge:
    def __init__(self, title):
        self.title, self.worst = title, {}

    def bound(self, what, err, bnd):
        self.worst[what] = float((np.asarray(err) / (np.asarray(bnd) + 1e-30)).max())

    def red(self, what, o, name, got):
        assert got.shape == o[name].shape, (what, got.shape, o[name].shape)
        self.bound(what, *SR.error_and_bound(o, name, got))

    def report(self):
        print('\n%s: worst error / bound  ' % self.title + '  '.join('%s %.3g' % kv for kv in sorted(self.worst.items())))
        bad = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not bad, (self.title, bad)


def refused(call, outs):
    with pytest.raises(RuntimeError, match='-22'):
        call()
    torch.cuda.synchronize()
    for t in outs:
        assert (t == SENT).all()


def same_bits(run):
    """run(beta) -> output tensors; relu with no beta and with a beta of NaN."""
    a = run(None)
    b = run(torch.full((64,), float('nan'), dtype=torch.float32, device='cuda'))
    torch.cuda.synchronize()
    for s, t in zip(a, b):
        assert torch.equal(s, t) and torch.isfinite(s).all()


def test_bn_bwd_sums_and_apply(ops):
    B, H = 65, 20
    p = problem(B, H)
    ld = _ld(H)
    R = ops.col_moments_chunks(B)
    assert R == 2 == len(SR.block_ranges(B, 64))
    dH, xhat, inv, beta = dev(p['dH'], ld), dev(p['xhat'], ld), dev(p['inv_std']), dev(p['beta'])
    Hact = {a: dev(p['Hact'][a], ld) for a in (SWISH, RELU)}

    def sums(act, b, part):
        ops.bn_bwd_sums(dH, ld, Hact[act], ld, xhat, ld, B, H, part, act, b)
        return part

    def apply(act, b, part, dZ, dbeta):
        ops.bn_bwd_apply(dH, ld, Hact[act], ld, xhat, ld, inv, part, R, float(B), B, H, dZ, ld, dbeta, act, b)
        return dZ, dbeta
    # (a)
    part, dZ, dbeta = sent(R, 2, H), sent(B, ld), sent(H)
    refused(lambda: sums(SWISH, None, part), [part])
    refused(lambda: apply(SWISH, None, torch.zeros(R, 2, H, device='cuda'), dZ, dbeta), [dZ, dbeta])
    # (b)
    same_bits(lambda b: [sums(RELU, b, sent(R, 2, H))])
    rpart = sums(RELU, None, sent(R, 2, H))
    same_bits(lambda b: apply(RELU, b, rpart, sent(B, ld), sent(H)))
    # (c)
    J = Judge('bn_bwd_sums + bn_bwd_apply, swish, B = %d, H = %d' % (B, H))
    sums(SWISH, beta, part)
    apply(SWISH, beta, part, dZ, dbeta)
    torch.cuda.synchronize()
    J.red('chunk sums', p['chunks'], 'sums', host(part))
    pp = host(part)
    S, S_tol = pp.sum(0), SR.REL * np.abs(pp).sum(0)                  # the kernel adds the chunks' sums in fp32
    J.bound('dbeta', np.abs(host(dbeta) - S[0]), S_tol[0])
    o = SR.bwd_step(1, p['dH'], p['Hact'][SWISH], p['xhat'], p['inv_std'], p['beta'], S[0], S[1], float(B), act=SWISH,
                    S_tol=(S_tol[0], S_tol[1]))
    J.red('dZ', o, 'dZ', host(dZ)[:, :H])
    assert (dZ[:, H:] == SENT).all()
    J.report()


@pytest.mark.parametrize('B', [32, 33])
def test_bn_bwd_small(ops, B):
    H = 12
    p = problem(B, H)
    ld = _ld(H)
    dH, xhat, inv, beta = dev(p['dH'], ld), dev(p['xhat'], ld), dev(p['inv_std']), dev(p['beta'])
    Hact = {a: dev(p['Hact'][a], ld) for a in (SWISH, RELU)}

    def run(act, b, dZ, dbeta):
        ops.bn_bwd_small(dH, ld, Hact[act], ld, xhat, ld, inv, float(B), B, H, dZ, ld, dbeta, act, b)
        return dZ, dbeta
    dZ, dbeta = sent(B, ld), sent(H)
    refused(lambda: run(SWISH, None, dZ, dbeta), [dZ, dbeta])
    same_bits(lambda b: run(RELU, b, sent(B, ld), sent(H)))
    J = Judge('bn_bwd_small, swish, B = %d, H = %d' % (B, H))
    run(SWISH, beta, dZ, dbeta)
    torch.cuda.synchronize()
    J.red('dbeta', p['step'], 'dbeta', host(dbeta))
    J.red('dZ', p['step'], 'dZ', host(dZ)[:, :H])
    assert (dZ[:, H:] == SENT).all()
    J.report()


@pytest.mark.parametrize('B', [32, 33])
def test_dense_bn_bwd_small(ops, B):
    K, H = 20, 12
    p = problem(B, H, K)
    ld, ldk = _ld(H), _ld(K)
    dH, xhat, inv, beta = dev(p['dH'], ld), dev(p['xhat'], ld), dev(p['inv_std']), dev(p['beta'])
    Hact = {a: dev(p['Hact'][a], ld) for a in (SWISH, RELU)}
    Hp, W = dev(p['Hp'], ldk), dev(p['W'], ld)

    def run(act, b, gW, dbeta, dHp):
        ops.dense_bn_bwd_small(dH, ld, Hact[act], ld, xhat, ld, inv, Hp, ldk, W, ld, B, K, H, True, float(B), act,
                               gW, ld, dbeta, dHp, ldk, b)
        return gW, dbeta, dHp
    outs = [sent(K + 1, ld), sent(H), sent(B, ldk)]
    refused(lambda: run(SWISH, None, *outs), outs)
    same_bits(lambda b: run(RELU, b, sent(K + 1, ld), sent(H), sent(B, ldk)))
    J = Judge('dense_bn_bwd_small, swish, B = %d, K = %d, H = %d' % (B, K, H))
    gW, dbeta, dHp = run(SWISH, beta, *outs)
    torch.cuda.synchronize()
    J.red('dbeta', p['step'], 'dbeta', host(dbeta))
    J.red('gW', p['step'], 'gW', host(gW)[:, :H])
    J.red('dHp', p['step'], 'dHprev', host(dHp)[:, :K])
    assert (gW[:, H:] == SENT).all() and (dHp[:, K:] == SENT).all()
    J.report()
