"""K-STACK (dca_amd/csrc/dcahip_layers.hip: stack_fwd_step_kernel / stack_bwd_step_kernel, the per-step bodies of
hidden_stack_fwd_kernel / hidden_stack_bwd_kernel, stack_bwd_chain_kernel and the SyncBN entries) against the fp64
reference tests/_stack_ref.py, through HipOps.

Only single steps, the single-workgroup chain and calls refused before any launch: nothing here waits at a grid barrier.

Teacher forcing: every single-step launch is compared with the reference evaluated on what THAT launch read, read back
from the device (the previous launch's Z, the partial statistics / sums in the workspace or in stat_out / sums_out, the
dH scratch, the forward's Hact / xhat / inv_std).  So a tolerance is that of one step in fp32 whatever the depth, and a relu
mask cannot flip between kernel and reference (the sign of the fp32 sum xhat + beta is the sign of the exact sum).

Tolerances (none derived from a kernel's output):
  * elementwise outputs, as test_bn_forward_backward: H, Z, xhat rtol = atol = 2e-5; inv_std rtol 1e-5; moving statistics
    rtol 1e-5, atol 1e-6;
  * reductions and products (per-block / per-rank statistics and sums, dbeta, dZ, gW with its bias row, dH[i - 1]):
    |err| <= 1e-6 * sum |terms| + allowance for what enters already rounded, both from _stack_ref (X_mag, X_in): the terms
    are those of the expression expanded down to the launch's fp32 inputs, the allowance is slope_tolerance (ONE ulp of the
    stored activation -- for codes 12, 13 of xhat + beta -- times the slope's sensitivity to it) carried through the same
    expression;
  * hard_sigmoid: the kernel's 0.2f is not 0.2, so its kink sits 4e-8 beside +-2.5; the seeded inputs keep away from it.
Every test prints the worst error / bound per output class before it asserts."""
import numpy as np
import pytest
import torch

import _stack_ref as SR
from _judge import EL, Judge  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = 7.0
MOM, EPS = 0.99, 1e-3
F32 = dict(dtype=torch.float32, device='cuda')


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def _ld(h):
    return h + (-h) % 4


class Prob:
    """One stack problem: fp32 inputs (widened to fp64 for the reference) and the batch-sized device buffers, every row
    ld >= H + (-H) % 4 floats, one row more than the batch, pad columns and the extra row holding the sentinel."""

    def __init__(self, hs, B, act=1, seed=0, wl='tight'):
        rng = np.random.RandomState(seed)
        self.hs, self.B, self.n, self.act, self.wl = tuple(hs), B, len(hs), act, wl
        n = self.n
        f = lambda a: np.asarray(a, np.float32)
        shift = -0.8 if act >= SR.ACT_PRE else 0.0      # a share of pre-activations below the minimum of swish / gelu
        # (code 11: batch norm bounds |xhat| by sqrt(B - 1); fwd_step asserts |xhat + beta| < 40, so exp cannot overflow)
        self.Z0 = f(rng.normal(size=(B, hs[0])) * 1.5 + rng.normal(size=hs[0]))
        self.W = [None] + [f(rng.normal(size=(hs[i - 1], hs[i])) * 0.4) for i in range(1, n)]
        self.bias = [None] + [f(rng.normal(size=hs[i]) * 0.1) for i in range(1, n)]
        self.beta = [f(rng.normal(size=h) * 0.3 + shift) for h in hs]
        self.mm0 = [f(rng.normal(size=h) * 0.1) for h in hs]
        self.mv0 = [f(rng.uniform(0.5, 1.5, size=h)) for h in hs]
        self.dHtop = f(rng.normal(size=(B, hs[-1])))
        self.ld = [_ld(h) for h in hs]
        mat = lambda i: torch.full((B + 1, self.ld[i]), SENT, **F32)
        self.Z, self.XH, self.H, self.dH = ([mat(i) for i in range(n)] for _ in range(4))
        self.Z[0][:B, :hs[0]] = dev(self.Z0)
        self.dH[n - 1][:B, :hs[-1]] = dev(self.dHtop)
        self.dZ0 = mat(0)
        self.Wd, self.ldw, self.Wbuf = [None], [0], [None]
        for i in range(1, n):
            K, h = hs[i - 1], hs[i]
            if wl == 'misaligned':                       # one float past a 16-byte boundary: the non-vector tile path
                buf = torch.full((K * h + 8,), SENT, **F32)
                w = buf[1:1 + K * h].view(K, h)
                ldw = h
            else:
                ldw = h + (4 if wl == 'padded' else 0)
                buf = torch.full((K, ldw), SENT, **F32)
                w = buf
            w[:, :h] = dev(self.W[i])
            assert w.data_ptr() % 16 == (4 if wl == 'misaligned' else 0)
            self.Wd.append(w); self.ldw.append(ldw); self.Wbuf.append(buf)
        self.bd = [None] + [dev(self.bias[i]) for i in range(1, n)]
        self.betad = [dev(b) for b in self.beta]
        self.ldg = [0] + [hs[i] + (4 if wl == 'padded' else 0) for i in range(1, n)]

    def batch_buffers(self):
        d = {'dZ0': self.dZ0}
        for i in range(self.n):
            d.update({'Z%d' % i: self.Z[i], 'XH%d' % i: self.XH[i], 'H%d' % i: self.H[i], 'dH%d' % i: self.dH[i]})
        return d

    def check_untouched(self, J):
        B = self.B
        for k, t in self.batch_buffers().items():
            h = self.hs[0] if k == 'dZ0' else self.hs[int(k.lstrip('ZXHd'))]
            J.true('pad columns of ' + k, bool((t[:, h:] == SENT).all()))
            J.true('extra row of ' + k, bool((t[B:] == SENT).all()))
        for i in range(1, self.n):
            ref = torch.full_like(self.Wbuf[i], SENT)
            if self.wl == 'misaligned':
                ref[1:1 + self.hs[i - 1] * self.hs[i]] = dev(self.W[i]).reshape(-1)
            else:
                ref[:, :self.hs[i]] = dev(self.W[i])
            J.true('W%d unchanged' % i, torch.equal(self.Wbuf[i], ref))


class Rank:
    """Rows [a, b) of a problem with what a data-parallel rank owns: workspace, moving statistics, inv_std, dbeta, gW.
    Test (a) is one rank over every row."""

    def __init__(self, ops, P, a, b):
        self.P, self.a, self.b, self.B = P, a, b, b - a
        hs, n = P.hs, P.n
        vec = lambda v, h: torch.cat([dev(v), torch.full((4,), SENT, **F32)]) if v is not None else torch.full((h + 4,), SENT, **F32)
        self.mm = [vec(P.mm0[i], hs[i]) for i in range(n)]
        self.mv = [vec(P.mv0[i], hs[i]) for i in range(n)]
        self.inv = [vec(None, hs[i]) for i in range(n)]
        self.dbeta = [vec(None, hs[i]) for i in range(n)]
        self.gW = [None] + [torch.full((hs[i - 1] + 2, P.ldg[i]), SENT, **F32) for i in range(1, n)]
        self.nbytes = ops.hidden_stack_workspace_bytes(n, self.B) if self.B > 0 else 0
        self.ws = torch.zeros(max(self.nbytes, 256), dtype=torch.uint8, device='cuda')[:max(self.nbytes, 1)]
        assert self.ws.data_ptr() % 16 == 0
        self.stat_out = [torch.full((2, hs[i]), SENT, **F32) for i in range(n)]
        self.sums_out = [torch.full((2, hs[i]), SENT, **F32) for i in range(n)]
        self.gw_ref, self.mean_ref = {}, {}

    def rows(self, t):
        return t[self.a:self.b]

    def fwd_entries(self):
        P, out = self.P, []
        for i in range(P.n):
            e = dict(H=P.hs[i], beta=P.betad[i], moving_mean=self.mm[i], moving_var=self.mv[i], Z=self.rows(P.Z[i]), ldz=P.ld[i],
                     xhat=self.rows(P.XH[i]), ldx=P.ld[i], Hout=self.rows(P.H[i]), ldh=P.ld[i], inv_std=self.inv[i])
            if i > 0:
                e.update(W=P.Wd[i], ldw=P.ldw[i], bias=P.bd[i], K=P.hs[i - 1])
            out.append(e)
        return out

    def bwd_layers(self):
        P, out = self.P, []
        for i in range(P.n):
            d = dict(H=P.hs[i], Hact=self.rows(P.H[i]), ldh=P.ld[i], xhat=self.rows(P.XH[i]), ldx=P.ld[i], inv_std=self.inv[i],
                     dbeta=self.dbeta[i], dH=self.rows(P.dH[i]), lddh=P.ld[i], beta=P.betad[i])
            if i > 0:
                d.update(W=P.Wd[i], ldw=P.ldw[i], K=P.hs[i - 1], Hprev=self.rows(P.H[i - 1]), ldp=P.ld[i - 1], gW=self.gW[i],
                         ldg=P.ldg[i])
            out.append(d)
        return out

    def dz0(self):
        return self.rows(self.P.dZ0)

    def part(self, i, nwg, H):
        """[nwg, 2, H] partial statistics / sums of layer i in the workspace."""
        f = self.ws[256:].view(torch.float32)
        o = i * nwg * 2 * 64
        return f[o:o + nwg * 2 * H].view(nwg, 2, H)

    def own_buffers(self):
        d = {'ws': self.ws}
        for i in range(self.P.n):
            d.update({'mm%d' % i: self.mm[i], 'mv%d' % i: self.mv[i], 'inv%d' % i: self.inv[i], 'dbeta%d' % i: self.dbeta[i],
                      'stat_out%d' % i: self.stat_out[i], 'sums_out%d' % i: self.sums_out[i]})
            if i > 0:
                d['gW%d' % i] = self.gW[i]
        return d

    def check_untouched(self, J):
        hs = self.P.hs
        J.true('workspace counters back at zero', bool((self.ws[:256] == 0).all()))
        for i in range(self.P.n):
            for k, t in (('mm', self.mm[i]), ('mv', self.mv[i]), ('inv', self.inv[i]), ('dbeta', self.dbeta[i])):
                J.true('tail of %s%d' % (k, i), bool((t[hs[i]:] == SENT).all()))
            if i > 0:
                J.true('pad of gW%d' % i, bool((self.gW[i][:, hs[i]:] == SENT).all() and (self.gW[i][hs[i - 1] + 1:] == SENT).all()))


def snapshot(P, ranks):
    d = {k: t.clone() for k, t in P.batch_buffers().items()}
    for r, R in enumerate(ranks):
        d.update({'%d.%s' % (r, k): t.clone() for k, t in R.own_buffers().items() if k != 'ws'})
    return d


def same_bits(J, what, s0, s1, keys=None):
    for k in (keys or sorted(s0)):
        J.true('%s: %s bit for bit' % (what, k), torch.equal(s0[k], s1[k]))


# ------------------------------------------------------------------ one forward step, launched and judged
def fwd_step(ops, J, R, st, rows=32, ext=None, sync=False, check=True):
    """Launches forward step `st` on rank R (sync: the data-parallel entry with ext = (entries [E, 2, H], counts [E])) and
    compares everything it wrote with the reference run on what it read."""
    P, B, n, hs, act = R.P, R.B, R.P.n, R.P.hs, R.P.act
    i = max(st - 1, 0)
    made = 0 if st == 0 else (i + 1 if i + 1 < n else None)
    mm0, mv0 = [t.clone() for t in R.mm], [t.clone() for t in R.mv]
    if sync:
        so = R.stat_out[made] if made is not None else None
        ops.hidden_stack_fwd_sync(R.fwd_entries(), B, MOM, EPS, act, st, ext[0] if ext else None, ext[1] if ext else None,
                                  int(ext[1].numel()) if ext else 0, so, R.ws)
    else:
        ops.hidden_stack_fwd(R.fwd_entries(), B, MOM, EPS, act, R.ws, rows_per_wg=rows, steps=(st, st))
    torch.cuda.synchronize()
    if not check:
        return
    what = 'fwd step %d rows [%d, %d)' % (st, R.a, R.b)
    ranges = SR.block_ranges(B, rows)
    nwg = len(ranges)
    Zin = host(R.rows(P.Z[i]))[:, :hs[i]]
    o = None
    if st > 0:
        if sync:
            ent, cnt = host(ext[0]), host(ext[1])
        else:
            ent, cnt = host(R.part(i, nwg, hs[i])), np.array([b - a for a, b in ranges], np.float64)
        last = i + 1 == n
        o = SR.fwd_step(st, Zin, cnt, ent[:, 0], ent[:, 1], P.beta[i].astype(np.float64),
                        None if last else P.W[i + 1].astype(np.float64), None if last else P.bias[i + 1].astype(np.float64),
                        host(mm0[i])[:hs[i]], host(mv0[i])[:hs[i]], act, ranges)
        R.mean_ref[i] = (o['mean'], o['var'])
        if act == 11:                                    # exponential: the pre-activations stay far inside the fp32 range of exp
            assert np.abs(o['xhat'] + P.beta[i]).max() < 40.0
        J.elem('xhat', what, host(R.rows(P.XH[i]))[:, :hs[i]], o['xhat'])
        J.elem('H', what, host(R.rows(P.H[i]))[:, :hs[i]], o['H'])
        J.elem('inv_std', what, host(R.inv[i])[:hs[i]], o['inv_std'])
        J.elem('mm', what, host(R.mm[i])[:hs[i]], o['mm'])
        J.elem('mv', what, host(R.mv[i])[:hs[i]], o['mv'])
        if not last:
            J.elem('Z', what, host(R.rows(P.Z[i + 1]))[:, :hs[i + 1]], o['Z'])
    for j in range(n):                                   # the moving statistics of every other layer stay as they were
        if st == 0 or j != i:
            J.true(what + ': mm / mv of layer %d untouched' % j, torch.equal(R.mm[j], mm0[j]) and torch.equal(R.mv[j], mv0[j]))
    if made is not None:
        # the statistics of the layer made, from the pre-activation the kernel itself wrote
        Zm = host(R.rows(P.Z[made]))[:, :hs[made]]
        s = SR.range_stats(Zm, ranges)
        got = host(R.part(made, nwg, hs[made]))
        J.bound('block mean', what, np.abs(got[:, 0] - s['mean']), SR.REL * s['mean_mag'])
        J.bound('block M2', what, np.abs(got[:, 1] - s['m2']), SR.REL * s['m2_mag'] + s['m2_in'])
        if sync:
            s = SR.range_stats(Zm, [(0, B)])
            got = host(R.stat_out[made])
            J.bound('rank mean', what, np.abs(got[0] - s['mean'][0]), SR.REL * s['mean_mag'][0])
            J.bound('rank M2', what, np.abs(got[1] - s['m2'][0]), SR.REL * s['m2_mag'][0] + s['m2_in'][0])


def bwd_step(ops, J, R, st, n_total, rows=32, ext=None, sync=False, check=True):
    """Backward step `st` (0 .. n) on rank R; sync: ext = the all-reduced sums [2, H] of the step's layer."""
    P, B, n, hs, act = R.P, R.B, R.P.n, R.P.hs, R.P.act
    i = n - 1 if st == 0 else n - st
    made = i if st == 0 else (i - 1 if i > 0 else None)
    if sync:
        ops.hidden_stack_bwd_sync(R.bwd_layers(), B, n_total, act, R.dz0(), P.ld[0], st, ext,
                                  R.sums_out[made] if made is not None else None, R.ws)
    else:
        ops.hidden_stack_bwd(R.bwd_layers(), B, n_total, act, R.dz0(), P.ld[0], R.ws, rows_per_wg=rows, steps=(st, st))
    torch.cuda.synchronize()
    if not check:
        return
    what = 'bwd step %d rows [%d, %d)' % (st, R.a, R.b)
    ranges = SR.block_ranges(B, rows)
    nwg = len(ranges)
    h = hs[i]
    cut = lambda t, w: host(R.rows(t))[:, :w]
    beta = P.beta[i].astype(np.float64)
    if st == 0:
        o = SR.bwd_step(0, cut(P.dH[i], h), cut(P.H[i], h), cut(P.XH[i], h), beta=beta, act=act, ranges=ranges)
        J.red('block sums', what, o, 'sums', host(R.part(i, nwg, h)))
        low_sums = o
        key = 'sums'
    else:
        if sync:
            S, S_tol = host(ext), (0.0, 0.0)
        else:
            p = host(R.part(i, nwg, h))
            S, S_tol = p.sum(0), tuple(SR.REL * np.abs(p).sum(0))        # the kernel adds the blocks' sums in fp32
            J.bound('dbeta', what, np.abs(host(R.dbeta[i])[:h] - S[0]), S_tol[0])
        low = None
        if i > 0:
            K = hs[i - 1]
            low = dict(Hact=cut(P.H[i - 1], K), xhat=cut(P.XH[i - 1], K), beta=P.beta[i - 1].astype(np.float64))
        o = SR.bwd_step(st, cut(P.dH[i], h), cut(P.H[i], h), cut(P.XH[i], h), host(R.inv[i])[:h], beta, S[0], S[1], n_total,
                        low['Hact'] if low else None, P.W[i].astype(np.float64) if low else None, low, act, ranges, 0.0, S_tol)
        if sync:
            J.red('dbeta', what, o, 'dbeta', host(R.dbeta[i])[:h])       # the local share, written with the sums one step earlier
        if i == 0:
            J.red('dZ0', what, o, 'dZ', host(R.dz0())[:, :h])
        else:
            R.gw_ref[i] = o
            J.red('dH[i-1]', what, o, 'dHprev', cut(P.dH[i - 1], hs[i - 1]))
            J.red('block sums', what, o, 'low_sums', host(R.part(i - 1, nwg, hs[i - 1])))
        low_sums, key = o, 'low_sums'
    if sync and made is not None:
        # this rank's sums of the layer made: the blocks' sums added in fp32
        o2 = {'s': low_sums[key].sum(0), 's_mag': low_sums[key + '_mag'].sum(0), 's_in': low_sums[key + '_in'].sum(0)}
        J.red('rank sums', what, o2, 's', host(R.sums_out[made]))
        J.true(what + ': dbeta of the layer made = the first half of sums_out',
               torch.equal(R.dbeta[made][:hs[made]], R.sums_out[made][0]))


def gw_step(ops, J, R, n_total, check=True):
    """Step n + 1: the blocks' weight-gradient partials added up."""
    P, n, hs = R.P, R.P.n, R.P.hs
    ops.hidden_stack_bwd(R.bwd_layers(), R.B, n_total, P.act, R.dz0(), P.ld[0], R.ws, rows_per_wg=32, steps=(n + 1, n + 1))
    torch.cuda.synchronize()
    if check:
        for i in range(1, n):
            J.red('gW', 'gW%d rows [%d, %d)' % (i, R.a, R.b), R.gw_ref[i], 'gW', host(R.gW[i])[:hs[i - 1] + 1, :hs[i]])


def single_gpu_pass(ops, J, P, rows, check=True, backward=True):
    """Both passes, one step per launch, on one rank that holds every row."""
    R = Rank(ops, P, 0, P.B)
    assert R.nbytes == ops.hidden_stack_workspace_bytes(P.n, P.B) and R.ws.numel() == R.nbytes
    n = P.n
    for st in range(n + 1):
        fwd_step(ops, J, R, st, rows, check=check)
    if check:
        for i in range(n):                               # updated exactly once per pass
            m, v = R.mean_ref[i]
            J.elem('mm', 'mm%d after the pass' % i, host(R.mm[i])[:P.hs[i]], P.mm0[i] - (P.mm0[i].astype(np.float64) - m) * (1 - MOM))
            J.elem('mv', 'mv%d after the pass' % i, host(R.mv[i])[:P.hs[i]], P.mv0[i] - (P.mv0[i].astype(np.float64) - v) * (1 - MOM))
        J.true('workspace counters zero after the forward pass', bool((R.ws[:256] == 0).all()))
    if backward:
        for st in range(n + 1):
            bwd_step(ops, J, R, st, float(P.B), rows, check=check)
        if rows == 32:
            gw_step(ops, J, R, float(P.B), check)
        else:                                            # the generic kernel adds the partials of ITS row partition
            ops.hidden_stack_bwd(R.bwd_layers(), R.B, float(P.B), P.act, R.dz0(), P.ld[0], R.ws, rows_per_wg=rows, steps=(n + 1, n + 1))
            torch.cuda.synchronize()
            if check:
                for i in range(1, n):
                    J.red('gW', 'gW%d' % i, R.gw_ref[i], 'gW', host(R.gW[i])[:P.hs[i - 1] + 1, :P.hs[i]])
    if check:
        P.check_untouched(J)
        R.check_untouched(J)
    return R


# ------------------------------------------------------------------ (a)
S3, S4, S8 = (64, 32, 64), (48, 20, 7, 33), (16, 8, 16, 8, 16, 8, 16, 8)
STEP_CASES = []
for _hs, _B, _rows in [(S3, 33, 32), (S3, 32, 32), (S3, 65, 32), (S3, 4100, 32), (S3, 130, 16), (S3, 130, 64), (S4, 513, 32),
                       ((10,), 300, 32), (S8, 70, 32), ((1, 1), 40, 32)]:
    for _wl in ('tight', 'padded'):
        STEP_CASES.append(pytest.param(_hs, _B, _rows, _wl, 1, id='%s-B%d-r%d-%s-relu' % ('x'.join(map(str, _hs)), _B, _rows, _wl)))
STEP_CASES.append(pytest.param(S3, 65, 32, 'misaligned', 1, id='64x32x64-B65-r32-misaligned-relu'))
for _code in (0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13):
    STEP_CASES.append(pytest.param(S3, 65, 32, 'tight', _code, id='64x32x64-B65-r32-tight-act%d' % _code))
STEP_CASES.append(pytest.param(S3, 1, 32, 'tight', 1, id='64x32x64-B1-r32-forward-only'))


@pytest.mark.parametrize('hs,B,rows,wl,act', STEP_CASES)
def test_step_kernels_vs_fp64(ops, hs, B, rows, wl, act):
    """dcahip_hidden_stack_fwd steps 0 .. n and dcahip_hidden_stack_bwd steps 0 .. n + 1, one step per call: at 32 rows per
    workgroup the step kernels, at 16 / 64 the per-step bodies of the generic kernels.  Every array a step writes is compared
    with the reference on the step's own inputs; a second run from the same inputs reproduces every output bit for bit.
    (B = 1: forward only -- xhat = 0 and inv_std = eps^-1/2 leave the backward nothing to compare.)"""
    J = Judge('steps %s B=%d rows=%d %s act=%d' % (hs, B, rows, wl, act))
    seed = 1000 + B + 7 * len(hs) + act
    P = Prob(hs, B, act, seed, wl)
    R = single_gpu_pass(ops, J, P, rows, backward=B > 1)
    first = snapshot(P, [R])
    P2 = Prob(hs, B, act, seed, wl)
    R2 = single_gpu_pass(ops, J, P2, rows, check=False, backward=B > 1)
    same_bits(J, 'second run', first, snapshot(P2, [R2]))
    J.report()


# ------------------------------------------------------------------ (b)
CHAIN_CASES = [pytest.param(hs, B, 1, id='%s-B%d-relu' % ('x'.join(map(str, hs)), B))
               for hs in (S3, S4, (16, 8), (10,)) for B in (2, 5, 32, 33, 64)]
CHAIN_CASES += [pytest.param(S3, 32, 12, id='64x32x64-B32-swish'), pytest.param(S3, 32, 5, id='64x32x64-B32-selu')]


@pytest.mark.parametrize('hs,B,act', CHAIN_CASES)
def test_backward_chain_vs_fp64(ops, hs, B, act):
    """dcahip_hidden_stack_bwd over all steps without a workspace: stack_bwd_chain_kernel (n = 1 .. 4, float4 and scalar
    kernel tiles, B <= 32 and B > 32).  Its inputs are the Hact / xhat / inv_std that dcahip_hidden_small_chain wrote for the
    same batch; the reference is the fp64 whole pass from those stored arrays, its bounds those of the chain (a result
    that feeds the next layer carries its allowance along, _stack_ref.bwd_pass)."""
    J = Judge('chain %s B=%d act=%d' % (hs, B, act))
    P = Prob(hs, B, act, 2000 + B + len(hs) + act)
    R = Rank(ops, P, 0, B)
    n = P.n
    ops.hidden_small_chain(R.fwd_entries(), None, 0, B, True, MOM, EPS, act)
    torch.cuda.synchronize()
    before = snapshot(P, [R])
    ops.hidden_stack_bwd(R.bwd_layers(), B, float(B), act, R.dz0(), P.ld[0], None)
    torch.cuda.synchronize()
    cut = lambda t, w: host(t)[:B, :w]
    layers = [dict(Hact=cut(P.H[i], hs[i]), xhat=cut(P.XH[i], hs[i]), inv_std=host(R.inv[i])[:hs[i]], beta=P.beta[i].astype(np.float64),
                   W=P.W[i].astype(np.float64) if i > 0 else None) for i in range(n)]
    ref = SR.bwd_pass(P.dHtop.astype(np.float64), layers, float(B), act)
    J.red('dZ0', 'dZ0', ref[0], 'dZ', cut(P.dZ0, hs[0]))
    for i in range(n):
        J.red('dbeta', 'dbeta%d' % i, ref[i], 'dbeta', host(R.dbeta[i])[:hs[i]])
        if i > 0:
            J.red('gW', 'gW%d' % i, ref[i], 'gW', host(R.gW[i])[:hs[i - 1] + 1, :hs[i]])
            J.red('dH[i-1]', 'dH%d' % (i - 1), ref[i], 'dHprev', cut(P.dH[i - 1], hs[i - 1]))
    after = snapshot(P, [R])
    same_bits(J, 'inputs of the chain', before, after,
              [k for k in before if k[0] in 'ZXH' or k.startswith(('0.mm', '0.mv', '0.inv')) or k == 'dH%d' % (n - 1)])
    P.check_untouched(J)
    R.check_untouched(J)
    J.report()


# ------------------------------------------------------------------ (c)
def _emulated_ranks(ops, J, P, counts, junk_at=None, check=True):
    """The call sequence of Engine._hidden_forward / _forward_backward for a data-parallel step, the ranks = consecutive row
    ranges of one batch run one after the other, the collectives done here: all-gather = concatenation of the stat_out,
    all-reduce = fp32 sum of the sums_out in rank order.  An EMPTY rank launches nothing (B = 0 is DCAHIP_EINVAL for these
    entries; the engine sends it down the per-operation path): what it contributes is what that path sends -- a zeroed
    (mean, M2) entry (Engine._batch_moments: self.stat_local[i].zero_()) with count 0, and zeros to the reduce
    (Engine._empty_step: torch.zeros(2 * h)).  junk_at: a further entry with count 0, mean 3, M2 5 at that index;
    junk_at = 'merged': every rank is handed ONE entry instead, the ranks' entries merged beforehand (fp64, rounded to fp32),
    with the global count -- a count other than the rank's own B, so the entry is used as handed in."""
    n, hs, Bg = P.n, P.hs, P.B
    ranks = [Rank(ops, P, a, b) for a, b in SR.split_ranges(counts)]
    live = [R for R in ranks if R.B > 0]

    def gather(i):
        ent = [R.stat_out[i] if R.B > 0 else torch.zeros(2, hs[i], **F32) for R in ranks]
        cnt = [float(R.B) for R in ranks]
        if junk_at == 'merged':
            e = np.stack([host(t) for t in ent])
            _, m, q = SR.merge_stats(cnt, e[:, 0], e[:, 1])
            return dev(np.stack([m, q])[None]).contiguous(), torch.tensor([float(Bg)], **F32)
        if junk_at is not None:
            ent.insert(junk_at, torch.stack([torch.full((hs[i],), 3.0, **F32), torch.full((hs[i],), 5.0, **F32)]))
            cnt.insert(junk_at, 0.0)
        return torch.stack(ent).contiguous(), torch.tensor(cnt, **F32)

    def reduce(i):
        tot = torch.zeros(2, hs[i], **F32)
        for R in ranks:
            tot = tot + (R.sums_out[i] if R.B > 0 else torch.zeros(2, hs[i], **F32))
        if check and len(live) > 2:
            S = np.stack([host(R.sums_out[i]) for R in live])
            J.bound('all-reduce', 'sums of layer %d' % i, np.abs(host(tot) - S.sum(0)), SR.REL * np.abs(S).sum(0))
        return tot

    for R in live:
        fwd_step(ops, J, R, 0, sync=True, check=check)
    for st in range(1, n + 1):
        ext = gather(st - 1)
        for R in live:
            fwd_step(ops, J, R, st, ext=ext, sync=True, check=check)
    for R in live:
        bwd_step(ops, J, R, 0, float(Bg), sync=True, check=check)
    for st in range(1, n + 1):
        ext = reduce(n - st)
        for R in live:
            bwd_step(ops, J, R, st, float(Bg), ext=ext, sync=True, check=check)
    for R in live:
        gw_step(ops, J, R, float(Bg), check)
    if check:
        for i in range(n):
            for R in live[1:]:
                J.true('ranks agree on mm / mv / inv_std of layer %d' % i, torch.equal(R.mm[i], live[0].mm[i]) and
                       torch.equal(R.mv[i], live[0].mv[i]) and torch.equal(R.inv[i], live[0].inv[i]))
            m, v = live[0].mean_ref[i]
            J.elem('mm', 'mm%d after the pass' % i, host(live[0].mm[i])[:hs[i]], P.mm0[i] - (P.mm0[i].astype(np.float64) - m) * (1 - MOM))
            J.elem('mv', 'mv%d after the pass' % i, host(live[0].mv[i])[:hs[i]], P.mv0[i] - (P.mv0[i].astype(np.float64) - v) * (1 - MOM))
            if i > 0:                                    # the ranks' shares add up to the gradient of the global batch
                o = {k: sum(R.gw_ref[i][k] for R in live) for k in ('gW', 'gW_mag', 'gW_in')}
                J.red('sum of gW', 'gW%d' % i, o, 'gW', sum(host(R.gW[i])[:hs[i - 1] + 1, :hs[i]] for R in live))
        J.true('every row of dZ0 written', bool((P.dZ0[:Bg, :hs[0]] != SENT).all()))
        P.check_untouched(J)
        for R in live:
            R.check_untouched(J)
    return ranks


SYNC_LAYOUTS = {'one': ([200], None), 'two': ([100, 100], None), 'partial': ([33, 1, 166], None), 'empty': ([64, 0, 136], None),
                'many': ([2] * 130, None), 'merged': ([100, 100], 'merged'), 'partial_junk': ([33, 1, 166], 3), 'many_junk': ([2] * 130, 129)}
SYNC_CASES = [pytest.param(hs, name, 1, id='%s-%s-relu' % ('x'.join(map(str, hs)), name)) for hs in (S3, S4) for name in SYNC_LAYOUTS]
SYNC_CASES += [pytest.param(hs, 'partial', 13, id='%s-partial-gelu' % 'x'.join(map(str, hs))) for hs in (S3, S4)]


@pytest.mark.parametrize('hs,layout,act', SYNC_CASES)
def test_sync_steps_emulated_ranks_vs_fp64(ops, hs, layout, act):
    """dcahip_hidden_stack_fwd_sync / _bwd_sync with the ranks of a data-parallel step emulated in one process (see
    _emulated_ranks): per rank and step against the reference with the statistics of the global batch and n_total = Bg;
    a single rank reproduces the single-GPU step kernels bit for bit; an entry with count 0 -- an empty rank's, or one that
    carries finite junk -- changes no result, among the first 128 entries (kept in registers) or beyond them; one entry
    merged beforehand, with a count other than the rank's own, is used as handed in."""
    counts, junk_at = SYNC_LAYOUTS[layout]
    Bg = sum(counts)
    J = Judge('sync %s %s act=%d' % (hs, layout, act))
    seed = 3000 + len(hs) + act
    P = Prob(hs, Bg, act, seed)
    ranks = _emulated_ranks(ops, J, P, counts, junk_at)
    if layout == 'one':
        P1 = Prob(hs, Bg, act, seed)
        R1 = single_gpu_pass(ops, J, P1, 32, check=False)
        s0, s1 = snapshot(P, ranks), snapshot(P1, [R1])
        same_bits(J, 'one rank = one GPU', s0, s1, [k for k in s1 if 'stat_out' not in k and 'sums_out' not in k])
    if isinstance(junk_at, int):
        P1 = Prob(hs, Bg, act, seed)
        base = _emulated_ranks(ops, J, P1, counts, None, check=False)
        same_bits(J, 'zero-count entry with junk', snapshot(P1, base), snapshot(P, ranks))
    J.report()


# ------------------------------------------------------------------ (d)
class _NullTensor:
    """A NULL device pointer that claims n bytes: tells the pointer check of an entry point from its size check."""
    is_cuda = True

    def __init__(self, n):
        self.n = n

    def data_ptr(self):
        return 0

    def numel(self):
        return self.n

    def element_size(self):
        return 1


def _refused(ops, J, what, P, R, call):
    before = snapshot(P, [R])
    ws0 = R.ws.clone()
    try:
        call()
        J.true(what + ': accepted', False)
    except RuntimeError as e:
        J.true(what + ': ' + str(e), 'code -22' in str(e))
    torch.cuda.synchronize()
    same_bits(J, what + ' wrote', before, snapshot(P, [R]))
    J.true(what + ' wrote the workspace', torch.equal(ws0, R.ws))


def test_stack_entry_points_refuse_what_they_cannot_take(ops):
    """Every call returns DCAHIP_EINVAL before any launch and writes nothing: every buffer keeps its contents."""
    J = Judge('refusals')
    f = lambda R, P, **kw: ops.hidden_stack_fwd(kw.pop('layers', None) or R.fwd_entries(), kw.pop('B', P.B), MOM, EPS, kw.pop('act', 1),
                                                kw.pop('ws', R.ws), **kw)
    b = lambda R, P, **kw: ops.hidden_stack_bwd(kw.pop('layers', None) or R.bwd_layers(), kw.pop('B', P.B), float(P.B), kw.pop('act', 1),
                                                R.dz0(), P.ld[0], kw.pop('ws', R.ws), **kw)
    P = Prob(S3, 100, 1, 5)
    R = Rank(ops, P, 0, 100)
    n = P.n
    for name, fn, last in (('fwd', f, n), ('bwd', b, n + 1)):
        for rows in (15, 65):
            _refused(ops, J, '%s rows_per_wg %d' % (name, rows), P, R, lambda: fn(R, P, rows_per_wg=rows, steps=(0, 0)))
        _refused(ops, J, name + ' first > last', P, R, lambda: fn(R, P, rows_per_wg=32, steps=(2, 1)))
        _refused(ops, J, name + ' last step beyond the pass', P, R, lambda: fn(R, P, rows_per_wg=32, steps=(last + 1, last + 1)))
        _refused(ops, J, name + ' workspace one byte short', P, R, lambda: fn(R, P, rows_per_wg=32, steps=(0, 0), ws=R.ws[:R.nbytes - 1]))
        big = torch.zeros(R.nbytes + 16, dtype=torch.uint8, device='cuda')
        _refused(ops, J, name + ' workspace 4 bytes off', P, R, lambda: fn(R, P, rows_per_wg=32, steps=(0, 0), ws=big[4:4 + R.nbytes]))
        J.true('the shifted workspace stayed zero', bool((big == 0).all()))
    _refused(ops, J, 'fwd NULL workspace of the right size', P, R, lambda: f(R, P, rows_per_wg=32, steps=(0, 0), ws=_NullTensor(R.nbytes)))
    _refused(ops, J, 'bwd NULL workspace of the right size', P, R, lambda: b(R, P, rows_per_wg=32, steps=(1, 1), ws=_NullTensor(R.nbytes)))
    _refused(ops, J, 'fwd empty workspace', P, R, lambda: f(R, P, rows_per_wg=32, steps=(0, 0), ws=torch.empty(0, dtype=torch.uint8, device='cuda')))
    _refused(ops, J, 'bwd NULL workspace, single step', P, R, lambda: b(R, P, rows_per_wg=32, steps=(1, 1), ws=None))
    _refused(ops, J, 'bwd NULL workspace, B > 64', P, R, lambda: b(R, P, rows_per_wg=64, ws=None))

    def without(layers, i, key):
        layers[i] = {k: v for k, v in layers[i].items() if k != key}
        return layers
    _refused(ops, J, 'bwd code 12 without beta', P, R, lambda: b(R, P, rows_per_wg=32, steps=(0, 0), act=12, layers=without(R.bwd_layers(), 1, 'beta')))
    _refused(ops, J, 'fwd single step, layer 1 without Z', P, R, lambda: f(R, P, rows_per_wg=32, steps=(1, 1), layers=without(R.fwd_entries(), 1, 'Z')))
    wrongK = R.fwd_entries(); wrongK[2]['K'] = 31
    _refused(ops, J, 'fwd K != previous H', P, R, lambda: f(R, P, rows_per_wg=32, steps=(0, 0), layers=wrongK))
    wrongK = R.bwd_layers(); wrongK[2]['K'] = 31
    _refused(ops, J, 'bwd K != previous H', P, R, lambda: b(R, P, rows_per_wg=32, steps=(0, 0), layers=wrongK))
    _refused(ops, J, 'fwd B = 0', P, R, lambda: f(R, P, B=0, rows_per_wg=32, steps=(0, 0)))
    _refused(ops, J, 'bwd B = 0', P, R, lambda: b(R, P, B=0, rows_per_wg=32, steps=(0, 0)))
    _refused(ops, J, 'fwd n = 0', P, R, lambda: ops.hidden_stack_fwd([], P.B, MOM, EPS, 1, R.ws, rows_per_wg=32, steps=(0, 0)))
    _refused(ops, J, 'bwd n = 0', P, R, lambda: ops.hidden_stack_bwd([], P.B, float(P.B), 1, R.dz0(), P.ld[0], R.ws, rows_per_wg=32, steps=(0, 0)))
    ext = (torch.zeros(1, 2, 64, **F32), torch.full((1,), 100.0, **F32))
    _refused(ops, J, 'fwd_sync step > n', P, R, lambda: ops.hidden_stack_fwd_sync(R.fwd_entries(), P.B, MOM, EPS, 1, n + 1, ext[0], ext[1], 1, None, R.ws))
    _refused(ops, J, 'fwd_sync step > 0 without entries', P, R, lambda: ops.hidden_stack_fwd_sync(R.fwd_entries(), P.B, MOM, EPS, 1, 1, None, None, 0, R.stat_out[1], R.ws))
    _refused(ops, J, 'bwd_sync step > n', P, R, lambda: ops.hidden_stack_bwd_sync(R.bwd_layers(), P.B, float(P.B), 1, R.dz0(), P.ld[0], n + 1, torch.zeros(2, 64, **F32), None, R.ws))
    _refused(ops, J, 'fwd_sync B = 0', P, R, lambda: ops.hidden_stack_fwd_sync(R.fwd_entries(), 0, MOM, EPS, 1, 0, None, None, 0, R.stat_out[0], R.ws))
    _refused(ops, J, 'bwd_sync B = 0', P, R, lambda: ops.hidden_stack_bwd_sync(R.bwd_layers(), 0, float(P.B), 1, R.dz0(), P.ld[0], 0, None, R.sums_out[n - 1], R.ws))
    _refused(ops, J, 'fwd_sync NULL workspace', P, R, lambda: ops.hidden_stack_fwd_sync(R.fwd_entries(), P.B, MOM, EPS, 1, 0, None, None, 0, R.stat_out[0], _NullTensor(R.nbytes)))
    _refused(ops, J, 'bwd_sync NULL workspace', P, R, lambda: ops.hidden_stack_bwd_sync(R.bwd_layers(), P.B, float(P.B), 1, R.dz0(), P.ld[0], 0, None, R.sums_out[n - 1], _NullTensor(R.nbytes)))
    _refused(ops, J, 'bwd_sync step > 0 without sums', P, R, lambda: ops.hidden_stack_bwd_sync(R.bwd_layers(), P.B, float(P.B), 1, R.dz0(), P.ld[0], 1, None, R.sums_out[1], R.ws))
    # nine layers; a layer wider than 64 (the workspace is sized for a stack the entry points do take)
    for name, hs in (('n = 9', (8,) * 9), ('a layer of 65 units', (64, 65, 64))):
        Pn = Prob(hs, 100, 1, 6)
        Rn = Rank(ops, Pn, 0, 100)
        Rn.ws = torch.zeros(ops.hidden_stack_workspace_bytes(8, 100), dtype=torch.uint8, device='cuda')
        _refused(ops, J, 'fwd ' + name, Pn, Rn, lambda: f(Rn, Pn, rows_per_wg=32, steps=(0, 0)))
        _refused(ops, J, 'bwd ' + name, Pn, Rn, lambda: b(Rn, Pn, rows_per_wg=32, steps=(0, 0)))
    # a range of steps whose grid would exceed 256 workgroups; a batch above hidden_stack_max_rows (buffers of the full size)
    Pb = Prob(S3, 5000, 1, 7)
    Rb = Rank(ops, Pb, 0, 5000)
    _refused(ops, J, 'fwd steps (0, 1) over 313 workgroups', Pb, Rb, lambda: f(Rb, Pb, rows_per_wg=16, steps=(0, 1)))
    _refused(ops, J, 'bwd steps (0, 1) over 313 workgroups', Pb, Rb, lambda: b(Rb, Pb, rows_per_wg=16, steps=(0, 1)))
    Bx = ops.hidden_stack_max_rows + 1
    assert ops.hidden_stack_workspace_bytes(3, Bx) == 0
    Px = Prob(S3, Bx, 1, 8)
    Rx = Rank(ops, Px, 0, Bx)
    Rx.ws = torch.zeros(ops.hidden_stack_workspace_bytes(3, Bx - 1), dtype=torch.uint8, device='cuda')
    _refused(ops, J, 'fwd B above hidden_stack_max_rows', Px, Rx, lambda: f(Rx, Px, rows_per_wg=64, steps=(0, 0)))
    _refused(ops, J, 'bwd B above hidden_stack_max_rows', Px, Rx, lambda: b(Rx, Px, rows_per_wg=64, steps=(0, 0)))
    J.report()
