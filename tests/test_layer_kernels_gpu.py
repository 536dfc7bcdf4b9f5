"""The per-operation hidden-layer kernels of dca_amd/csrc/dcahip_layers.hip -- what the engine runs when the fused stack
(K-STACK) does not apply: a layer wider than 64 units, batch norm off, dropout / PReLU on, a data-parallel step, the
reference-default batch of 32 -- against the fp64 reference tests/_stack_ref.py, through HipOps:

  (a) col_moments, moments_combine, bn_relu_apply (training with chunk entries, with counted entries, B == 0, inference)
  (b) bn_bwd_sums, bn_bwd_apply (also with n_total != B and one external sums entry: the data-parallel form)
  (c) bn_relu_train_small, bn_bwd_small, dense_bn_small, dense_bn_bwd_small, hidden_small_chain (B <= 64, one launch each)
  (d) relu_fwd, relu_bwd          (e) colsum_chain

Conventions.  Every matrix has rows of ld = H + (-H) % 4 + 4 floats and one extra row; pad columns, the extra row and every
output hold the sentinel 7.0 before the launch and the pads are asserted intact after it; vectors carry three sentinel
elements behind their end.  Every element of every output is compared: nothing is masked or dropped.

Teacher forcing.  Each launch is compared with the reference evaluated on the fp32 operands THAT launch read; a launch that
consumes another's output is judged on what was read back from the device (the chunk entries, the chunk sums, a stored Z or
Hout).  So every tolerance is that of one kernel, and a relu mask cannot flip between kernel and reference.

Tolerances (none derived from a kernel's output):
  * elementwise outputs: the flat classes of tests/_judge.py (H, xhat: rtol = atol = 2e-5; inv_std rtol 1e-5; moving
    statistics rtol 1e-5, atol 1e-6) -- in the forward tests plus the first-order effect of t_mean / t_M2
    (_stack_ref.moments_tolerance / entries_tolerance / fwd_bounds): an fp32 mean carries ulp32(mean) however it is formed,
    which on a column of mean 3000 and spread 0.3 is 20 x the flat class of xhat; on ordinary columns the terms vanish
    beside the flat classes.  A one-pass E[x^2] - E[x]^2 variance would miss these bounds by orders of magnitude;
  * reductions and products (chunk statistics and sums, dbeta, dZ, Z = Hp W + b, gW with its bias row, dHp):
    |err| <= 1e-6 * sum |terms| + the allowance for what enters already rounded (_stack_ref: X_mag, X_in);
  * colsum_chain: each of the 4 row lanes adds m = ceil(B / 4) terms one after the other in fp32, so the a-priori bound is
    ((m + 2) 2^-24 + 1e-6) * sum |x| per column (1e-6 alone is the TYPICAL error of such a sum at m = 1025); the chain factor
    is exp(theta) to 1e-6 relative inside the clip [1e-3, 1e4] and exactly 0 outside.
Conditions on the inputs (asserted on the host, on the operands a launch reads, before anything is compared;
tests/_layer_cases.py): hard_sigmoid keeps 1e-4 away from its kink (the kernel's 0.2f moves it by 4e-8); exponential keeps
|x| < 40; in backward tests of codes 1 and 8, whose mask is taken from the stored h, no h has underflowed; on the
conditioned columns no pre-activation of relu lies within the column's allowance of 0.  A seed that violates one is
replaced, never filtered.
A second run from the same inputs must reproduce every output bit for bit.  Every test prints its worst error / bound
per output class before it asserts."""
import functools

import numpy as np
import pytest
import torch

import _layer_cases as LC
import _stack_ref as SR
from _judge import EL, Judge

pytestmark = pytest.mark.gpu

SENT = 7.0
MOM, EPS = 0.99, 1e-3
F32 = dict(dtype=torch.float32, device='cuda')
RELU, TANH, SELU = 1, 2, 5
ALL = SR.CODES


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _ld(h):
    return h + (-h) % 4 + 4


def host(t):
    return t.detach().cpu().double().numpy()


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def mat(B, H, a=None, ld=None):
    """[B + 1, ld] of the sentinel with a (fp32) in its first B rows / H columns."""
    t = torch.full((B + 1, ld or _ld(H)), SENT, **F32)
    if a is not None:
        t[:B, :H] = torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()
    return t


def vec(n, a=None):
    t = torch.full((n + 3,), SENT, **F32)
    if a is not None:
        t[:n] = torch.as_tensor(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
    return t


def body(t, B, H):
    return host(t)[:B, :H]


def pads_intact(J, name, t, B, H):
    J.true('pad columns of ' + name, bool((t[:, H:] == SENT).all()))
    J.true('extra row of ' + name, bool((t[B:] == SENT).all()))


def tail_intact(J, name, t, n):
    J.true('tail of ' + name, bool((t[n:] == SENT).all()))


def untouched(J, name, t):
    J.true(name + ' left at the sentinel', bool((t == SENT).all()))


def bits(J, what, a, b):
    for k in a:
        J.true('%s: %s bit for bit' % (what, k), torch.equal(a[k], b[k]))


def codes_id(c):
    return 'act%d' % c


# ------------------------------------------------------------------ (a) col_moments + bn_relu_apply
def _apply_bounds(J, tag, o, code, beta, t_mean, t_m2, n, got, train=True):
    bnd = SR.fwd_bounds(o, code, beta, t_mean, t_m2, n, EL)
    keys = ('xhat', 'H', 'inv_std', 'mm', 'mv') if train else ('xhat', 'H', 'inv_std')
    for k in keys:
        if got.get(k) is not None:
            J.bound('%s %s' % (tag, k), tag, np.abs(got[k] - o[k]), bnd[k])


def _launch_apply(ops, Z, B, H, entries, counts, E, beta, mm0, mv0, code, xhat=True, inv=True):
    ld = _ld(H)
    o = dict(H=mat(B, H), xhat=mat(B, H), inv_std=vec(H), mm=vec(H, mm0), mv=vec(H, mv0))
    ops.bn_relu_apply(Z, ld, B, H, entries, counts, E, beta, o['mm'], o['mv'], MOM, EPS, code, o['H'], ld,
                      o['xhat'] if xhat else None, ld, o['inv_std'] if inv else None)
    torch.cuda.synchronize()
    return o


def _read_apply(o, B, H):
    return dict(xhat=body(o['xhat'], B, H), H=body(o['H'], B, H), inv_std=host(o['inv_std'])[:H], mm=host(o['mm'])[:H],
                mv=host(o['mv'])[:H])


def _check_apply_pads(J, o, B, H):
    pads_intact(J, 'Hout', o['H'], B, H)
    pads_intact(J, 'xhat', o['xhat'], B, H)
    for k in ('inv_std', 'mm', 'mv'):
        tail_intact(J, k, o[k], H)


FWD_CASES = [pytest.param(65, 20, c, False, id='65x20-act%d' % c) for c in ALL]
FWD_CASES += [pytest.param(B, H, c, False, id='%dx%d-act%d' % (B, H, c)) for B, H in LC.LARGE_SHAPES[1:] for c in (RELU, TANH)]
FWD_CASES += [pytest.param(B, H, c, True, id='%dx%d-act%d-conditioned' % (B, H, c)) for B, H in LC.COND_SHAPES for c in (0, RELU)]


@pytest.mark.parametrize('B,H,code,conditioned', FWD_CASES)
def test_col_moments_and_bn_relu_apply(ops, B, H, code, conditioned):
    """dcahip_col_moments, then dcahip_bn_relu_apply on its chunk entries (counts NULL: the chunk partition).  The chunk
    (mean, M2) against range_stats over the kernel's own chunk ranges; xhat, H, inv_std and the moving statistics against
    fwd_step (i) on the entries the kernel itself wrote and (ii) on the statistics of Z itself (both launches end to end),
    under the same bounds; H is bit-identical without xhat / inv_std; inference (entries NULL) normalises with the moving
    statistics and leaves them bit-unchanged."""
    J = Judge('(a) %d x %d act=%d%s' % (B, H, code, ' conditioned' if conditioned else ''))
    p = LC.large_fwd_problem(B, H, conditioned)
    ld = _ld(H)
    Z64, beta64, mm64, mv64 = (f64(p[k]) for k in ('Z', 'beta', 'mm0', 'mv0'))
    R = ops.col_moments_chunks(B)
    ranges = SR.chunk_ranges(B, R)
    assert ranges == SR.chunk_ranges(B)
    cnt = [b - a for a, b in ranges]
    st, g = SR.range_stats(Z64, ranges), SR.range_stats(Z64, [(0, B)])
    t_mean, t_m2 = SR.moments_tolerance(st, g)
    o2 = SR.fwd_step(1, Z64, [B], g['mean'], g['m2'], beta64, None, None, mm64, mv64, code)
    LC.fwd_conditions(code, o2['xhat'] + beta64, o2['inv_std'] * t_mean)
    oi = {'inv_std': 1.0 / np.sqrt(mv64 + EPS)}
    oi['xhat'] = (Z64 - mm64) * oi['inv_std']
    oi['H'] = SR.act_fwd(code, oi['xhat'] + beta64)
    LC.fwd_conditions(code, oi['xhat'] + beta64)

    Z, beta = mat(B, H, p['Z']), vec(H, p['beta'])
    runs = []
    for _ in range(2):
        part = vec(R * 2 * H)
        ops.col_moments(Z, ld, B, H, part)
        runs.append((part, _launch_apply(ops, Z, B, H, part, None, R, beta, p['mm0'], p['mv0'], code)))
    part, o = runs[0]
    bits(J, 'second run', dict(o, part=part), dict(runs[1][1], part=runs[1][0]))
    got_part = host(part)[:R * 2 * H].reshape(R, 2, H)
    tail_intact(J, 'part', part, R * 2 * H)
    J.bound('chunk mean', 'col_moments', np.abs(got_part[:, 0] - st['mean']), SR.REL * st['mean_mag'])
    J.bound('chunk M2', 'col_moments', np.abs(got_part[:, 1] - st['m2']), SR.REL * st['m2_mag'] + st['m2_in'])
    got = _read_apply(o, B, H)
    o1 = SR.fwd_step(1, Z64, cnt, got_part[:, 0], got_part[:, 1], beta64, None, None, mm64, mv64, code)
    _apply_bounds(J, 'forced', o1, code, beta64, t_mean, t_m2, B, got)
    _apply_bounds(J, 'end to end', o2, code, beta64, t_mean, t_m2, B, got)
    _check_apply_pads(J, o, B, H)
    J.true('Z unchanged', torch.equal(Z, mat(B, H, p['Z'])))
    # without xhat / without inv_std: the same H, nothing written in their place
    for kw in (dict(xhat=False), dict(inv=False)):
        v = _launch_apply(ops, Z, B, H, part, None, R, beta, p['mm0'], p['mv0'], code, **kw)
        J.true('H bit for bit with %s' % kw, torch.equal(v['H'], o['H']) and torch.equal(v['mm'], o['mm']) and torch.equal(v['mv'], o['mv']))
        untouched(J, 'the absent output of %s' % kw, v['xhat'] if 'xhat' in kw else v['inv_std'])
    v = _launch_apply(ops, Z, B, H, None, None, 0, beta, p['mm0'], p['mv0'], code)
    _apply_bounds(J, 'inference', oi, code, beta64, 0.0, 0.0, B, _read_apply(v, B, H), train=False)
    J.true('inference leaves mm / mv bit-unchanged', torch.equal(v['mm'], vec(H, p['mm0'])) and torch.equal(v['mv'], vec(H, p['mv0'])))
    _check_apply_pads(J, v, B, H)
    J.report()


@functools.lru_cache(maxsize=None)
def _entries_problem(E, H=70):
    """E entries (count, mean, M2) of consecutive row ranges of one matrix, rounded to fp32 -- the merge's exact inputs;
    unequal counts, and for E > 1 one entry of count 0 that holds finite junk (mean 3, M2 5)."""
    rng = np.random.RandomState(500 + E)
    counts = [int(c) for c in rng.randint(1, 7, size=E)]
    if E > 1:
        counts[E // 2] = 0
    if E == 1:
        counts = [41]
    N = sum(counts)
    Zall = f64(rng.normal(size=(N, H)) * 1.5 + rng.normal(size=H))
    s = SR.range_stats(Zall, SR.split_ranges(counts))
    ent = np.stack([s['mean'], s['m2']], 1).astype(np.float32)             # [E, 2, H]
    if E > 1:
        ent[E // 2, 0], ent[E // 2, 1] = 3.0, 5.0
    return counts, Zall, ent


@pytest.mark.parametrize('E', [1, 3, 17, 256])
def test_moments_combine(ops, E):
    """dcahip_moments_combine (merge_entries_wg: 16 entries per trip of a workgroup) against merge_stats of the same fp32
    entries: two column blocks, the second ragged; one to 16 trips; a zero-count entry with junk is ignored."""
    H = 70
    J = Judge('(a) moments_combine E=%d H=%d' % (E, H))
    counts, _, ent = _entries_problem(E)
    e64 = ent.astype(np.float64)
    n, gm, gq = SR.merge_stats(counts, e64[:, 0], e64[:, 1])
    t_mean, t_m2 = SR.entries_tolerance(counts, e64[:, 0], e64[:, 1])
    entd, cntd = vec(E * 2 * H, ent), vec(E, np.float32(counts))
    outs = []
    for _ in range(2):
        out = vec(2 * H)
        ops.moments_combine(entd, cntd, E, H, out)
        torch.cuda.synchronize()
        outs.append(out)
    J.true('second run bit for bit', torch.equal(outs[0], outs[1]))
    got = host(outs[0])
    J.bound('mean', 'merged mean', np.abs(got[:H] - gm), t_mean)
    J.bound('M2', 'merged M2', np.abs(got[H:2 * H] - gq), t_m2)
    tail_intact(J, 'out', outs[0], 2 * H)
    J.true('entries / counts unchanged', torch.equal(entd, vec(E * 2 * H, ent)) and torch.equal(cntd, vec(E, np.float32(counts))))
    J.report()


RANKS = [40, 0, 90]


@functools.lru_cache(maxsize=None)
def _rank_problem(H=70):
    rng = np.random.RandomState(77)
    N = sum(RANKS)
    p = dict(Z=LC.f32(rng.normal(size=(N, H)) * 1.5 + rng.normal(size=H)), beta=LC.f32(rng.normal(size=H) * 0.3),
             mm0=LC.f32(rng.normal(size=H) * 0.1), mv0=LC.f32(rng.uniform(0.5, 1.5, size=H)))
    s = SR.range_stats(f64(p['Z']), SR.split_ranges(RANKS))
    ent = np.stack([s['mean'], s['m2']], 1).astype(np.float32)
    ent[1, 0], ent[1, 1] = 3.0, 5.0
    p['ent'] = ent
    return p


@pytest.mark.parametrize('B', [40, 0], ids=['rank0', 'empty-rank'])
def test_bn_relu_apply_with_counted_entries(ops, B):
    """dcahip_bn_relu_apply as a data-parallel rank calls it: three entries with explicit counts (one 0, holding junk), the
    rank's own rows normalised with the statistics of the union.  B == 0 (the header: legal, only the moving statistics are
    updated; Engine._empty_step): mm / mv / inv_std as for any rank, Hout and xhat untouched.  Z is a view that starts at
    row 1 of a larger tensor, so that a read in front of it stays inside an allocation."""
    H, code = 70, RELU
    J = Judge('(a) bn_relu_apply counted entries B=%d' % B)
    p = _rank_problem()
    e64 = p['ent'].astype(np.float64)
    beta64, mm64, mv64 = (f64(p[k]) for k in ('beta', 'mm0', 'mv0'))
    t_mean, t_m2 = SR.entries_tolerance(RANKS, e64[:, 0], e64[:, 1])
    Zr = f64(p['Z'][:B])
    o = SR.fwd_step(1, Zr.reshape(B, H), RANKS, e64[:, 0], e64[:, 1], beta64, None, None, mm64, mv64, code)
    LC.fwd_conditions(code, o['xhat'] + beta64)
    big = torch.full((B + 3, _ld(H)), SENT, **F32)
    big[1:1 + B, :H] = torch.as_tensor(p['Z'][:B]).cuda()
    Z = big[1:]
    assert Z.data_ptr() == big.data_ptr() + 4 * _ld(H)
    entd, cntd, beta = vec(3 * 2 * H, p['ent']), vec(3, np.float32(RANKS)), vec(H, p['beta'])
    runs = [_launch_apply(ops, Z, B, H, entd, cntd, 3, beta, p['mm0'], p['mv0'], code) for _ in range(2)]
    bits(J, 'second run', runs[0], runs[1])
    got = _read_apply(runs[0], B, H)
    _apply_bounds(J, 'ranks', o, code, beta64, t_mean, t_m2, float(sum(RANKS)), got)
    _check_apply_pads(J, runs[0], B, H)
    if B == 0:
        untouched(J, 'Hout', runs[0]['H'])
        untouched(J, 'xhat', runs[0]['xhat'])
        J.true('mm / mv moved', bool((runs[0]['mm'][:H] != vec(H, p['mm0'])[:H]).any()))
    J.report()


# ------------------------------------------------------------------ (b) bn_bwd_sums + bn_bwd_apply
BWD_CASES = [pytest.param(65, 20, c, 1, id='65x20-act%d' % c) for c in ALL]
BWD_CASES += [pytest.param(B, H, c, 1, id='%dx%d-act%d' % (B, H, c)) for B, H in LC.LARGE_SHAPES[2:] for c in (RELU, TANH)]
BWD_CASES += [pytest.param(130, 64, RELU, 2, id='130x64-act1-n_total-2B-external-sums')]


@pytest.mark.parametrize('B,H,code,dp', BWD_CASES)
def test_bn_bwd_sums_and_apply(ops, B, H, code, dp):
    """dcahip_bn_bwd_sums (chunk sums against bwd_step 0 over the kernel's chunk ranges), then dcahip_bn_bwd_apply on the
    sums read back: dbeta = their fp32 total, dZ against bwd_step 1.  dp = 2: the data-parallel form -- n_total = 2 B and
    ONE external entry of all-reduced sums, used as handed in."""
    J = Judge('(b) %d x %d act=%d%s' % (B, H, code, ' n_total=2B' if dp == 2 else ''))
    p = LC.bwd_problem(B, H, code)
    ld = _ld(H)
    R = ops.col_moments_chunks(B)
    ranges = SR.chunk_ranges(B, R)
    o0 = SR.bwd_step(0, p['dH'], p['Hact'], p['xhat'], beta=p['beta'], act=code, ranges=ranges)
    dH, Hact, xhat = mat(B, H, p['dH']), mat(B, H, p['Hact']), mat(B, H, p['xhat'])
    inv, beta = vec(H, p['inv_std']), vec(H, p['beta'])
    n_total = float(dp * B)
    ext = None
    if dp == 2:                                          # the sums of "both ranks": any fp32 numbers of the right size
        tot = o0['sums'].sum(0)
        ext = vec(2 * H, np.float32(2.0 * tot + 0.25))
    runs = []
    for _ in range(2):
        part, dZ, dbeta = vec(R * 2 * H), mat(B, H), vec(H)
        ops.bn_bwd_sums(dH, ld, Hact, ld, xhat, ld, B, H, part, code, beta)
        if ext is None:
            ops.bn_bwd_apply(dH, ld, Hact, ld, xhat, ld, inv, part, R, n_total, B, H, dZ, ld, dbeta, code, beta)
        else:
            ops.bn_bwd_apply(dH, ld, Hact, ld, xhat, ld, inv, ext, 1, n_total, B, H, dZ, ld, dbeta, code, beta)
        torch.cuda.synchronize()
        runs.append(dict(part=part, dZ=dZ, dbeta=dbeta))
    bits(J, 'second run', runs[0], runs[1])
    r = runs[0]
    pp = host(r['part'])[:R * 2 * H].reshape(R, 2, H)
    J.red('chunk sums', 'bn_bwd_sums', o0, 'sums', pp)
    if ext is None:
        S, S_tol = pp.sum(0), SR.REL * np.abs(pp).sum(0)                  # the kernel adds the chunks' sums in fp32
    else:
        S, S_tol = host(ext)[:2 * H].reshape(2, H), np.zeros((2, H))      # one entry: taken as it is
    J.bound('dbeta', 'dbeta', np.abs(host(r['dbeta'])[:H] - S[0]), S_tol[0])
    o = SR.bwd_step(1, p['dH'], p['Hact'], p['xhat'], p['inv_std'], p['beta'], S[0], S[1], n_total, act=code,
                    S_tol=(S_tol[0], S_tol[1]))
    J.red('dZ', 'bn_bwd_apply', o, 'dZ', body(r['dZ'], B, H))
    pads_intact(J, 'dZ', r['dZ'], B, H)
    tail_intact(J, 'part', r['part'], R * 2 * H)
    tail_intact(J, 'dbeta', r['dbeta'], H)
    J.true('inputs unchanged', torch.equal(dH, mat(B, H, p['dH'])) and torch.equal(Hact, mat(B, H, p['Hact'])) and
           torch.equal(xhat, mat(B, H, p['xhat'])))
    J.report()


# ------------------------------------------------------------------ (c) single-launch kernels, B <= 64
SMALL_B = (1, 5, 32, 33, 64)


def _small_fwd_problem(B, H, K=0, seed=0, tame=False):
    """tame: inputs and kernels small enough for a chain of exponentials without batch norm to stay far inside fp32."""
    rng = np.random.RandomState(6000 + 100 * B + H + 7 * K + seed)
    zs, ws = (0.2, 0.03) if tame else (1.5, 0.3)
    p = dict(beta=LC.f32(rng.normal(size=H) * 0.3), mm0=LC.f32(rng.normal(size=H) * 0.1), mv0=LC.f32(rng.uniform(0.5, 1.5, size=H)))
    if K:
        p.update(Hp=LC.f32(rng.normal(size=(B, K))), W=LC.f32(rng.normal(size=(K, H)) * ws), bias=LC.f32(rng.normal(size=H) * 0.1))
    else:
        p['Z'] = LC.f32(rng.normal(size=(B, H)) * zs + rng.normal(size=H) * zs / 1.5)
    return p


def _judge_bn_layer(J, tag, Zgot, p, code, got, B, H):
    """xhat / H / inv_std / mm / mv of a layer that forms its own statistics in fp32, against fwd_step on the Z it read."""
    Z64 = np.asarray(Zgot, np.float64)
    g = SR.range_stats(Z64, [(0, B)])
    t_mean, t_m2 = SR.moments_tolerance(g, g)
    beta64 = f64(p['beta'])
    o = SR.fwd_step(1, Z64, [B], g['mean'], g['m2'], beta64, None, None, f64(p['mm0']), f64(p['mv0']), code)
    LC.fwd_conditions(code, o['xhat'] + beta64)
    _apply_bounds(J, tag, o, code, beta64, t_mean, t_m2, B, got)


SMALL_BN_CASES = [pytest.param(33, 12, c, id='B33-H12-act%d' % c) for c in ALL]
SMALL_BN_CASES += [pytest.param(B, H, c, id='B%d-H%d-act%d' % (B, H, c)) for B in SMALL_B for H in (12, 64, 70) for c in (RELU, SELU)
                   if (B, H) != (33, 12)]


@pytest.mark.parametrize('B,H,code', SMALL_BN_CASES)
def test_bn_relu_train_small(ops, B, H, code):
    """dcahip_bn_relu_train_small (both template instances and their edges; H = 70: two workgroups, the second ragged)."""
    J = Judge('(c) bn_relu_train_small B=%d H=%d act=%d' % (B, H, code))
    p = _small_fwd_problem(B, H)
    ld = _ld(H)
    Z, beta = mat(B, H, p['Z']), vec(H, p['beta'])
    runs = []
    for _ in range(2):
        o = dict(H=mat(B, H), xhat=mat(B, H), inv_std=vec(H), mm=vec(H, p['mm0']), mv=vec(H, p['mv0']))
        ops.bn_relu_train_small(Z, ld, B, H, beta, o['mm'], o['mv'], MOM, EPS, code, o['H'], ld, o['xhat'], ld, o['inv_std'])
        torch.cuda.synchronize()
        runs.append(o)
    bits(J, 'second run', runs[0], runs[1])
    _judge_bn_layer(J, 'bn', f64(p['Z']), p, code, _read_apply(runs[0], B, H), B, H)
    _check_apply_pads(J, runs[0], B, H)
    v = dict(H=mat(B, H), mm=vec(H, p['mm0']), mv=vec(H, p['mv0']))
    ops.bn_relu_train_small(Z, ld, B, H, beta, v['mm'], v['mv'], MOM, EPS, code, v['H'], ld, None, ld, None)
    torch.cuda.synchronize()
    bits(J, 'without xhat / inv_std', v, {k: runs[0][k] for k in v})
    J.report()


SMALL_BWD_CASES = [pytest.param(33, 12, c, id='B33-H12-act%d' % c) for c in ALL]
SMALL_BWD_CASES += [pytest.param(B, H, c, id='B%d-H%d-act%d' % (B, H, c)) for B in SMALL_B[1:] for H in (12, 64, 70) for c in (RELU, SELU)
                    if (B, H) != (33, 12)]


def _bwd_reference(p, n_total):
    """bwd_step 1 with the batch sums of the fp64 pass and their allowance (the kernel adds them up in fp32)."""
    args = (p['dH'], p['Hact'], p['xhat'])
    o0 = SR.bwd_step(0, *args, beta=p['beta'], act=p['code'])
    tol = SR.REL * o0['sums_mag'][0] + o0['sums_in'][0]
    return SR.bwd_step(1, *args, p['inv_std'], p['beta'], o0['sums'][0, 0], o0['sums'][0, 1], n_total, p.get('Hp'), p.get('W'),
                       None, p['code'], None, 0.0, (tol[0], tol[1]))


@pytest.mark.parametrize('B,H,code', SMALL_BWD_CASES)
def test_bn_bwd_small(ops, B, H, code):
    J = Judge('(c) bn_bwd_small B=%d H=%d act=%d' % (B, H, code))
    p = LC.bwd_problem(B, H, code)
    ld = _ld(H)
    dH, Hact, xhat = mat(B, H, p['dH']), mat(B, H, p['Hact']), mat(B, H, p['xhat'])
    inv, beta = vec(H, p['inv_std']), vec(H, p['beta'])
    runs = []
    for _ in range(2):
        o = dict(dZ=mat(B, H), dbeta=vec(H))
        ops.bn_bwd_small(dH, ld, Hact, ld, xhat, ld, inv, float(B), B, H, o['dZ'], ld, o['dbeta'], code, beta)
        torch.cuda.synchronize()
        runs.append(o)
    bits(J, 'second run', runs[0], runs[1])
    ref = _bwd_reference(p, float(B))
    J.red('dbeta', 'dbeta', ref, 'dbeta', host(runs[0]['dbeta'])[:H])
    J.red('dZ', 'dZ', ref, 'dZ', body(runs[0]['dZ'], B, H))
    pads_intact(J, 'dZ', runs[0]['dZ'], B, H)
    tail_intact(J, 'dbeta', runs[0]['dbeta'], H)
    J.report()


def _launch_dense(ops, p, B, K, H, bn, code, with_z=True):
    ld, ldk = _ld(H), _ld(K)
    Hp, W, bias, beta = mat(B, K, p['Hp']), mat(K, H, p['W']), vec(H, p['bias']), vec(H, p['beta'])
    o = dict(Z=mat(B, H), H=mat(B, H), xhat=mat(B, H), inv_std=vec(H), mm=vec(H, p['mm0']), mv=vec(H, p['mv0']))
    ops.dense_bn_small(Hp, ldk, W, ld, bias, B, K, H, bn, beta if bn else None, o['mm'] if bn else None, o['mv'] if bn else None,
                       MOM, EPS, code, o['Z'] if with_z else None, ld, o['xhat'] if bn else None, ld, o['H'], ld,
                       o['inv_std'] if bn else None)
    torch.cuda.synchronize()
    return o


def _judge_dense(J, tag, o, Hp64, p, B, K, H, bn, code):
    """Z = Hp W + b against the product of the fp32 operands; the rest against the reference on the Z the kernel wrote."""
    W64, b64 = f64(p['W']), f64(p['bias'])
    Zref = Hp64 @ W64 + b64
    Zgot = body(o['Z'], B, H)
    J.bound(tag + ' Z', tag, np.abs(Zgot - Zref), SR.REL * (np.abs(Hp64) @ np.abs(W64) + np.abs(b64)))
    if bn:
        _judge_bn_layer(J, tag, Zgot, p, code, _read_apply(o, B, H), B, H)
    else:
        LC.fwd_conditions(code, Zgot)
        J.elem('H', tag + ' H', body(o['H'], B, H), SR.act_fwd(code, Zgot))
        for k in ('xhat', 'inv_std'):
            untouched(J, tag + ' ' + k, o[k])
        J.true(tag + ' mm / mv unchanged', torch.equal(o['mm'], vec(H, p['mm0'])) and torch.equal(o['mv'], vec(H, p['mv0'])))
    for k in ('Z', 'H', 'xhat'):
        pads_intact(J, tag + ' ' + k, o[k], B, H)
    for k in ('inv_std', 'mm', 'mv'):
        tail_intact(J, tag + ' ' + k, o[k], H)


DENSE_KH = [(20, 12), (7, 70), (64, 64)]
DENSE_CASES = [pytest.param(33, 20, 12, c, bn, id='B33-K20-H12-act%d-bn%d' % (c, bn)) for c in ALL for bn in (1, 0)]
DENSE_CASES += [pytest.param(B, K, H, c, bn, id='B%d-K%d-H%d-act%d-bn%d' % (B, K, H, c, bn)) for B in SMALL_B for K, H in DENSE_KH
                for c in (RELU, SELU) for bn in (1, 0) if (B, K, H) != (33, 20, 12)]


@pytest.mark.parametrize('B,K,H,code,bn', DENSE_CASES)
def test_dense_bn_small(ops, B, K, H, code, bn):
    """dcahip_dense_bn_small: Dense -> (batch norm) -> activation in one launch; K = 7: the K loop rounded up to 8; H = 70: two
    workgroups; Z NULL gives the same outputs bit for bit."""
    J = Judge('(c) dense_bn_small B=%d K=%d H=%d act=%d bn=%d' % (B, K, H, code, bn))
    p = _small_fwd_problem(B, H, K)
    runs = [_launch_dense(ops, p, B, K, H, bn, code) for _ in range(2)]
    bits(J, 'second run', runs[0], runs[1])
    _judge_dense(J, 'dense', runs[0], f64(p['Hp']), p, B, K, H, bn, code)
    v = _launch_dense(ops, p, B, K, H, bn, code, with_z=False)
    untouched(J, 'Z of the run without Z', v['Z'])
    bits(J, 'Z NULL', {k: v[k] for k in v if k != 'Z'}, runs[0])
    J.report()


DBWD_KH = [(20, 12), (7, 33), (64, 64)]
DBWD_CASES = [pytest.param(33, 20, 12, c, bn, id='B33-K20-H12-act%d-bn%d' % (c, bn)) for c in ALL for bn in (1, 0)]
DBWD_CASES += [pytest.param(B, K, H, c, bn, id='B%d-K%d-H%d-act%d-bn%d' % (B, K, H, c, bn)) for B in SMALL_B[1:] for K, H in DBWD_KH
               for c in (RELU, SELU) for bn in (1, 0) if (B, K, H) != (33, 20, 12)]


@pytest.mark.parametrize('B,K,H,code,bn', DBWD_CASES)
def test_dense_bn_bwd_small(ops, B, K, H, code, bn):
    """dcahip_dense_bn_bwd_small: dbeta, gW with its bias row and dHp of one layer.  Without batch norm dZ = dH act'(Z): the
    reference is bwd_step with xhat = Z, beta = 0, inv_std = 1 and zero sums, and codes 12, 13 are handed Z in the Hact slot.
    dHp NULL leaves gW / dbeta bit-identical."""
    J = Judge('(c) dense_bn_bwd_small B=%d K=%d H=%d act=%d bn=%d' % (B, K, H, code, bn))
    p = LC.bwd_problem(B, H, code, K)
    ld, ldk = _ld(H), _ld(K)
    if bn:
        ref = _bwd_reference(p, float(B))
        slot = p['Hact']
    else:                                                # pre-activation Z := xhat + beta of the problem
        z = f64(p['x'])
        hz = f64(SR.act_fwd(code, z))
        LC.bwd_conditions(code, z, hz)
        zero = np.zeros(H)
        ref = SR.bwd_step(1, p['dH'], hz, z, np.ones(H), None, zero, zero, 1.0, p['Hp'], p['W'], None, code)
        slot = z if code >= SR.ACT_PRE else hz
    dH, Hact, xhat = mat(B, H, p['dH']), mat(B, H, slot), mat(B, H, p['xhat'])
    inv, beta = vec(H, p['inv_std']), vec(H, p['beta'])
    Hp, W = mat(B, K, p['Hp']), mat(K, H, p['W'])

    def run(with_dhp):
        o = dict(gW=mat(K + 1, H), dbeta=vec(H), dHp=mat(B, K))
        ops.dense_bn_bwd_small(dH, ld, Hact, ld, xhat if bn else None, ld, inv if bn else None, Hp, ldk, W, ld, B, K, H, bn, float(B),
                               code, o['gW'], ld, o['dbeta'], o['dHp'] if with_dhp else None, ldk, beta if bn else None)
        torch.cuda.synchronize()
        return o
    runs = [run(True), run(True)]
    bits(J, 'second run', runs[0], runs[1])
    o = runs[0]
    if bn:
        J.red('dbeta', 'dbeta', ref, 'dbeta', host(o['dbeta'])[:H])
    else:
        untouched(J, 'dbeta without batch norm', o['dbeta'])
    J.red('gW', 'gW', ref, 'gW', body(o['gW'], K + 1, H))
    J.red('dHp', 'dHp', ref, 'dHprev', body(o['dHp'], B, K))
    pads_intact(J, 'gW', o['gW'], K + 1, H)
    pads_intact(J, 'dHp', o['dHp'], B, K)
    tail_intact(J, 'dbeta', o['dbeta'], H)
    v = run(False)
    untouched(J, 'dHp of the run without dHp', v['dHp'])
    bits(J, 'dHp NULL', {k: v[k] for k in ('gW', 'dbeta')}, o)
    J.report()


S3, S4 = (64, 32, 64), (48, 20, 7, 33)
CHAIN_CASES = [pytest.param(S3, 33, c, bn, 0, id='64x32x64-B33-act%d-bn%d' % (c, bn)) for c in ALL for bn in (1, 0)]
CHAIN_CASES += [pytest.param(hs, B, RELU, bn, 0, id='%s-B%d-act1-bn%d' % ('x'.join(map(str, hs)), B, bn))
                for hs in (S3, S4, (16, 8), (10,)) for B in SMALL_B for bn in (1, 0) if (hs, B) != (S3, 33)]
CHAIN_CASES += [pytest.param(S3, B, c, bn, 20, id='Hin20-64x32x64-B%d-act%d-bn%d' % (B, c, bn)) for B in (32, 33) for c in (RELU, 12)
                for bn in (1, 0)]


@pytest.mark.parametrize('hs,B,code,bn,K0', CHAIN_CASES)
def test_hidden_small_chain_forward(ops, hs, B, code, bn, K0):
    """dcahip_hidden_small_chain: every layer teacher-forced from the Hout / Z the chain itself stored, and the whole result
    bit for bit that of the per-layer kernels (the header: same formulas and outputs as dcahip_bn_relu_train_small /
    dcahip_dense_bn_small one after the other; without batch norm entry 0 without a kernel is dcahip_relu_fwd).
    K0 > 0: entry 0 has a kernel and reads Hin [B, K0] -- the header's other form."""
    J = Judge('(c) hidden_small_chain %s B=%d act=%d bn=%d K0=%d' % (hs, B, code, bn, K0))
    n = len(hs)
    Ks = [K0] + list(hs[:-1])
    ps = [_small_fwd_problem(B, hs[i], Ks[i], seed=31 * i + code, tame=code == 11 and not bn) for i in range(n)]
    Hin = mat(B, K0, ps[0]['Hp']) if K0 else None

    def buffers():
        return [dict(Z=mat(B, h, None if (i or K0) else ps[0]['Z']), H=mat(B, h), xhat=mat(B, h), inv_std=vec(h),
                     mm=vec(h, ps[i]['mm0']), mv=vec(h, ps[i]['mv0'])) for i, h in enumerate(hs)]
    Wd = [mat(Ks[i], hs[i], ps[i]['W']) if Ks[i] else None for i in range(n)]
    bd = [vec(hs[i], ps[i]['bias']) if Ks[i] else None for i in range(n)]
    betad = [vec(h, ps[i]['beta']) for i, h in enumerate(hs)]

    def chain():
        bufs = buffers()
        layers = []
        for i, h in enumerate(hs):
            b = bufs[i]
            e = dict(H=h, Z=b['Z'], ldz=_ld(h), Hout=b['H'], ldh=_ld(h))
            if bn:
                e.update(beta=betad[i], moving_mean=b['mm'], moving_var=b['mv'], xhat=b['xhat'], ldx=_ld(h), inv_std=b['inv_std'])
            if Ks[i]:
                e.update(W=Wd[i], ldw=_ld(h), bias=bd[i], K=Ks[i])
            layers.append(e)
        ops.hidden_small_chain(layers, Hin, _ld(K0) if K0 else 0, B, bn, MOM, EPS, code)
        torch.cuda.synchronize()
        return bufs
    runs = [chain(), chain()]
    for i in range(n):
        bits(J, 'second run, layer %d' % i, runs[0][i], runs[1][i])
    got = runs[0]
    # layer by layer from what the chain stored
    for i, h in enumerate(hs):
        tag = 'layer %d' % i
        if Ks[i]:
            Hp64 = f64(ps[0]['Hp']) if i == 0 else body(got[i - 1]['H'], B, hs[i - 1])
            _judge_dense(J, tag, got[i], Hp64, ps[i], B, Ks[i], h, bn, code)
        else:
            J.true('Z0 unchanged', torch.equal(got[0]['Z'], mat(B, h, ps[0]['Z'])))
            if bn:
                _judge_bn_layer(J, tag, f64(ps[0]['Z']), ps[0], code, _read_apply(got[0], B, h), B, h)
            else:
                LC.fwd_conditions(code, f64(ps[0]['Z']))
                J.elem('H', tag + ' H', body(got[0]['H'], B, h), SR.act_fwd(code, f64(ps[0]['Z'])))
            for k in ('H', 'xhat'):
                pads_intact(J, tag + ' ' + k, got[0][k], B, h)
    # the per-layer kernels on the same inputs
    per = buffers()
    for i, h in enumerate(hs):
        b, ld = per[i], _ld(h)
        if Ks[i]:
            src, ldp = (Hin, _ld(K0)) if i == 0 else (per[i - 1]['H'], _ld(hs[i - 1]))
            ops.dense_bn_small(src, ldp, Wd[i], ld, bd[i], B, Ks[i], h, bn, betad[i] if bn else None, b['mm'] if bn else None,
                               b['mv'] if bn else None, MOM, EPS, code, b['Z'], ld, b['xhat'] if bn else None, ld, b['H'], ld,
                               b['inv_std'] if bn else None)
        elif bn:
            ops.bn_relu_train_small(b['Z'], ld, B, h, betad[i], b['mm'], b['mv'], MOM, EPS, code, b['H'], ld, b['xhat'], ld, b['inv_std'])
        else:
            ops.relu_fwd(b['Z'], ld, B, h, b['H'], ld, code)
    torch.cuda.synchronize()
    for i in range(n):
        bits(J, 'chain = per-layer kernels, layer %d' % i, got[i], per[i])
    J.report()


# ------------------------------------------------------------------ (d) relu_fwd / relu_bwd
ELEM_SHAPES = [(1, 1, 4), (37, 203, 208), (600, 1000, 1004)]      # 600 000 elements > 2048 x 256: a second grid-stride trip


@functools.lru_cache(maxsize=None)
def _elem_input(B, H, small):
    """Pre-activations with 0.0, -0.0 and values of magnitude `small` and 30 among them; dH of the backward."""
    rng = np.random.RandomState(9000 + B + H)
    x = LC.f32(rng.normal(size=(B, H)) * 1.5)
    special = np.float32([0.0, -0.0, small, -small, 30.0, -30.0])
    near = np.abs(np.abs(x) - 2.5) < 2e-4               # 600 000 draws put some at hard_sigmoid's kink whatever the seed:
    x[near] += np.float32(1e-3)                         # they are moved off it here, in the input, for every code alike
    flat = x.reshape(-1)
    if flat.size >= 4 * special.size:
        for j, pos in enumerate(np.linspace(0, flat.size - 1, 3 * special.size).astype(int)):
            flat[pos] = special[j % special.size]
    return x, LC.f32(rng.normal(size=(B, H)))


@pytest.mark.parametrize('code', ALL, ids=codes_id)
@pytest.mark.parametrize('B,H,ld', ELEM_SHAPES, ids=lambda v: str(v))
def test_relu_fwd(ops, B, H, ld, code):
    J = Judge('(d) relu_fwd %d x %d act=%d' % (B, H, code))
    x, _ = _elem_input(B, H, 1e-30)
    x64 = f64(x)
    LC.fwd_conditions(code, x64)
    Z = mat(B, H, x, ld)
    outs = []
    for _ in range(2):
        out = mat(B, H, None, ld)
        ops.relu_fwd(Z, ld, B, H, out, ld, code)
        torch.cuda.synchronize()
        outs.append(out)
    J.true('second run bit for bit', torch.equal(outs[0], outs[1]))
    J.elem('H', 'H', body(outs[0], B, H), SR.act_fwd(code, x64))
    pads_intact(J, 'Hout', outs[0], B, H)
    J.true('Z unchanged', torch.equal(Z, mat(B, H, x, ld)))
    J.report()


@pytest.mark.parametrize('code', ALL, ids=codes_id)
@pytest.mark.parametrize('B,H,ld', ELEM_SHAPES, ids=lambda v: str(v))
def test_relu_bwd(ops, B, H, ld, code):
    """dZ = dH act'(.) with the slope from the stored h (codes 0-11) or from Z handed in the Hact slot (codes 12, 13).  The
    small inputs are of magnitude 4e-30 here, so that LeakyReLU's stored 0.3 x stays above the 1e-30 the conditions ask."""
    J = Judge('(d) relu_bwd %d x %d act=%d' % (B, H, code))
    x, d = _elem_input(B, H, 4e-30)
    x64, d64 = f64(x), f64(d)
    h64 = f64(SR.act_fwd(code, x64))
    LC.bwd_conditions(code, x64, h64)
    dH, Hact = mat(B, H, d, ld), mat(B, H, x64 if code >= SR.ACT_PRE else h64, ld)
    outs = []
    for _ in range(2):
        out = mat(B, H, None, ld)
        ops.relu_bwd(dH, ld, Hact, ld, B, H, out, ld, code)
        torch.cuda.synchronize()
        outs.append(out)
    J.true('second run bit for bit', torch.equal(outs[0], outs[1]))
    s = SR.act_slope(code, x64)
    # (codes 12, 13 read x itself here, not an fp32 sum xhat + beta: slope_tolerance's ulp of x is an allowance unused)
    J.bound('dZ', 'dZ', np.abs(body(outs[0], B, H) - d64 * s), np.abs(d64) * SR.slope_tolerance(code, x64, h64) + SR.REL * np.abs(d64 * s))
    pads_intact(J, 'dZ', outs[0], B, H)
    J.report()


# ------------------------------------------------------------------ (e) colsum_chain
def _theta(N):
    """log-dispersions at both clip edges of clip(exp(w), 1e-3, 1e4), far outside, and across [-9, 11]."""
    edge = [np.log(1e-3) - 1e-3, np.log(1e-3) + 1e-3, np.log(1e4) - 1e-3, np.log(1e4) + 1e-3, -50.0, 50.0]
    t = np.float32(edge + list(np.linspace(-9.0, 11.0, max(N - 6, 0))))[:N]
    assert len(t) == N
    return t


@pytest.mark.parametrize('with_theta', [False, True], ids=['plain', 'theta'])
@pytest.mark.parametrize('B,N', [(5, 6), (64, 70), (4099, 130)])
def test_colsum_chain(ops, B, N, with_theta):
    """out[c] = (sum over rows of x[:, c]) * d clip(exp(theta_c), 1e-3, 1e4) / d theta_c.  |x| in [0.5, 1.5] with one sign per
    column: a dropped row moves a sum by a few times the bound or more.  The factor alone: one row of ones."""
    J = Judge('(e) colsum_chain %d x %d%s' % (B, N, ' theta' if with_theta else ''))
    rng = np.random.RandomState(300 + B + N)
    x = LC.f32(rng.uniform(0.5, 1.5, size=(B, N)) * rng.choice([-1.0, 1.0], size=N))
    x64 = f64(x)
    th = _theta(N)
    fac = np.exp(th.astype(np.float64))
    inside = (fac >= 1e-3) & (fac <= 1e4)
    assert inside.sum() >= 2 and (~inside).sum() >= 4
    fac = np.where(inside, fac, 0.0) if with_theta else np.ones(N)
    m = -(-B // 4)
    bnd = ((m + 2) * 2.0 ** -24 + SR.REL) * np.abs(x64).sum(0)
    assert B < 8 or (np.abs(x64).min(0) > 1.9 * bnd).all()               # a dropped row would show
    ld = _ld(N)
    X, thd = mat(B, N, x), (vec(N, th) if with_theta else None)
    outs = []
    for _ in range(2):
        out = vec(N)
        ops.colsum_chain(X, ld, B, N, thd, out)
        torch.cuda.synchronize()
        outs.append(out)
    J.true('second run bit for bit', torch.equal(outs[0], outs[1]))
    got = host(outs[0])[:N]
    S = x64.sum(0)
    J.bound('colsum', 'sums', np.abs(got - S * fac), (bnd + (1e-6 * np.abs(S) if with_theta else 0.0)) * fac)
    tail_intact(J, 'out', outs[0], N)
    if with_theta:
        J.true('exactly 0 outside the clip', bool((got[~inside] == 0.0).all()))
        one, out = mat(1, N, np.ones((1, N))), vec(N)
        ops.colsum_chain(one, ld, 1, N, thd, out)
        torch.cuda.synchronize()
        f = host(out)[:N]
        J.bound('chain factor', 'factor', np.abs(f - fac), 1e-6 * fac)
        J.true('factor exactly 0 outside the clip', bool((f[~inside] == 0.0).all()))
    J.report()
