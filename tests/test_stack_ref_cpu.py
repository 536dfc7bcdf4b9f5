"""The fp64 reference of the K-STACK and per-layer kernel tests (tests/_stack_ref.py) is itself checked here, without a GPU:
against the network oracle's autodiff, for the equality of a merge over row ranges with the one-range pass, for the
slope-from-output forms, for the chunk partition of the large-batch kernels, and -- with a numpy-fp32 restatement of
col_moments + bn_relu_apply -- for the bounds that tests/test_layer_kernels_gpu.py holds those kernels to."""
import numpy as np
import pytest

import _keras_acts as KA
import _layer_cases as LC
import _stack_ref as SR
from _judge import EL
from oracle import net_np as N

STACKS = [(64, 32, 64), (48, 20, 7, 33)]
ACTS = ['relu', 'tanh', 'selu', 'swish', 'gelu']


def _close(got, ref, what, tol=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max()
    assert err <= tol * max(np.abs(ref).max(), 1e-300), (what, float(err), float(np.abs(ref).max()))


def _stack_problem(hs, B, seed, shift=0.0):
    rng = np.random.RandomState(seed)
    L = len(hs)
    Z0 = rng.normal(size=(B, hs[0])) * 1.5 + rng.normal(size=hs[0])
    layers = []
    for i, h in enumerate(hs):
        d = dict(beta=rng.normal(size=h) * 0.3 + shift, mm=rng.normal(size=h) * 0.1, mv=rng.uniform(0.5, 1.5, size=h))
        if i > 0:
            d.update(W=rng.normal(size=(hs[i - 1], h)) * 0.4, bias=rng.normal(size=h) * 0.1)
        layers.append(d)
    dH = rng.normal(size=(B, hs[L - 1]))
    return Z0, layers, dH


@pytest.mark.parametrize('activation', ACTS)
@pytest.mark.parametrize('hs', STACKS)
def test_stack_ref_equals_the_network_oracle(monkeypatch, hs, activation):
    """_stack_ref's forward (H, Z, moving statistics) and backward (dbeta, gW, dZ0) against oracle.net_np's forward /
    loss_and_grads.  The oracle reaches the stack through an identity input (Z0 = W0 + b0, so g['W0'] = dZ0) and an
    identity mean head with a linear loss (the gradient w.r.t. the last layer's output is the arbitrary dH)."""
    KA.extend_oracle(monkeypatch)
    B, L = 37, len(hs)
    code = N.ACT_CODES[activation]
    Z0, layers, dH = _stack_problem(hs, B, 11 + L, shift=-0.8 if code >= SR.ACT_PRE else 0.0)
    p = {'W0': Z0.copy(), 'b0': np.zeros(hs[0]), 'W_mean': np.eye(hs[-1]), 'b_mean': np.zeros(hs[-1])}
    for i, d in enumerate(layers):
        p['beta%d' % i], p['mm%d' % i], p['mv%d' % i] = d['beta'].copy(), d['mm'].copy(), d['mv'].copy()
        if i > 0:
            p['W%d' % i], p['b%d' % i] = d['W'].copy(), d['bias'].copy()
    net = N.OracleAE('normal', p, hs, True, activation=activation)
    monkeypatch.setattr(net, '_loss_grads', lambda c, Y, n_total: (0.0, 0.0, dH, None, None))
    _, g = net.loss_and_grads(np.eye(B), np.zeros((B, hs[-1])), np.ones(B))
    c = net.cache
    fw = SR.fwd_pass(Z0, layers, code)
    for i in range(L):
        _close(fw[i]['Z'], c['Z'][i], 'Z%d' % i)
        _close(fw[i]['xhat'], c['xh'][i], 'xhat%d' % i)
        _close(fw[i]['inv_std'], c['inv'][i], 'inv%d' % i)
        _close(fw[i]['H'], c['H'][i + 1], 'H%d' % i)
        _close(fw[i]['mm'], net.p['mm%d' % i], 'mm%d' % i)
        _close(fw[i]['mv'], net.p['mv%d' % i], 'mv%d' % i)
    bl = [dict(Hact=fw[i]['H'], xhat=fw[i]['xhat'], inv_std=fw[i]['inv_std'], beta=layers[i]['beta'],
               W=layers[i].get('W')) for i in range(L)]
    bw = SR.bwd_pass(dH, bl, float(B), code)
    _close(bw[0]['dZ'], g['W0'], 'dZ0')
    for i in range(L):
        _close(bw[i]['dbeta'], g['beta%d' % i], 'dbeta%d' % i)
        if i > 0:
            _close(bw[i]['gW'][:-1], g['W%d' % i], 'gW%d' % i)
            # (the bias in front of a batch norm: its gradient cancels to round-off -- judged against the summed magnitudes)
            assert np.abs(bw[i]['gW'][-1] - g['b%d' % i]).max() <= 1e-12 * bw[i]['gW_mag'][-1].max()


RANGE_SETS = {'one': [200], 'partial_and_empty': [33, 1, 0, 166],
              'many': [int(c) for c in np.random.RandomState(5).permutation([1] * 80 + [2] * 30 + [3] * 20)]}


@pytest.mark.parametrize('name', sorted(RANGE_SETS))
@pytest.mark.parametrize('code', [1, 13])
def test_merge_over_row_ranges_equals_the_global_pass(name, code):
    """Per-range (mean, M2) and per-range sums, merged, reproduce the one-range statistics and every output of every step."""
    counts = RANGE_SETS[name]
    if name == 'many':
        assert len(counts) == 130 and 1 <= min(counts) and sum(counts) == 200
    B, hs = 200, (48, 20, 7, 33)
    assert sum(counts) == B
    ranges = SR.split_ranges(counts)
    L = len(hs)
    Z0, layers, dH = _stack_problem(hs, B, 3, shift=-0.8 if code >= SR.ACT_PRE else 0.0)
    glob = SR.fwd_pass(Z0, layers, code)
    Z = Z0
    st = SR.fwd_step(0, Z, ranges=ranges)['stats']
    for i in range(L):
        n, gm, gq = SR.merge_stats(st['count'], st['mean'], st['m2'])
        one = SR.range_stats(Z, [(0, B)])
        assert n == B
        _close(gm, one['mean'][0], 'mean%d' % i)
        _close(gq, one['m2'][0], 'M2 %d' % i)
        Nx = layers[i + 1] if i + 1 < L else {}
        # every rank's rows with the merged entries = the rows of the global pass
        for a, b in ranges:
            if b == a:
                continue
            o = SR.fwd_step(i + 1, Z[a:b], st['count'], st['mean'], st['m2'], layers[i]['beta'], Nx.get('W'), Nx.get('bias'),
                            layers[i]['mm'], layers[i]['mv'], code)
            for k in ('xhat', 'H'):
                _close(o[k], glob[i][k][a:b], '%s%d' % (k, i))
            for k in ('inv_std', 'mm', 'mv'):
                _close(o[k], glob[i][k], '%s%d' % (k, i))
            if i + 1 < L:
                _close(o['Z'], glob[i + 1]['Z'][a:b], 'Z%d' % (i + 1))
        if i + 1 < L:
            Z = glob[i + 1]['Z']
            st = SR.range_stats(Z, ranges)
    bl = [dict(Hact=glob[i]['H'], xhat=glob[i]['xhat'], inv_std=glob[i]['inv_std'], beta=layers[i]['beta'],
               W=layers[i].get('W')) for i in range(L)]
    ref = SR.bwd_pass(dH, bl, float(B), code)
    dHi = dH
    sums = SR.bwd_step(0, dHi, bl[-1]['Hact'], bl[-1]['xhat'], beta=bl[-1]['beta'], act=code, ranges=ranges)['sums'].sum(0)
    for i in reversed(range(L)):
        P = bl[i - 1] if i > 0 else None
        gW, low, dbeta = 0.0, 0.0, 0.0
        dHp = np.zeros((B, hs[i - 1])) if P else None
        for a, b in ranges:
            if b == a:
                continue
            o = SR.bwd_step(L - i, dHi[a:b], bl[i]['Hact'][a:b], bl[i]['xhat'][a:b], bl[i]['inv_std'], bl[i]['beta'],
                            sums[0], sums[1], float(B), P['Hact'][a:b] if P else None, bl[i]['W'] if P else None,
                            dict(Hact=P['Hact'][a:b], xhat=P['xhat'][a:b], beta=P['beta']) if P else None, code)
            _close(o['dZ'], ref[i]['dZ'][a:b], 'dZ%d' % i, 1e-12 * max(1.0, ref[i]['dZ_mag'].max() / np.abs(ref[i]['dZ']).max()))
            dbeta = dbeta + o['dbeta']
            if P:
                gW = gW + o['gW']
                low = low + o['low_sums'][0]
                dHp[a:b] = o['dHprev']
        assert np.abs(dbeta - ref[i]['dbeta']).max() <= 1e-12 * ref[i]['dbeta_mag'].max()
        if P:
            assert (np.abs(gW - ref[i]['gW']) <= 1e-12 * ref[i]['gW_mag'] + 1e-300).all()
            assert (np.abs(dHp - ref[i]['dHprev']) <= 1e-12 * ref[i]['dHprev_mag'] + 1e-300).all()
            assert (np.abs(low - ref[i]['low_sums'][0]) <= 1e-12 * ref[i]['low_sums_mag'][0] + 1e-300).all()
            dHi, sums = dHp, low


def test_zero_count_entry_is_ignored_by_the_merge():
    rng = np.random.RandomState(0)
    m, q = rng.normal(size=(3, 5)), rng.uniform(1, 2, size=(3, 5))
    a = SR.merge_stats([4, 9, 2], m, q)
    b = SR.merge_stats([4, 9, 0, 2], np.insert(m, 2, 3.0, axis=0), np.insert(q, 2, 5.0, axis=0))
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize('code', [2, 3, 4, 5, 6, 7, 8, 10, 11])
def test_slope_from_the_output_equals_the_slope_from_x(code):
    """The forms through h = act(x) that the kernels use for codes 0-11 (this guards the reference, not the kernel)."""
    rng = np.random.RandomState(code)
    x = np.concatenate([rng.normal(size=4000) * 1.5 - 0.3, np.linspace(-4.0, 4.0, 161) + 1e-3])
    got = SR.act_slope_from_out(code, SR.act_fwd(code, x))
    np.testing.assert_allclose(got, SR.act_slope(code, x), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('code', SR.CODES)
def test_slope_is_the_derivative_of_the_activation(code):
    """act_slope against a central difference of act_fwd (away from the kinks), and the fp64 activations of codes 10-13
    against tests/_keras_acts.py."""
    rng = np.random.RandomState(100 + code)
    x = rng.normal(size=2000) * 1.5
    x = x[(np.abs(x) > 1e-3) & (np.abs(np.abs(x) - 2.5) > 1e-3)]
    d = 1e-6
    num = (SR.act_fwd(code, x + d) - SR.act_fwd(code, x - d)) / (2 * d)
    np.testing.assert_allclose(SR.act_slope(code, x), num, rtol=1e-7, atol=1e-8)
    if code >= 10:
        np.testing.assert_allclose(SR.act_fwd(code, x), KA.fwd(code, x), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(SR.act_slope(code, x), KA.grad(code, x), rtol=1e-12, atol=1e-15)
    elif code <= 8:
        np.testing.assert_allclose(SR.act_fwd(code, x), N.act_fwd(code, x), rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------ chunk_ranges and the bounds of the large-batch forward
@pytest.mark.parametrize('B', [1, 2, 63, 64, 65, 130, 2800, 4096, 16383, 16384])
def test_chunk_ranges_equals_block_ranges_below_the_cap(B):
    assert SR.chunk_ranges(B) == SR.block_ranges(B, 64) == SR.chunk_ranges(B, len(SR.block_ranges(B, 64)))


def test_chunk_ranges_under_the_cap():
    """n_chunks / chunk_rows of dcahip_layers.hip at B = 16450: 256 chunks of 65 rows, chunk 253 holds 5, the last two none."""
    r = SR.chunk_ranges(16450)
    assert len(r) == 256 == SR.MAX_CHUNKS and all(b - a == 65 for a, b in r[:253])
    assert r[253] == (16445, 16450) and r[254] == r[255] == (16450, 16450)
    assert sum(b - a for a, b in r) == 16450
    assert len(SR.block_ranges(16450, 64)) == 258          # what the chunks would be without the cap


F = np.float32


def _lane_sums(x):
    """Column sums of fp32 x [rows, H] the way a workgroup forms them: 4 interleaved row lanes, each adding its rows one
    after the other in fp32, the lanes added pairwise."""
    l = [x[t::4].cumsum(0, dtype=F)[-1] if len(x[t::4]) else np.zeros(x.shape[1], F) for t in range(4)]
    return (l[0] + l[1]) + (l[2] + l[3])


def emu_col_moments(Z, ranges):
    """numpy-fp32 restatement of col_moments_kernel: two passes, part[r] = (mean, M2) of chunk r."""
    part = np.zeros((len(ranges), 2, Z.shape[1]), F)
    for r, (a, b) in enumerate(ranges):
        if b > a:
            mean = _lane_sums(Z[a:b]) / F(b - a)
            d = Z[a:b] - mean
            part[r, 0], part[r, 1] = mean, _lane_sums(d * d)
    return part


def emu_bn_apply(Z, counts, part, beta, mm, mv, code, mom=F(SR.BN_MOMENTUM), eps=F(SR.BN_EPS)):
    """numpy restatement of bn_relu_apply_kernel: merge of the entries in fp64 (two passes), everything else in fp32."""
    c = np.asarray(counts, np.float64)[:, None]
    n = c.sum()
    m64 = (c * part[:, 0].astype(np.float64)).sum(0) / n
    q64 = (np.where(c > 0, part[:, 1].astype(np.float64) + c * np.square(part[:, 0].astype(np.float64) - m64), 0.0)).sum(0)
    mean, var = m64.astype(F), (q64 / n).astype(F)
    inv = F(1) / np.sqrt(var + eps)
    xh = (Z - mean) * inv
    x = xh + beta
    H = {0: lambda: x, 1: lambda: np.maximum(x, F(0)), 2: lambda: np.tanh(x)}[code]()
    one = F(1) - mom
    assert all(a.dtype == F for a in (mean, var, inv, xh, H))
    return dict(xhat=xh, H=H, inv_std=inv, mm=mm - (mm - mean) * one, mv=mv - (mv - var) * one)


def _ratio(err, bnd):
    return float((np.abs(err) / (bnd + 1e-30)).max())


def _judge_emulation(p, code):
    """Worst error / bound of the emulation: per chunk; against fwd_step on the entries it wrote; against the statistics
    of Z itself.  Returns the ratios and, per column, the errors of xhat / inv_std against the flat classes."""
    B, H = p['B'], p['H']
    Z64 = p['Z'].astype(np.float64)
    ranges = SR.chunk_ranges(B)
    cnt = [b - a for a, b in ranges]
    part = emu_col_moments(p['Z'], ranges)
    st, g = SR.range_stats(Z64, ranges), SR.range_stats(Z64, [(0, B)])
    out = {'chunk mean': _ratio(part[:, 0] - st['mean'], SR.REL * st['mean_mag']),
           'chunk M2': _ratio(part[:, 1] - st['m2'], SR.REL * st['m2_mag'] + st['m2_in'])}
    t_mean, t_m2 = SR.moments_tolerance(st, g)
    e = emu_bn_apply(p['Z'], cnt, part, p['beta'], p['mm0'], p['mv0'], code)
    flat = {}
    for tag, ent in (('forced', (cnt, part[:, 0], part[:, 1])), ('end to end', ([B], g['mean'], g['m2']))):
        o = SR.fwd_step(1, Z64, ent[0], ent[1], ent[2], p['beta'].astype(np.float64), None, None, p['mm0'].astype(np.float64),
                        p['mv0'].astype(np.float64), code)
        LC.fwd_conditions(code, o['xhat'] + p['beta'], o['inv_std'] * t_mean)
        bnd = SR.fwd_bounds(o, code, p['beta'], t_mean, t_m2, B, EL)
        for k in ('xhat', 'H', 'inv_std', 'mm', 'mv'):
            out['%s %s' % (tag, k)] = _ratio(e[k] - o[k], bnd[k])
        flat[tag] = (np.abs(e['xhat'] - o['xhat']) / (EL['xhat'][1] + EL['xhat'][0] * np.abs(o['xhat'])),
                     np.abs(e['inv_std'] - o['inv_std']) / (1e-5 * o['inv_std']))
    return out, flat


@pytest.mark.parametrize('code', [0, 1, 2])
@pytest.mark.parametrize('B,H', LC.LARGE_SHAPES)
def test_fp32_restatement_meets_the_large_batch_forward_bounds(B, H, code):
    out, _ = _judge_emulation(LC.large_fwd_problem(B, H), code)
    print('\nemulation %d x %d code %d: ' % (B, H, code) + '  '.join('%s %.3g' % kv for kv in sorted(out.items())))
    assert max(out.values()) <= 1.0, out


@pytest.mark.parametrize('code', [0, 1])
@pytest.mark.parametrize('B,H', LC.COND_SHAPES)
def test_conditioned_columns_need_the_reference_terms(B, H, code):
    """With the conditioned columns the restatement stays inside the bounds that carry t_mean / t_M2, and on the
    (3000, 0.3) column it MISSES the flat classes: xhat by the rounding of an fp32 mean of 3000 (ulp 2.4e-4) times
    inv_std = 3.3, inv_std -- against the statistics of Z itself -- by the chunk means' errors entering the merge (with the
    two chunks of 65 rows; over the 44 chunks of 2800 rows these errors average out to just under the flat class, so there
    the figure is only printed)."""
    out, flat = _judge_emulation(LC.large_fwd_problem(B, H, conditioned=True), code)
    print('\nemulation %d x %d code %d conditioned: ' % (B, H, code) + '  '.join('%s %.3g' % kv for kv in sorted(out.items())))
    assert max(out.values()) <= 1.0, out
    c = LC.COND_COLS[H][LC.WORST_COL]
    xh, inv = flat['end to end']
    print('(3000, 0.3) column against the flat classes: xhat %.3g  inv_std %.3g' % (xh[:, c].max(), inv[c]))
    assert xh[:, c].max() > 1.0 and flat['forced'][0][:, c].max() > 1.0
    assert B != 65 or inv[c] > 1.0
