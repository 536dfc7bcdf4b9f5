"""dcahip_zinb_heads_infer (heads_infer_kernel<4> and <1>) on the MI355X against the fp64 oracle, at the layouts and values
of tests/_heads_infer_cases.py: both forms of the kernel, one and several 256-lane segments, the grid-stride loop, every
subset of the outputs, in and out of place, the linear mean, pre-activations at the clips and beyond the range of expf, NaN,
and the argument errors.  tests/test_heads_infer_cases_cpu.py checks the table and the reference themselves.

Every call goes through HipOps.heads_infer.  The outputs are compared over [:B, :G] with RTOL |ref| + ATOL (3e-6 and the
smallest normal fp32, see _heads_infer_cases.py); every other word of the output buffer -- rows from B on, columns from Gp
(V = 4) or G (V = 1) on, planes that were not asked for -- and, out of place, the whole input buffer must keep its bits.
The pad columns [G, Gp) of a requested plane may be written by the vector form and are left unspecified.
"""
import numpy as np
import pytest
import torch

import _heads_infer_cases as C

pytestmark = pytest.mark.gpu

I32 = torch.int32


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _buffers(case, data):
    """(input buffer, output buffer) on the device, SENTINEL everywhere but the planted input planes."""
    B, G, rows = case.B, case.G, case.B + C.GUARD_ROWS
    A = np.full((rows, case.lda), C.SENTINEL, np.float32)
    for h in case.heads_in:
        o = case.offs[C.HEADS.index(h)]
        A[:B, o:o + G] = data[h]
    dA = torch.from_numpy(A).cuda()
    assert dA.data_ptr() % 16 == 0
    if case.in_place:
        return dA, dA
    flat = torch.full((rows * case.ldo + 4,), float(C.SENTINEL), dtype=torch.float32, device='cuda')
    assert flat.data_ptr() % 16 == 0
    return dA, flat[case.out_shift:case.out_shift + rows * case.ldo].view(rows, case.ldo)


_runs = {}


def run(ops, case, nan=False):
    """One call of the case; checks that nothing outside the requested outputs moved; {head: [B, G] fp32 host array}."""
    key = (case.name, nan)
    if key in _runs:
        return _runs[key]
    B, G = case.B, case.G
    data = C.inputs(B, G, nan)
    dA, dO = _buffers(case, data)
    in_before, out_before = dA.clone(), dO.clone()
    sf = torch.from_numpy(data['sf'].astype(np.float32)).cuda()
    a_in = [dA[:, case.offs[i]:] if h in case.heads_in else None for i, h in enumerate(C.HEADS)]
    a_out = [dO[:, case.ooffs[i]:] if h in case.heads_out else None for i, h in enumerate(C.HEADS)]
    path = C.expected_path(case)
    for t, off in zip(a_out, case.ooffs):              # the pointers are what the table says they are
        assert t is None or (t.data_ptr() % 16 == 0) == ((case.out_shift + off) % 4 == 0)
    ops.heads_infer(a_in[0], a_in[1], a_in[2], case.lda, sf, B, G, a_out[0], a_out[1], a_out[2], case.ldo, case.flags)
    torch.cuda.synchronize()
    width = G if path.V == 1 else C.gp(G)
    may = torch.zeros(dO.shape, dtype=torch.bool, device='cuda')
    for h in case.heads_out:
        o = case.ooffs[C.HEADS.index(h)]
        may[:B, o:o + width] = True
    moved = (dO.view(I32) != out_before.view(I32)) & ~may
    assert not bool(moved.any()), (case.name, 'written outside the outputs at', moved.nonzero()[:5].tolist())
    if not case.in_place:
        assert torch.equal(dA.view(I32), in_before.view(I32)), (case.name, 'the inputs of an out-of-place call changed')
    out = {h: dO[:B, case.ooffs[C.HEADS.index(h)]:][:, :G].cpu().numpy() for h in case.heads_out}
    if B * G <= 100000:
        _runs[key] = out
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def linear_mean_f32(data):
    with np.errstate(over='ignore', invalid='ignore'):
        return data['mean'].astype(np.float32) * data['sf'].astype(np.float32)[:, None]


@pytest.mark.parametrize('case', C.LAYOUT_CASES, ids=lambda c: c.name)
def test_layout_against_fp64(ops, case):
    got = run(ops, case)
    assert set(got) == set(case.heads_out)
    ref = C.reference(case.B, case.G, case.flags)
    path = C.expected_path(case)
    print('%s: V %d, %d segments, %d items%s; worst error / bar: %s'
          % (case.name, path.V, path.nseg, path.items, ' (grid-stride)' if path.stride else '',
             ', '.join('%s %.3f' % (h, C.worst(got[h], ref[h])) for h in case.heads_out)))
    for h in case.heads_out:
        if h == 'mean' and case.flags & C.MSE:          # one fp32 product: bit for bit
            want = linear_mean_f32(C.inputs(case.B, case.G))
            assert same_bits(got[h], want), np.argwhere(got[h].view(np.int32) != want.view(np.int32))[:5]
            continue
        ok = C.within(got[h], ref[h])
        assert ok.all(), (case.name, h, int((~ok).sum()), np.argwhere(~ok)[:5].tolist(), got[h][~ok][:5], ref[h][~ok][:5])


@pytest.mark.parametrize('a,b', C.SAME_BITS_IN_OUT)
def test_in_place_and_out_of_place_give_the_same_bits(ops, a, b):
    ra, rb = run(ops, C.BY_NAME[a]), run(ops, C.BY_NAME[b])
    for h in C.HEADS:
        assert same_bits(ra[h], rb[h]), h


@pytest.mark.parametrize('a,b', C.SAME_BITS_V1_V4)
def test_scalar_and_vector_form_give_the_same_bits(ops, a, b):
    """The arithmetic of an element does not depend on the form that loads it."""
    assert (C.expected_path(C.BY_NAME[a]).V, C.expected_path(C.BY_NAME[b]).V) == (1, 4)
    ra, rb = run(ops, C.BY_NAME[a]), run(ops, C.BY_NAME[b])
    for h in C.HEADS:
        assert same_bits(ra[h], rb[h]), h


@pytest.mark.parametrize('flags', [0, C.MSE], ids=['exp', 'linear'])
@pytest.mark.parametrize('name', C.NAN_CASES)
def test_nan_stays_nan(ops, name, flags):
    """A NaN pre-activation gives NaN in its head, as tf.clip_by_value and the oracle's np.clip do -- not the lower clip
    constant that fminf(fmaxf(NaN, lo), hi) returns -- and every other element keeps the bits of the run without it."""
    case = C.BY_NAME[name]._replace(flags=flags, name=name + ('_linear' if flags else ''))
    clean, got = run(ops, case), run(ops, case, nan=True)
    ref = C.reference(case.B, case.G, flags, nan=True)
    pos = C.nan_positions(case.B, case.G)
    for h in C.HEADS:
        want = np.isnan(ref[h])
        assert want.sum() == 1 and want[pos[h]]
        print('%s %s: at the NaN input the kernel wrote %r' % (case.name, h, got[h][pos[h]]))
        assert np.array_equal(np.isnan(got[h]), want), (h, got[h][pos[h]], np.argwhere(np.isnan(got[h])).tolist())
        assert same_bits(got[h][~want], clean[h][~want]), h


def test_argument_errors_raise_and_write_nothing(ops):
    B, G, Gp = 3, 8, 8
    A = torch.full((B, 3 * Gp), 0.25, device='cuda')
    O = torch.full((B, 3 * Gp), float(C.SENTINEL), device='cuda')
    sf = torch.ones(B, device='cuda')
    am, ad, ap = A[:, 0:], A[:, Gp:], A[:, 2 * Gp:]
    om, od, op = O[:, 0:], O[:, Gp:], O[:, 2 * Gp:]
    a_before, o_before = A.clone(), O.clone()

    def call(B=B, G=G, sf_=sf, ins=(am, ad, ap), outs=(om, od, op)):
        ops.heads_infer(ins[0], ins[1], ins[2], 3 * Gp, sf_, B, G, outs[0], outs[1], outs[2], 3 * Gp)
    bad = [dict(B=0), dict(G=0), dict(B=-1), dict(G=-4), dict(sf_=None),
           dict(ins=(None, ad, ap)), dict(ins=(am, None, ap)), dict(ins=(am, ad, None)),
           dict(ins=(None, None, None)), dict(ins=(None, ad, ap), outs=(om, None, None))]
    for kw in bad:
        with pytest.raises(RuntimeError, match='heads_infer failed with code -22'):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(O, o_before) and torch.equal(A, a_before)
    call(ins=(None, ad, None), outs=(None, od, None))        # an input without its output, and no input at all for the others: fine
    call(ins=(am, ad, ap), outs=(None, None, op))
    torch.cuda.synchronize()
    assert torch.equal(O[:, :Gp], o_before[:, :Gp]) and not torch.equal(O[:, Gp:], o_before[:, Gp:])
    assert float((O[:, 2 * Gp:] - 0.5621765).abs().max()) < 1e-6          # sigmoid(0.25)
