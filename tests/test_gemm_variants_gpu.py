"""Every kernel instantiation dcahip_sgemm can launch -- four tiles, three layouts, 16-byte and scalar loaders, the exact
fp32 and the three-bf16-piece arithmetic, the three endings of a split -- against fp64, on the cases of tests/_gemm_cases.py
(tests/test_gemm_variants_cpu.py proves on the host that the table reaches all of them).

Bounds (none of them new): a case that runs on three bf16 pieces is held to the contract of include/dcahip.h, 5e-7 of
sum|ab| (+ |bias|) per element; a case that runs exact to the chain bound tests/test_kernels_gpu.py::test_sgemm_vs_numpy
applies up to K = 3000, 2e-6 of the same + 1e-6; the column-sum row as there.  Which one applies is read from
dcahip_sgemm_plan, the function the launch itself takes its arithmetic from."""
import numpy as np
import pytest
import torch

import _gemm_cases as GC

pytestmark = pytest.mark.gpu

SENTINEL = 123.0
WS_GUARD = 64                  # floats behind the workspace the library asked for


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _place(a, offset):
    """The array on the device, its first element `offset` floats behind a 16-byte boundary."""
    flat = torch.empty(a.size + 4, device='cuda')
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return view


def _bits(t):
    return t.view(torch.int32)


class Problem:
    """The device operands of one case; run() is one dcahip_sgemm call into a fresh C and a fresh workspace."""

    def __init__(self, ops, case, **kw):
        self.ops, self.case = ops, case
        ta, tb, M, N, K, split, align, flags = case
        self.o = o = GC.operands(case, **kw)
        oa, ob = GC.offsets(case)
        self.A, self.B = _place(o['a_store'], oa), _place(o['b_store'], ob)
        self.bias = torch.from_numpy(o['bias']).cuda() if o['bias'] is not None else None
        self.perm = torch.from_numpy(o['perm']).cuda() if o['perm'] is not None else None
        self.cursor = torch.tensor([o['cursor']], dtype=torch.int64, device='cuda') if o['cursor'] is not None else None
        self.colsum = 'c' in flags
        self.Mo = M + int(self.colsum)
        self.plan = ops.sgemm_plan(ta, tb, M, N, K, self.A, o['lda'], self.B, o['ldb'], colsum_row=self.colsum, split_k=split)
        self.ws_floats = ops.sgemm_workspace_bytes(ta, tb, M, N, K, self.colsum, split) // 4

    def run(self):
        ta, tb, M, N, K, split, align, flags = self.case
        o = self.o
        C = torch.full((self.Mo + 1, o['ldc']), SENTINEL, device='cuda')         # one guard row
        ws = torch.full((self.ws_floats + WS_GUARD,), float('nan'), device='cuda')
        self.ops.sgemm(ta, tb, M, N, K, self.A, o['lda'], self.B, o['ldb'], C, o['ldc'], bias=self.bias, perm=self.perm,
                       cursor=self.cursor, colsum_row=self.colsum, split_k=split, ws=ws[:self.ws_floats] if self.ws_floats else None)
        torch.cuda.synchronize()
        return C, ws


@pytest.mark.parametrize('case', GC.CASES, ids=GC.case_id)
def test_sgemm_variant_vs_fp64(ops, case):
    ta, tb, M, N, K, split, align, flags = case
    p = Problem(ops, case)
    o = p.o
    tile_m, tile_n, mtiles, ntiles, nsplit, kslab, x3, vec = p.plan
    assert vec == (4 if align == 'v4' else 1), p.plan
    assert p.ws_floats == (nsplit * p.Mo * N if nsplit > 1 else 0)
    C, ws = p.run()
    out = C.cpu().numpy()

    # nothing outside [M (+ 1), N] changes, nothing behind the workspace either; the reduce read written slabs only
    assert (out[p.Mo:] == SENTINEL).all() and (out[:, N:] == SENTINEL).all()
    assert torch.isnan(ws[p.ws_floats:]).all()
    assert np.isfinite(out[:p.Mo, :N]).all(), np.argwhere(~np.isfinite(out[:p.Mo, :N]))[:5]

    ref = o['opA'] @ o['opB']
    mag = np.abs(o['opA']) @ np.abs(o['opB'])
    if o['bias'] is not None:
        ref = ref + o['bias'].astype(np.float64)
        mag = mag + np.abs(o['bias'].astype(np.float64))
    err = np.abs(out[:M, :N].astype(np.float64) - ref)
    tol = (5e-7 * mag + 1e-30) if x3 else (2e-6 * mag + 1e-6)
    print('%s: tile %dx%d, %s, V=%d, split %d; max err / sum|ab| = %.3g' % (
        GC.case_id(case), tile_m, tile_n, 'x3' if x3 else 'exact', vec, nsplit, float((err / mag).max())))
    assert (err <= tol).all(), (err.max(), float((err / mag).max()), np.argwhere(err > tol)[:5])
    if p.colsum:
        Bkn = o['opB']
        np.testing.assert_allclose(out[M, :N], Bkn.sum(axis=0), rtol=0, atol=2e-6 * np.abs(Bkn).sum(axis=0).max() + 1e-6)

    # deterministic: the same call gives the same bits
    C2, _ = p.run()
    assert torch.equal(_bits(C), _bits(C2))


SCALE_CASES = [c for c in GC.CASES if 's' in c[7]]


def _magnitudes(rng, shape):
    """Entries of magnitude in [1/4, 1): scaled by at most 2^+-40 they, their three bf16 pieces and every partial sum of
    their products stay far from overflow and from the denormals."""
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 1.0, shape)


@pytest.mark.parametrize('case', SCALE_CASES, ids=GC.case_id)
def test_sgemm_is_invariant_under_power_of_two_scaling(ops, case):
    """Rows of op(A) times 2^a_m, columns of op(B) times 2^b_n, the k-th element of A times 2^s_k and of B times 2^-s_k
    (integers in [-20, 20]): every product a b is the unscaled one times 2^(a_m + b_n) exactly, and so is every rounding of
    both arithmetics -- the output equals the unscaled output times 2^(a_m + b_n) bit for bit.  An absolute threshold, a
    flushed third piece or a rounding that depends on the magnitude breaks this; no tolerance against fp64 sees them."""
    ta, tb, M, N, K, split, align, flags = case
    rng = np.random.RandomState(31 * M + 17 * N + K)
    a_m, b_n, s_k = (rng.randint(-20, 21, n) for n in (M, N, K))
    plain = Problem(ops, case, values=_magnitudes)
    scaled = Problem(ops, case, values=_magnitudes, scale=(a_m, b_n, s_k))
    assert plain.plan == scaled.plan
    out = plain.run()[0].cpu().numpy()[:M, :N]
    got = scaled.run()[0].cpu().numpy()[:M, :N]
    want = np.ldexp(out, (a_m[:, None] + b_n[None, :]).astype(np.int32))
    assert want.dtype == np.float32 and np.isfinite(want).all() and (np.abs(want) > 1e-30).all()
    differ = np.argwhere(want.view(np.int32) != got.view(np.int32))
    assert differ.size == 0, (len(differ), differ[:5], [(want[i, j], got[i, j]) for i, j in differ[:5]])
