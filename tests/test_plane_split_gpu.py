"""The kernels that feed the plane products -- dcahip_split_planes (three bf16 pieces), dcahip_split_planes_h2 (two fp16
pieces after a block scale) and dcahip_absmax_exp (the block exponent) -- bit for bit against their numpy restatements in
tests/_plane_gemm_cases.py: the pieces are a pure function of the input (round to nearest even of x 2^e, then of the exact
residual).  tests/test_plane_gemm_cases_cpu.py holds the restatements to the project's error bounds."""
import numpy as np
import pytest
import torch

import _plane_gemm_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 0x7E7E                 # what the row behind the planes holds


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _place(a, offset=0):
    """The array on the device, its first element `offset` floats behind a 16-byte boundary."""
    flat = torch.empty(a.size + 4, device='cuda')
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return view


# name: (storage rows, R, C, ld - C, source offset in floats, ldp - r8(C), gather)
SPLIT_CASES = {
    'vector':        (37, 37, 56, 4, 0, 0, ''),           # ld % 4 == 0, aligned, C % 8 == 0: 16-byte loads throughout
    'ragged-C':      (37, 37, 53, 3, 0, 0, ''),           # C % 8 != 0: the last unit of a row element by element
    'ld-odd':        (37, 37, 53, 4, 0, 0, ''),           # ld % 4 == 1: scalar loads
    'source-offset': (37, 37, 53, 3, 1, 0, ''),           # the source one float past a 16-byte boundary: scalar loads
    'wide-ldp':      (37, 37, 53, 3, 0, 16, ''),          # ldp > r8(C): zeros up to ldp
    'perm-cursor':   (37, 20, 53, 3, 0, 0, 'p'),
    'cursor':        (37, 20, 53, 3, 0, 8, 'u'),
    # more than 16384 x 256 units of 8 elements (the grid's cap): the grid-stride loop runs; the data sit in the first units
    # of every row, the rows from 4092 on belong to the second trip
    'grid-cap':      (4100, 4100, 100, 4, 0, 8200 - 104, ''),
}
CURSOR = 3


def _split_case(name, pieces, rng):
    n_store, R, C, dld, off, dldp, gather = SPLIT_CASES[name]
    ld, ldp = C + dld, PC.r8(C) + dldp
    assert (name == 'ld-odd') == (ld % 4 == 1) and (ld % 4 == 0 or name == 'ld-odd')
    x = PC.split_inputs(rng, (n_store, C), pieces)
    src = np.full((n_store, ld), np.nan, np.float32)
    src[:, :C] = x
    perm = cursor = None
    rows = np.arange(R)
    if gather == 'p':
        perm = rng.permutation(n_store)[:CURSOR + R].astype(np.int32)
        cursor, rows = CURSOR, perm[CURSOR:]
    elif gather == 'u':
        cursor, rows = CURSOR, np.arange(CURSOR, CURSOR + R)
    return dict(x=x, src=_place(src, off), ld=ld, ldp=ldp, R=R, C=C, rows=rows, n_store=n_store,
                perm=None if perm is None else torch.from_numpy(perm).cuda(),
                cursor=None if cursor is None else torch.tensor([cursor], dtype=torch.int64, device='cuda'))


def _check_planes(planes, want_bits, R, C):
    """planes [P, R + 1, ldp] against the pieces' bit patterns [P][R, C]: zeros from C on, the guard row untouched."""
    got = planes.view(torch.int16)
    for q, w in enumerate(want_bits):
        wt = torch.from_numpy(np.ascontiguousarray(w).view(np.int16)).cuda()
        differ = (got[q, :R, :C] != wt).nonzero()
        assert differ.numel() == 0, (q, len(differ), differ[:5].tolist())
    assert not got[:, :R, C:].any()
    assert (got[:, R] == GUARD).all()


def _guarded(pieces, R, ldp, dtype):
    planes = torch.empty(pieces, R + 1, ldp, dtype=dtype, device='cuda')
    planes.view(torch.int16).fill_(GUARD)
    return planes


@pytest.mark.parametrize('name', SPLIT_CASES)
def test_split_planes_bits(ops, name):
    c = _split_case(name, 3, np.random.RandomState(len(name)))
    planes = _guarded(3, c['R'], c['ldp'], torch.bfloat16)
    ops.split_planes(c['src'], c['ld'], c['R'], c['C'], planes, perm=c['perm'], cursor=c['cursor'])
    torch.cuda.synchronize()
    _check_planes(planes, PC.p3_split(c['x'][c['rows']]), c['R'], c['C'])


@pytest.mark.parametrize('name', list(SPLIT_CASES) + ['exp-null'])
def test_split_planes_h2_bits(ops, name):
    c = _split_case('vector' if name == 'exp-null' else name, 2, np.random.RandomState(len(name)))
    planes = _guarded(2, c['R'], c['ldp'], torch.float16)
    if name == 'exp-null':
        e, word = 0, None
    else:
        word = torch.full((2,), 77, dtype=torch.int32, device='cuda')
        ops.absmax_exp(c['src'], c['ld'], c['n_store'], c['C'], word)
        e = int(word[0])
        assert e == PC.block_exp(np.abs(c['x']).max())
        assert 2.0 ** 13 <= np.abs(c['x']).max() * 2.0 ** e < 2.0 ** 14
    ops.split_planes_h2(c['src'], c['ld'], c['R'], c['C'], planes, word, perm=c['perm'], cursor=c['cursor'])
    torch.cuda.synchronize()
    h1, h2 = PC.h2_split(c['x'][c['rows']], e)
    if name != 'exp-null':
        assert (np.abs(h2[h2 != 0]).min() < 2.0 ** -14) and (h2 == 0).any()      # denormal second pieces, and vanished ones
    assert (h1.view(np.uint16) == 0x8000).any() and (h1.view(np.uint16) == 0).any()          # -0 and +0
    _check_planes(planes, [h1.view(np.uint16), h2.view(np.uint16)], c['R'], c['C'])


def _exp_of(ops, src, ld, R, C):
    word = torch.full((2,), 77, dtype=torch.int32, device='cuda')
    ops.absmax_exp(src, ld, R, C, word)
    return int(word[0])


@pytest.mark.parametrize('name,dld,off', [('strided-vector', 6, 0), ('ld-odd', 7, 0), ('source-offset', 6, 1)])
def test_absmax_exp_strided(ops, name, dld, off):
    """ld > C with NaN and 1e30 in the padding: on the 16-byte path of a strided matrix (ld % 4 == 0, aligned) and for each
    reason for the scalar path.  The maximum in the first quad, in the ragged last quad of a row, negative, denormal."""
    R, C = 33, 50
    ld = C + dld
    rng = np.random.RandomState(5)
    base = np.full((R, ld), np.nan, np.float32)
    base[:, C::2] = 1e30
    base[:, :C] = rng.uniform(-1, 1, (R, C))
    assert _exp_of(ops, _place(base, off), ld, R, C) == PC.block_exp(np.abs(base[:, :C]).max()) == 14
    for (r, c), v in (((0, 0), 3.0e5), ((0, 3), -70000.0), ((R - 1, C - 1), 9.0e9), ((R - 1, C - 2), -2.0 ** 20),
                      ((17, 23), 2.0 ** 73), ((17, 24), -1.5 * 2.0 ** 74), ((5, 48), 3.0e38)):
        m = base.copy()
        m[r, c] = v
        assert _exp_of(ops, _place(m, off), ld, R, C) == PC.block_exp(abs(v)), (r, c, v)
    # a denormal maximum, a NaN beside it (ignored); an all-zero block; a block that holds an infinity
    tiny = np.where(np.isnan(base) | (base == 1e30), base, 0).astype(np.float32)
    tiny[:, :C] = np.ldexp(rng.uniform(-1, 1, (R, C)), -141).astype(np.float32)
    tiny[7, C - 1] = -2.0 ** -140
    tiny[8, 0] = np.nan
    assert PC.block_exp(2.0 ** -140) == 60 and _exp_of(ops, _place(tiny, off), ld, R, C) == 60
    zero = np.where(np.isnan(base) | (base == 1e30), base, 0).astype(np.float32)
    assert _exp_of(ops, _place(zero, off), ld, R, C) == 0
    for inf in (np.inf, -np.inf):
        m = base.copy()
        m[11, 13] = inf
        assert _exp_of(ops, _place(m, off), ld, R, C) == 0
    m = base.copy()
    m[2, 2], m[30, C - 1], m[9, 9] = np.nan, np.nan, -3.0
    assert _exp_of(ops, _place(m, off), ld, R, C) == PC.block_exp(3.0) == 12


def test_absmax_exp_dense_past_the_grid_cap(ops):
    """A dense matrix (ld == C, aligned) of more than 4 x 2048 x 256 quads: the loop with four loads in flight and the
    remainder loop behind it both run.  The maximum in the first quad, in the unrolled region, in both trips of the remainder."""
    R, C = 2601, 4032
    stride = 2048 * 256
    assert C % 4 == 0 and 5 * stride < R * (C // 4) < 6 * stride
    rng = np.random.RandomState(9)
    base = rng.uniform(-1, 1, (R, C)).astype(np.float32)
    d = torch.from_numpy(base).cuda()
    assert d.data_ptr() % 16 == 0
    assert _exp_of(ops, d, C, R, C) == 14
    quad = lambda r, c: r * (C // 4) + c // 4
    spots = (((0, 1), 3.0e5, 0), ((1000, 77), -9.0e9, 1), ((2080, 1000), 5.0e3, 3), ((2081, 100), -2.0 ** 30, 4),
             ((R - 1, C - 1), 7.0e7, 5))
    for (r, c), v, trip in spots:
        assert quad(r, c) // stride == trip, (r, c, quad(r, c) // stride)
        d[r, c] = v
        assert _exp_of(ops, d, C, R, C) == PC.block_exp(abs(v)), (r, c, v)
        d[r, c] = float(base[r, c])
    assert _exp_of(ops, d, C, R, C) == 14
