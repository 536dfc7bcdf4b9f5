"""K-PREP driver: dca/io.py:88-111 (``normalize``) on the GPU.

The reference preprocesses on the host with scanpy (filter_genes / filter_cells /
normalize_per_cell / log1p / scale), then Keras copies batches of the result to the device.
Here the raw counts are uploaded ONCE; gene / cell counts, size factors, log1p and the per-gene
z-score are streaming passes over the resident matrix (dcahip_prep_*), and the tensors the
training engine needs (X, Y, size factors) never leave HBM.  The host AnnData still receives
what the reference's ``normalize`` leaves behind -- ``adata.X`` (normalised), ``adata.raw``
(counts), ``obs['n_counts', 'size_factors']``, ``var['n_counts']`` -- so the function is a
drop-in for ``dca_amd.io.normalize``.

Index outputs (which genes / cells survive the filters) are bit-exact with the host path: the
sums are exact integer arithmetic.  The median of the library sizes is taken on the host
(``np.median`` over n values), exactly as the reference does.
"""
import numpy as np
import scipy.sparse as sp_sparse
import torch

from ._device import default_ops, device_of


def host_chunk_tensor(a):
    """A host chunk as a CPU tensor for the upload (read only here).  A read-only array (a select-everything subset of the
    AnnData stand-in shares its parent's matrix that way) is wrapped through a writeable VIEW: torch warns about -- and
    would misbehave on writes through -- non-writeable arrays, and nothing is written through this tensor."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not a.flags.writeable:
        v = a.view()
        try:
            v.flags.writeable = True
            a = v
        except ValueError:                  # the owner itself is read only (a memory map opened 'r', say): copy the chunk
            a = a.copy()
    return torch.from_numpy(a)



class DeviceData:
    """Preprocessed tensors resident on the device: X [n, ldx] (network input), Y [n, ldy]
    (raw counts, the loss target), sf [n] -- or, in the counts-resident form, the raw counts as CSR (csr: a CsrCounts)
    with sf and norm and no dense X / Y: the engine gathers each minibatch from it (Engine.attach_counts)."""

    def __init__(self, X, Y, sf, n, G, host_x=None, norm=None, csr=None):
        self.X, self.Y, self.sf, self.n, self.G = X, Y, sf, n, G
        self.csr = csr
        self.device = csr.device if csr is not None else getattr(X, 'device', None)
        # how X was made from Y (fac, do_log, mean, std: dca/io.py:99-109) -- lets the engine run the first layer on the
        # non-zero counts (Engine.attach_device_data); the compact byte store of Y is built once and kept here
        self.norm = norm
        self.compact = None
        # what adata.X held when these tensors were made: train() / predict() use the resident tensors only while the
        # host matrix still is that matrix (the reference always feeds the CURRENT adata.X, network.py:188-211)
        self.host_mark = fingerprint(host_x) if host_x is not None else None

    def matches(self, host_x):
        return self.host_mark is None or fingerprint(host_x) == self.host_mark

    def attach(self, eng):
        """Hands these tensors to the engine (the dense ones, or the CSR of the counts-resident form).  An engine that
        fits a gene subset (train(output_subset=...)) keeps its column map (Engine.out_cols) and gets it back here, so that
        the tiles of a later inference pass have the shapes of its network; the dense counts of all genes are no target
        for such a network and stay out (inference reads X only)."""
        subset = eng.lay.G_out != self.G
        if self.csr is not None:
            out_cols = getattr(eng, 'out_cols', None)
            if out_cols is not None and len(out_cols) == eng.lay.G_out:
                eng.attach_counts(self.csr, self.sf, self.norm, out_cols=out_cols)
            else:
                eng.attach_counts(self.csr, self.sf, self.norm)
        elif subset:
            eng.attach_device_data(self.X, None, self.sf, norm=self.norm, compact=False)
        else:
            eng.attach_device_data(self.X, self.Y, self.sf, norm=self.norm, compact=self.compact)


def fingerprint(X):
    """EXACT content mark of a host matrix: shape, dtype and a 64-bit hash of every byte (libdcahost, threaded: ~0.1 s for
    the 5.5 GB benchmark matrix; sparse matrices: of their data / indices / indptr arrays).  An in-place edit of any element
    between normalize() and train() / predict() changes it, and the resident tensors are then not used."""
    def mark(a):
        a = np.ascontiguousarray(a)
        try:
            from . import hostlib
            return hostlib.checksum(a)
        except (OSError, RuntimeError, AttributeError):          # no native host library (no compiler on the host): slower, same guarantee
            import hashlib
            return hashlib.blake2b(a.view(np.uint8).reshape(-1), digest_size=8).hexdigest()
    if hasattr(X, 'toarray'):
        # the arrays of the matrix' OWN format (no conversion; the format name is part of the mark: equal matrices in
        # another format or index order do not match, which only costs a re-upload)
        fmt = getattr(X, 'format', type(X).__name__)
        parts = [np.asarray(getattr(X, k)) for k in ('data', 'indices', 'indptr', 'row', 'col', 'offsets') if hasattr(X, k)]
        if not parts:
            parts = [np.asarray(X.tocsr().data)]
        return (tuple(X.shape), 'sparse', fmt) + tuple((str(p.dtype), mark(p)) for p in parts)
    Xa = np.asarray(X)
    return (tuple(Xa.shape), str(Xa.dtype), mark(Xa))


def _r4(x):
    return (x + 3) // 4 * 4


_STAGE = {}


def _stage_buffers(rows, cols):
    """Two page-locked [rows, cols] float32 buffers, kept for the life of the process (locking pages costs about as
    much as copying them)."""
    key = (rows, cols)
    if key not in _STAGE:
        _STAGE.clear()
        _STAGE[key] = [torch.empty(rows, cols, dtype=torch.float32).pin_memory() for _ in range(2)]
    return _STAGE[key]


def csr_capable(X, dev, ops):
    """Whether the host matrix X goes to `dev` as CSR (upload_sparse): a scipy.sparse matrix, a GPU, ops with the kernel."""
    return sp_sparse.issparse(X) and dev.type == 'cuda' and ops is not None and hasattr(ops, 'csr_expand')


def plan_csr_chunks(indptr, nnz_cap, row_cap):
    """Row chunks [(r0, r1), ...] of a CSR matrix with row pointer `indptr` (n + 1 entries, int32 or int64): consecutive,
    every row in exactly one, each of at most row_cap rows and at most nnz_cap entries -- except a chunk of ONE row, which
    holds its row whatever the row's length.  (Any indptr gives a plan; a malformed one is caught by the kernel.)"""
    indptr = np.asarray(indptr)
    n = len(indptr) - 1
    nnz_cap, row_cap = int(nnz_cap), int(row_cap)
    assert nnz_cap >= 1 and row_cap >= 1
    chunks = []
    r0 = 0
    while r0 < n:
        # the last row r1 with indptr[r1] - indptr[r0] <= nnz_cap (indptr ascending)
        r1 = int(np.searchsorted(indptr, int(indptr[r0]) + nnz_cap, side='right')) - 1
        r1 = max(r0 + 1, min(r1, r0 + row_cap, n))
        chunks.append((r0, r1))
        r0 = r1
    return chunks


_CSR_STAGE = {}


def _csr_stage(rows, nnz):
    """Two page-locked slots (indptr int32 [rows + 1], indices int32 [nnz], values fp32 [nnz]) for upload_sparse, kept
    for the life of the process apart from _stage_buffers' (which keeps one shape only); grown when a matrix needs more."""
    have = _CSR_STAGE.get('slots')
    if have is None or have[0][0].numel() < rows + 1 or have[0][1].numel() < nnz:
        rows = max(rows, have[0][0].numel() - 1 if have else 0)
        nnz = max(nnz, have[0][1].numel() if have else 0)
        _CSR_STAGE['slots'] = None
        _CSR_STAGE['slots'] = [(torch.empty(rows + 1, dtype=torch.int32).pin_memory(),
                                torch.empty(max(nnz, 1), dtype=torch.int32).pin_memory(),
                                torch.empty(max(nnz, 1), dtype=torch.float32).pin_memory()) for _ in range(2)]
    return _CSR_STAGE['slots']


def _pack(dst, src):
    """dst[:] = src converted to dst's dtype (round to nearest for floats, as np.asarray(src, float32) does); host threads
    for large same-dtype runs."""
    if src.dtype == dst.dtype and src.nbytes >= (1 << 20):
        from . import hostlib
        hostlib.parallel_copy(dst, np.ascontiguousarray(src))
    else:
        np.copyto(dst, src, casting='unsafe')


def pack_csr_chunk(X, r0, r1, indptr_out, indices_out, values_out):
    """Rows r0 .. r1 of the CSR matrix X into the given int32 / int32 / fp32 arrays (at least r1 - r0 + 1 and the chunk's
    entries long): chunk-relative indptr, column indices, values in fp32.  A matrix without canonical format is made
    canonical on a COPY of the chunk (sum_duplicates: duplicates add in the source dtype, as toarray() does); X is never
    modified.  Column indices that do not fit int32 are clamped to -1 (the kernel counts them).  Returns the chunk's nnz."""
    ip = X.indptr
    a, b = int(ip[r0]), int(ip[r1])
    rel = ip[r0:r1 + 1].astype(np.int64) - a
    idx, val = X.indices[max(a, 0):max(b, a, 0)], X.data[max(a, 0):max(b, a, 0)]
    if not X.has_canonical_format:
        sub = sp_sparse.csr_matrix((val.copy(), idx.copy(), rel.copy()), shape=(r1 - r0, X.shape[1]))
        sub.sum_duplicates()
        rel, idx, val = sub.indptr, sub.indices, sub.data
    m = len(idx)
    np.copyto(indptr_out[:r1 - r0 + 1], np.clip(rel, -1, 2 ** 31 - 1), casting='unsafe')
    if idx.dtype.itemsize > 4:
        idx = np.where((idx >= 0) & (idx < 2 ** 31), idx, -1)
    _pack(indices_out[:m], idx)
    _pack(values_out[:m], val)
    return m


def upload_sparse(X, dev, ops, ld, nnz_cap=1 << 22, row_cap=1 << 14):
    """scipy.sparse host matrix [n, G] -> new [n, ld] fp32 device tensor (ld >= G; pad columns zero), without a dense copy
    on the host: row chunks of the CSR arrays travel through two page-locked slots (chunk i + 1 is packed while chunk i
    crosses PCIe and dcahip_csr_expand writes its dense rows).  Bit for bit what the dense upload of X.toarray() gives.
    Other sparse formats are converted to CSR once.  A malformed matrix (a column outside [0, G), a bad indptr) raises
    ValueError."""
    n, G = X.shape
    if X.format != 'csr':
        X = X.tocsr()
    out = torch.empty(n, ld, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    ip = X.indptr.astype(np.int64, copy=False)
    if len(ip) != n + 1 or ip[0] != 0 or ip[-1] > len(X.indices) or len(X.data) != len(X.indices) or (np.diff(ip) < 0).any():
        # (checked here, O(n): scipy's own canonical-format test and the chunk slices trust indptr)
        raise ValueError('dca_amd: malformed sparse matrix: indptr is not a non-decreasing row pointer into its %d entries'
                         % len(X.indices))
    chunks = plan_csr_chunks(ip, max(int(nnz_cap), G), row_cap)
    cap = max(int(ip[r1] - ip[r0]) for r0, r1 in chunks)
    stage = _csr_stage(max(r1 - r0 for r0, r1 in chunks), cap)
    cap = stage[0][1].numel()
    dbuf = [(torch.empty(s[0].numel(), dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
             torch.empty(cap, dtype=torch.float32, device=dev)) for s in stage]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    events = [torch.cuda.Event() for _ in range(2)]
    for ci, (r0, r1) in enumerate(chunks):
        slot = ci % 2
        if ci >= 2:
            events[slot].synchronize()                 # the copies that last read this slot are done
        hp, hi, hv = stage[slot]
        m = pack_csr_chunk(X, r0, r1, hp.numpy(), hi.numpy(), hv.numpy())
        dp, di, dv = dbuf[slot]
        dp[:r1 - r0 + 1].copy_(hp[:r1 - r0 + 1], non_blocking=True)
        di[:m].copy_(hi[:m], non_blocking=True)
        dv[:m].copy_(hv[:m], non_blocking=True)
        events[slot].record()
        ops.csr_expand(dp, di, dv, m, r1 - r0, G, out[r0:r1], ld, status)
    torch.cuda.current_stream().synchronize()
    bad = int(status.item())
    if bad:
        raise ValueError('dca_amd: malformed sparse matrix: %d entries / rows outside the matrix (a column outside '
                         '[0, %d) or an indptr out of order)' % (bad, G))
    return out


# ---------------------------------------------------------------------------------------------------- counts-resident mode
class CsrCounts:
    """Raw counts resident on the device as CSR (include/dcahip.h, dcahip_csr_gather): indptr [n + 1] int64 (absolute
    offsets), indices [nnz] int32, values [nnz] fp32, canonical rows, n x G."""

    def __init__(self, indptr, indices, values, n, G):
        self.indptr, self.indices, self.values = indptr, indices, values
        self.n, self.G = int(n), int(G)
        self.nnz = int(values.numel())
        self.device = indptr.device
        self.compact_verdict = None         # compact.csr_verdict: whether / how these counts take a per-batch byte tile

    @property
    def nbytes(self):
        return self.indptr.numel() * 8 + self.nnz * 8


def dense_bytes(n, G):
    """Device bytes of the dense form of an n x G dataset: X and Y in fp32 ([n, r4(G)] each), the byte store (about one
    byte per element) and the first layer's per-cell table (about 1 KB per cell)."""
    return int(n) * _r4(int(G)) * 9 + int(n) * 1024


def counts_bytes(n, nnz):
    """Device bytes of the counts-resident form: the CSR (int64 row pointer, int32 column + fp32 value per entry)."""
    return (int(n) + 1) * 8 + int(nnz) * 8


RESIDENT_MODES = ('auto', 'counts', 'dense')


def choose_residency(mode, dense_need, counts_need, free, world=1, output_subset=False, use_raw_as_output=True,
                     has_norm=True, subset_gather=False):
    """'dense' or 'counts': where the counts of a dataset live on the device (EngineConfig.resident).  'dense' keeps
    today's [n, G] matrices; 'counts' keeps the CSR and gathers each minibatch.  'auto' stays dense whenever its estimate
    fits into `free` device bytes, and whenever counts mode cannot apply: data parallel (world > 1), an output_subset,
    use_raw_as_output=False, an input that is not a known function of the counts (has_norm=False).  Forcing 'counts' in
    one of those cases raises ValueError saying why.  subset_gather=True: the ops gather a gene subset from the CSR
    (csr_gather_cols, Engine.attach_counts(out_cols=...)), so an output_subset no longer stops counts mode."""
    if mode not in RESIDENT_MODES:
        raise ValueError('resident must be one of %s (got %r)' % (', '.join(RESIDENT_MODES), mode))
    if mode == 'dense':
        return 'dense'
    why = None
    if world > 1:
        why = 'data-parallel runs (%d ranks) keep dense residency' % world
    elif output_subset and not subset_gather:
        why = 'an output_subset needs the dense count matrix'
    elif not use_raw_as_output:
        why = 'use_raw_as_output=False trains on the normalised input, which is not kept'
    elif not has_norm:
        why = 'the input is not a known function of the counts (no normalisation description)'
    if mode == 'counts':
        if why is not None:
            raise ValueError('dca_amd: counts-resident mode does not apply: ' + why)
        return 'counts'
    if why is not None or dense_need <= free:
        return 'dense'
    return 'counts'


def device_budget(dev):
    """Bytes the caching allocator can still hand out on `dev`: the device's free memory plus what the allocator holds
    unused, within its per-process fraction."""
    free, total = torch.cuda.mem_get_info(dev)
    reserved, allocated = torch.cuda.memory_reserved(dev), torch.cuda.memory_allocated(dev)
    frac = torch.cuda.get_per_process_memory_fraction(dev) if hasattr(torch.cuda, 'get_per_process_memory_fraction') else 1.0
    return max(0, min(free + reserved - allocated, int(frac * total) - allocated))


def _nnz(X):
    """The stored entries of a sparse host matrix; 0 for a dense one (choose_residency does not use the counts' size, and
    counting the non-zeros of a dense matrix is a pass over all of it)."""
    return int(X.nnz) if sp_sparse.issparse(X) else 0


def residency(X, dev, ops, mode=None):
    """The residency of host matrix X on `dev` for K-PREP (choose_residency with the device's budget).  Counts mode needs
    ops with the CSR kernels; 'auto' without them stays dense."""
    if mode is None:
        from . import config as _config
        mode = _config.current().resident
    if mode == 'dense':
        return 'dense'
    import os
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if not hasattr(ops, 'csr_gather'):
        if mode == 'counts':
            raise ValueError('dca_amd: counts-resident mode needs the CSR kernels (ops %s has no csr_gather)'
                             % getattr(ops, 'name', type(ops).__name__))
        return 'dense'
    n, G = X.shape
    need = dense_bytes(n, G)
    if mode == 'auto':
        if dev.type != 'cuda' or world > 1:
            return 'dense'
        free = device_budget(dev)
        if need <= free:
            return 'dense'
        return choose_residency(mode, need, counts_bytes(n, _nnz(X)), free, world=world)
    return choose_residency(mode, need, 0, 0, world=world)


def compress_capable(X, dev, ops):
    """Whether the dense host matrix X becomes a CsrCounts on the device (upload_csr's device route): a GPU, ops with
    csr_compress, a 2-d numpy array of a dtype for which the device route gives the host route's arrays bit for bit.  The
    kernel stores what is non-zero AFTER the conversion to fp32, the host route what is non-zero before it: the same for
    float32, integers and booleans (a non-zero integer never rounds to 0.0f).  A non-zero float64 can round to 0.0f, which
    the host route keeps as a stored zero: float64 and every other dtype stay on the host route (float16 too: scipy.sparse
    refuses it, so there are no host arrays to equal and the refusal stays)."""
    if sp_sparse.issparse(X) or dev.type != 'cuda' or ops is None or not hasattr(ops, 'csr_compress'):
        return False
    if not isinstance(X, np.ndarray) or X.ndim != 2 or X.shape[0] == 0 or X.shape[1] == 0:
        return False
    return X.dtype == np.float32 or X.dtype.kind in 'biu'


def _compress_dense(X, dev, ops, chunk_rows):
    """upload_csr's device route (see there)."""
    n, G = X.shape
    ld = _r4(G)
    rows_cap = max(1, min(int(chunk_rows), n, (2 ** 31 - 1) // G))
    stage = _stage_buffers(rows_cap, G)
    dense = torch.empty(rows_cap, ld, dtype=torch.float32, device=dev)
    sidx = torch.empty(rows_cap * G, dtype=torch.int32, device=dev)
    sval = torch.empty(rows_cap * G, dtype=torch.float32, device=dev)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ends = [torch.zeros(1, dtype=torch.int64).pin_memory() for _ in range(2)]
    events = [torch.cuda.Event() for _ in range(2)]
    idx_parts, val_parts = [], []

    def collect(slot, base):
        # the chunk compressed last: its end offset (a read-back of one word), its entries out of the scratch
        events[slot].synchronize()
        end = int(ends[slot].item())
        idx_parts.append(sidx[:end - base].clone())
        val_parts.append(sval[:end - base].clone())
        return end

    base, prev = 0, None
    for ci, s in enumerate(range(0, n, rows_cap)):
        e = min(n, s + rows_cap)
        slot = ci % 2
        # (the copy that last read this page-locked slot belongs to chunk ci - 2, whose event collect() has waited for)
        _pack(stage[slot][:e - s].numpy(), X[s:e])
        dense[:e - s, :G].copy_(stage[slot][:e - s], non_blocking=True)
        if prev is not None:
            base = collect(prev, base)          # the device works on chunk ci - 1 and the copy of chunk ci meanwhile
        ops.csr_compress(dense, ld, e - s, G, base, indptr[s:e + 1], sidx, sval, status)
        ends[slot].copy_(indptr[e:e + 1], non_blocking=True)
        events[slot].record()
        prev = slot
    total = collect(prev, base)
    if int(status.item()):
        raise RuntimeError('dca_amd: csr_compress left %d entries unwritten' % int(status.item()))
    del dense, sidx, sval
    indices = idx_parts[0] if len(idx_parts) == 1 else torch.cat(idx_parts)
    del idx_parts
    values = val_parts[0] if len(val_parts) == 1 else torch.cat(val_parts)
    del val_parts
    assert indices.numel() == total
    return CsrCounts(indptr, indices, values, n, G)


def upload_csr(X, dev, ops, nnz_cap=1 << 22, row_cap=1 << 14, dense_rows=2048, device_compress=True):
    """Host matrix [n, G] -> a CsrCounts on `dev`.

    A scipy.sparse matrix is staged through the page-locked slots of upload_sparse (pack_csr_chunk: canonical rows, fp32
    values) without expanding it.  A malformed matrix raises ValueError.

    A dense matrix is compressed ON THE DEVICE when compress_capable() says so (device_compress=False: never): chunks of
    dense_rows rows cross PCIe through the page-locked double slots of the dense upload (_stage_buffers; host threads pack
    chunk i + 1 while chunk i is copied and compressed), dcahip_csr_compress writes the chunk's row pointer into the final
    indptr and its entries into a chunk-sized scratch, and one word read back per chunk tells how many there were; the
    pieces are joined on the device at the end.  The arrays equal the host route's bit for bit.  Peak device memory of this
    route: the larger of (the final CSR + the chunk scratch) and 1.5 x the final CSR, where the chunk scratch is the dense
    chunk and room for all of its elements as entries, dense_rows x G x 12 bytes (0.49 GB at 2 048 x 20 000); the dense
    matrix is never allocated.  Any other dense matrix (no GPU, ops without the kernel, float64, float16, ...) is compressed by
    scipy on the host and takes the sparse route."""
    n, G = X.shape
    if device_compress and compress_capable(X, dev, ops):
        return _compress_dense(X, dev, ops, min(int(dense_rows), int(row_cap)))
    if not sp_sparse.issparse(X):
        X = sp_sparse.csr_matrix(np.asarray(X))
    if X.format != 'csr':
        X = X.tocsr()
    ip = X.indptr.astype(np.int64, copy=False)
    if len(ip) != n + 1 or ip[0] != 0 or ip[-1] > len(X.indices) or len(X.data) != len(X.indices) or (np.diff(ip) < 0).any():
        raise ValueError('dca_amd: malformed sparse matrix: indptr is not a non-decreasing row pointer into its %d entries'
                         % len(X.indices))
    total = int(ip[-1])
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    values = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    base = 0
    if dev.type != 'cuda':
        for r0, r1 in plan_csr_chunks(ip, max(int(nnz_cap), G), row_cap):
            hp = np.empty(r1 - r0 + 1, np.int32)
            hi = np.empty(int(ip[r1] - ip[r0]), np.int32)
            hv = np.empty(int(ip[r1] - ip[r0]), np.float32)
            m = pack_csr_chunk(X, r0, r1, hp, hi, hv)
            indptr[r0:r1 + 1] = torch.from_numpy(hp.astype(np.int64) + base)
            indices[base:base + m] = torch.from_numpy(hi[:m])
            values[base:base + m] = torch.from_numpy(hv[:m])
            base += m
    elif n > 0:
        chunks = plan_csr_chunks(ip, max(int(nnz_cap), G), row_cap)
        cap = max(int(ip[r1] - ip[r0]) for r0, r1 in chunks)
        stage = _csr_stage(max(r1 - r0 for r0, r1 in chunks), cap)
        dptr = [torch.empty(sl[0].numel(), dtype=torch.int32, device=dev) for sl in stage]
        events = [torch.cuda.Event() for _ in range(2)]
        for ci, (r0, r1) in enumerate(chunks):
            slot = ci % 2
            if ci >= 2:
                events[slot].synchronize()
            hp, hi, hv = stage[slot]
            m = pack_csr_chunk(X, r0, r1, hp.numpy(), hi.numpy(), hv.numpy())
            dptr[slot][:r1 - r0 + 1].copy_(hp[:r1 - r0 + 1], non_blocking=True)
            indices[base:base + m].copy_(hi[:m], non_blocking=True)
            values[base:base + m].copy_(hv[:m], non_blocking=True)
            torch.add(dptr[slot][:r1 - r0 + 1].to(torch.int64), base, out=indptr[r0:r1 + 1])
            events[slot].record()
            base += m
        torch.cuda.current_stream().synchronize()
    csr = CsrCounts(indptr, indices[:base], values[:base], n, G)
    if n > 0:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.zeros(n, dtype=torch.float32, device=dev)
        ops.csr_row_sums(csr, out, status)
        bad = int(status.item())
        if bad:
            raise ValueError('dca_amd: malformed sparse matrix: %d entries / rows outside the matrix (a column outside '
                             '[0, %d) or an indptr out of order)' % (bad, G))
    return csr


def csr_gene_counts(ops, csr):
    """gene_counts of the dense matrix, bit for bit, from the CSR."""
    dev, n, G = csr.device, csr.n, csr.G
    R = ops.prep_chunks(n)
    part = torch.zeros(R * 2 * _r4(G), dtype=torch.float64, device=dev)
    sums = torch.zeros(G, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_col_pass(csr, None, False, part, status)
    ops.prep_col_finish(part, R, G, float(n), sums, None, None)
    return sums


def csr_cell_counts(ops, csr):
    """cell_counts of the dense matrix (exact for counts) from the CSR."""
    out = torch.zeros(csr.n, dtype=torch.float32, device=csr.device)
    ops.csr_row_sums(csr, out, torch.zeros(1, dtype=torch.int32, device=csr.device))
    return out


def subset_csr(ops, csr, rows=None, cols=None):
    """The resident CSR without the rows / columns that the boolean host masks `rows` [n] / `cols` [G] drop (None: keep
    all) -> a new CsrCounts, bit for bit upload_csr of the host matrix subset the same way (X[rows][:, cols]); the entries
    never leave the device (dcahip_csr_subset).  Device memory: the result is written into arrays of csr's size and cut to
    its own when entries were dropped."""
    dev = csr.device
    n_out = csr.n if rows is None else int(np.count_nonzero(rows))
    G_out = csr.G if cols is None else int(np.count_nonzero(cols))
    mask = lambda m, k: None if m is None else torch.from_numpy(                                  # noqa: E731
        np.ascontiguousarray(np.asarray(m).reshape(k) != 0).view(np.uint8)).to(dev)
    rk, ck = mask(rows, csr.n), mask(cols, csr.G)
    indptr = torch.zeros(n_out + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(csr.nnz, dtype=torch.int32, device=dev)
    values = torch.empty(csr.nnz, dtype=torch.float32, device=dev)
    ws = torch.empty(csr.n + csr.G, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_subset(csr, rk, ck, n_out, indptr, indices, values, ws, status)
    total = int(indptr[n_out].item())
    bad = int(status.item())
    if bad:
        raise ValueError('dca_amd: malformed resident CSR: %d entries / rows outside the matrix' % bad)
    if total < csr.nnz:
        indices, values = indices[:total].clone(), values[:total].clone()
    return CsrCounts(indptr, indices, values, n_out, G_out)


def csr_norm(ops, csr, fac, logtrans_input, normalize_input):
    """The description of transform()'s X for counts held as CSR: dict(fac, do_log, mean, std), mean / std bit for bit
    those of the dense pass (csr_col_pass's partials -> prep_col_finish)."""
    mean = std = None
    if normalize_input:
        dev, n, G = csr.device, csr.n, csr.G
        R = ops.prep_chunks(n)
        Gp = _r4(G)
        part = torch.zeros(R * 2 * Gp, dtype=torch.float64, device=dev)
        ops.csr_col_pass(csr, fac, logtrans_input, part, torch.zeros(1, dtype=torch.int32, device=dev))
        mean = torch.zeros(Gp, dtype=torch.float32, device=dev)
        std = torch.ones(Gp, dtype=torch.float32, device=dev)
        ops.prep_col_finish(part, R, G, float(n), None, mean, std)
    return dict(fac=fac, do_log=bool(logtrans_input), mean=mean, std=std)


def norm_args(norm):
    """(fac, do_log, mean, std) of a normalisation dict (csr_norm, transform(return_norm=True)): the operands the gather
    entries and the byte store's description of the network input take, in their order."""
    return norm.get('fac'), norm.get('do_log', False), norm.get('mean'), norm.get('std')


def download_csr(ops, csr, norm, chunk_rows=2048):
    """The normalised input X of counts held as CSR -> new host array [n, G]: row ranges gathered into one device tile and
    copied down (the dense matrix is never resident on the device)."""
    n, G = csr.n, csr.G
    dev = csr.device
    out = np.empty((n, G), dtype=np.float32)
    if n == 0:
        return out
    b = min(chunk_rows, n)
    ld = _r4(G)
    Yt = torch.empty(b, ld, dtype=torch.float32, device=dev)
    Xt = torch.empty(b, ld, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for s in range(0, n, b):
        e = min(n, s + b)
        ops.csr_gather(csr, None, None, s, e - s, None, *norm_args(norm), Yt, ld, Xt, ld, None, status)
        out[s:e] = Xt[:e - s, :G].cpu().numpy()
    return out


def _upload(X, dev, chunk_rows=2048, ops=None):
    """Host matrix -> [n, r4(G)] device tensor.  On a GPU the rows travel through two page-locked staging buffers:
    host threads fill buffer i + 1 (dcahost_parallel_copy) while buffer i crosses PCIe -- a pageable .to(device)
    of the 5.5 GB benchmark matrix moves ~13 GB/s, this ~45.  A scipy.sparse matrix goes as CSR (upload_sparse) when
    `ops` has the kernel."""
    n, G = X.shape
    if csr_capable(X, dev, ops):
        return upload_sparse(X, dev, ops, _r4(G))
    out = torch.zeros(n, _r4(G), dtype=torch.float32, device=dev)
    dense = not hasattr(X, 'toarray')
    staged = dev.type == 'cuda' and dense and X.dtype == np.float32 and X.flags['C_CONTIGUOUS'] and n * G >= (1 << 22)
    if not staged:
        for s in range(0, n, 8192):
            e = min(n, s + 8192)
            xs = X[s:e]
            xs = xs.toarray() if hasattr(xs, 'toarray') else np.asarray(xs)
            out[s:e, :G] = host_chunk_tensor(xs).to(dev)
        return out
    from . import hostlib
    chunk_rows = min(chunk_rows, n)
    stage = _stage_buffers(chunk_rows, G)
    events = [torch.cuda.Event() for _ in range(2)]
    for ci, s in enumerate(range(0, n, chunk_rows)):
        e = min(n, s + chunk_rows)
        slot = ci % 2
        if ci >= 2:
            events[slot].synchronize()                 # the copy that last read this buffer is done
        hostlib.parallel_copy(stage[slot][:e - s].numpy(), X[s:e])
        out[s:e, :G].copy_(stage[slot][:e - s], non_blocking=True)
        events[slot].record()
    torch.cuda.current_stream().synchronize()
    return out


def _download(X, n, G, chunk_rows=2048):
    """Device [n, >= G] tensor -> new host array [n, G] (the mirror of _upload)."""
    if X.device.type != 'cuda' or n * G < (1 << 22):
        return X[:n, :G].cpu().numpy()
    from . import hostlib
    out = np.empty((n, G), dtype=np.float32)
    chunk_rows = min(chunk_rows, n)
    stage = _stage_buffers(chunk_rows, G)
    events = [torch.cuda.Event() for _ in range(2)]
    prev = None
    for ci, s in enumerate(range(0, n, chunk_rows)):
        e = min(n, s + chunk_rows)
        slot = ci % 2
        stage[slot][:e - s].copy_(X[s:e, :G], non_blocking=True)
        events[slot].record()
        if prev is not None:
            ps, pe, pslot = prev
            events[pslot].synchronize()
            hostlib.parallel_copy(out[ps:pe], stage[pslot][:pe - ps].numpy())
        prev = (s, e, slot)
    if prev is not None:
        ps, pe, pslot = prev
        events[pslot].synchronize()
        hostlib.parallel_copy(out[ps:pe], stage[pslot][:pe - ps].numpy())
    return out


def gene_counts(ops, Y, n, G):
    dev = Y.device
    R = ops.prep_chunks(n)
    part = torch.zeros(R * 2 * _r4(G), dtype=torch.float64, device=dev)
    sums = torch.zeros(G, dtype=torch.float32, device=dev)
    ops.prep_col_pass(Y, Y.shape[1], n, G, None, False, None, 0, part)
    ops.prep_col_finish(part, R, G, float(n), sums, None, None)
    return sums


def cell_counts(ops, Y, n, G):
    out = torch.zeros(n, dtype=torch.float32, device=Y.device)
    ops.prep_row_sums(Y, Y.shape[1], n, G, out)
    return out


def transform(ops, Y, n, G, fac, logtrans_input, normalize_input, comm=None, return_norm=False):
    """X = scale(log1p(Y / fac)) on the device (each step optional).  With a communicator the
    per-gene statistics are those of all ranks' shards (data-parallel preprocessing).
    return_norm: also the description of the transform, (X, dict(fac, do_log, mean, std))."""
    dev = Y.device
    ld = Y.shape[1]
    X = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    R = ops.prep_chunks(n)
    Gp = _r4(G)
    part = torch.zeros(R * 2 * Gp, dtype=torch.float64, device=dev)
    ops.prep_col_pass(Y, ld, n, G, fac, logtrans_input, X, ld, part)
    mean = std = None
    if normalize_input:
        mean = torch.zeros(Gp, dtype=torch.float32, device=dev)
        std = torch.ones(Gp, dtype=torch.float32, device=dev)
        n_total = float(n)
        if comm is not None and comm.world > 1:
            tot = part.view(R, 2 * Gp).sum(dim=0)
            cnt = torch.tensor([n_total], dtype=torch.float64, device=dev)
            comm.all_reduce_sum(tot); comm.all_reduce_sum(cnt)
            n_total = float(cnt.item())
            ops.prep_col_finish(tot, 1, G, n_total, None, mean, std)
        else:
            ops.prep_col_finish(part, R, G, n_total, None, mean, std)
        ops.prep_scale(X, ld, n, G, mean, std)
    if return_norm:
        return X, dict(fac=fac, do_log=bool(logtrans_input), mean=mean, std=std)
    return X


def resident_counts(X, ops=None, device=None):
    """(Y, gene_totals): the host count matrix on the device and the exact integer total of every gene.  Y is a CsrCounts
    when the counts go counts-resident (residency()), else the dense [n, r4(G)] tensor."""
    ops = default_ops(ops)
    dev = torch.device(device) if device is not None else device_of(None, ops)
    n, G = X.shape
    if residency(X, dev, ops) == 'counts':
        csr = upload_csr(X, dev, ops)
        return csr, csr_gene_counts(ops, csr).cpu().numpy()
    Y = _upload(X, dev, ops=ops)
    return Y, gene_counts(ops, Y, n, G).cpu().numpy()


def normalize_device(adata, filter_min_counts=True, size_factors=True, normalize_input=True,
                     logtrans_input=True, ops=None, device=None, to_host=True, Y=None):
    """``io.normalize`` with the arithmetic on the device.  Returns (adata, DeviceData)."""
    from . import io as _io
    ops = default_ops(ops)
    dev = torch.device(device) if device is not None else device_of(None, ops)
    n, G = adata.X.shape
    if isinstance(Y, CsrCounts) and (Y.n, Y.G) == (n, G):
        return _normalize_counts(adata, filter_min_counts, size_factors, normalize_input, logtrans_input, ops, dev,
                                 to_host, Y)
    if Y is None and residency(adata.X, dev, ops) == 'counts':
        return _normalize_counts(adata, filter_min_counts, size_factors, normalize_input, logtrans_input, ops, dev,
                                 to_host, None)
    if Y is None or isinstance(Y, CsrCounts) or tuple(Y.shape) != (n, _r4(G)):
        Y = _upload(adata.X, dev, ops=ops)       # (else: resident_counts() uploaded these counts already)

    if filter_min_counts:                                         # io.py:90-92
        gc = gene_counts(ops, Y, n, G).cpu().numpy()
        adata.var['n_counts'] = gc
        keep = gc >= 1
        if not keep.all():
            _io._subset(adata, cols=keep)
            idx = torch.as_tensor(np.nonzero(keep)[0], device=dev)
            G = int(keep.sum())
            Yn = torch.zeros(n, _r4(G), dtype=torch.float32, device=dev)
            Yn[:, :G] = Y.index_select(1, idx)
            Y = Yn
        cc = cell_counts(ops, Y, n, G).cpu().numpy()
        adata.obs['n_counts'] = cc
        keep = cc >= 1
        if not keep.all():
            _io._subset(adata, rows=keep)
            Y = Y.index_select(0, torch.as_tensor(np.nonzero(keep)[0], device=dev)).contiguous()
            n = int(keep.sum())

    if size_factors or normalize_input or logtrans_input:         # io.py:94-97
        adata.raw = adata.copy()
    else:
        adata.raw = adata

    fac_d = None
    if size_factors:                                              # io.py:99-101 (normalize_per_cell)
        counts = cell_counts(ops, Y, n, G).cpu().numpy()
        adata.obs['n_counts'] = counts
        keep = counts >= 1
        if not keep.all():
            _io._subset(adata, rows=keep)
            Y = Y.index_select(0, torch.as_tensor(np.nonzero(keep)[0], device=dev)).contiguous()
            counts = counts[keep]
            n = int(keep.sum())
        after = np.median(counts)
        c2 = counts + (counts == 0)
        fac = (c2 / after).astype(np.float32)
        adata.obs['size_factors'] = adata.obs.n_counts / np.median(adata.obs.n_counts)
        fac_d = torch.as_tensor(fac).to(dev)
        sf_d = torch.as_tensor(np.asarray(adata.obs['size_factors'].values, dtype=np.float32)).to(dev)
    else:
        adata.obs['size_factors'] = 1.0
        sf_d = torch.ones(n, dtype=torch.float32, device=dev)

    if fac_d is not None or logtrans_input or normalize_input:
        X, norm = transform(ops, Y, n, G, fac_d, logtrans_input, normalize_input, return_norm=True)
    else:
        X, norm = Y, dict(fac=None, do_log=False, mean=None, std=None)
    if to_host:
        adata.X = _download(X, n, G)
    return adata, DeviceData(X, Y, sf_d, n, G, host_x=adata.X if to_host else None, norm=norm)


def _normalize_counts(adata, filter_min_counts, size_factors, normalize_input, logtrans_input, ops, dev, to_host, csr):
    """normalize_device in the counts-resident form: the statistics from the CSR kernels; each filter subsets the host
    AnnData as the dense form does and the RESIDENT CSR with it (subset_csr) -- or, with ops that lack csr_subset, uploads
    the subset host matrix again; the host AnnData ends up exactly as the dense form leaves it."""
    from . import io as _io
    n, G = adata.X.shape
    if csr is None:
        csr = upload_csr(adata.X, dev, ops)

    def filtered(csr, rows=None, cols=None):
        # (the host AnnData has been subset already)
        if hasattr(ops, 'csr_subset'):
            return subset_csr(ops, csr, rows=rows, cols=cols)
        return upload_csr(adata.X, dev, ops)
    if filter_min_counts:                                         # io.py:90-92
        gc = csr_gene_counts(ops, csr).cpu().numpy()
        adata.var['n_counts'] = gc
        keep = gc >= 1
        if not keep.all():
            _io._subset(adata, cols=keep)
            G = int(keep.sum())
            csr = filtered(csr, cols=keep)
        cc = csr_cell_counts(ops, csr).cpu().numpy()
        adata.obs['n_counts'] = cc
        keep = cc >= 1
        if not keep.all():
            _io._subset(adata, rows=keep)
            n = int(keep.sum())
            csr = filtered(csr, rows=keep)

    if size_factors or normalize_input or logtrans_input:         # io.py:94-97
        adata.raw = adata.copy()
    else:
        adata.raw = adata

    fac_d = None
    if size_factors:                                              # io.py:99-101 (normalize_per_cell)
        counts = csr_cell_counts(ops, csr).cpu().numpy()
        adata.obs['n_counts'] = counts
        keep = counts >= 1
        if not keep.all():
            _io._subset(adata, rows=keep)
            counts = counts[keep]
            n = int(keep.sum())
            csr = filtered(csr, rows=keep)
        after = np.median(counts)
        c2 = counts + (counts == 0)
        fac = (c2 / after).astype(np.float32)
        adata.obs['size_factors'] = adata.obs.n_counts / np.median(adata.obs.n_counts)
        fac_d = torch.as_tensor(fac).to(dev)
        sf_d = torch.as_tensor(np.asarray(adata.obs['size_factors'].values, dtype=np.float32)).to(dev)
    else:
        adata.obs['size_factors'] = 1.0
        sf_d = torch.ones(n, dtype=torch.float32, device=dev)

    norm = csr_norm(ops, csr, fac_d, logtrans_input, normalize_input)
    if to_host:
        adata.X = download_csr(ops, csr, norm)
    return adata, DeviceData(None, None, sf_d, n, G, host_x=adata.X if to_host else None, norm=norm, csr=csr)
