"""Cost of the exact silhouette of a clustering of a latent space on the GPU (HipOps.silhouette -> dcahip_silhouette,
K-SILHOUETTE) at (n, d, k) = (68 579, 32, 16), (68 579, 32, 64) and (1 000 000, 32, 16).  The points are what a ReLU latent
looks like (bench_knn.latent_like: non-negative, 24 clusters far from the origin); the labels are k-means labels of them
(cluster.kmeans, one start, 20 iterations).  Device events, one warm-up, the median of the rounds.  Per shape:

  kernels_ms   dcahip_silhouette alone (its five or six launches; workspace and outputs allocated before);
  call_ms      HipOps.silhouette (allocations and the read-back of the status word and the sizes included);
  valu_bound   DESIGN 4.6's issue bound of the pair loop, t_bound = n^2 d / (PEAK / 4), and the fraction of it reached;
  knn          (a) dcahip_knn with k = 15 on the same points in the same process, alternating with the silhouette: the same
               distance loop with a top-k list in place of the square root and the double add;
  torch        (b) what a user would compose on the same device: torch.cdist in chunks of queries, then a double product with
               the one-hot label matrix, then a / b / s with tensor operations -- with compute_mode
               'donot_use_mm_for_euclid_dist' (the direct form) and with the default (the Gram form above 25 rows), the worst
               error of s of each against the kernel beside it.  Above 131 072 points it is timed on --torch-queries
               queries against all candidates and SCALED (the output says so);
  sklearn      (c) sklearn.metrics.silhouette_samples on 16 host threads on the first 8 192 points, SCALED by (n / 8 192)^2:
               a rough figure;
  share        at the first shape: the pair loop of the scan over one range (tools/microbench/silhouette_scan_share.hip,
               built into tools/_dbg/, not part of the library) with and without the square root, the conversion and the
               double add -- their share of the scan.

  python tools/bench_silhouette.py [--rounds 5] [--out profiles/silhouette_bench.json]
  python tools/bench_silhouette.py --build-only        # compile the share kernel (no GPU needed)"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PEAK_FP32_VALU = 157.3e12           # FLOP/s, the vector pipe of the MI355X (packed fp32 FMA)
THREADS = 16
SHARE_SRC = os.path.join(ROOT, 'tools', 'microbench', 'silhouette_scan_share.hip')
SHARE_LIB = os.path.join(ROOT, 'tools', '_dbg', 'libsilhouette_scan_share.so')


def build_share():
    """tools/_dbg/libsilhouette_scan_share.so from tools/microbench/silhouette_scan_share.hip, when absent or older."""
    from dca_amd import build
    deps = [SHARE_SRC, os.path.join(build.CSRC, 'knn_dist.hpp')]
    if os.path.exists(SHARE_LIB) and all(os.path.getmtime(SHARE_LIB) >= os.path.getmtime(d) for d in deps):
        return SHARE_LIB
    os.makedirs(os.path.dirname(SHARE_LIB), exist_ok=True)
    subprocess.check_call([build._hipcc(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '-fPIC', '-shared',
                           '-o', SHARE_LIB, SHARE_SRC])
    return SHARE_LIB


def _timed(fn):
    """Milliseconds of fn's work on the current stream, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _med(t):
    return sorted(t)[len(t) // 2]


def torch_silhouette(Z, codes, k, mode, chunk, queries=None):
    """The composition with tensor operations: s of the first `queries` points (all when None).  Per chunk of queries the
    [chunk, n] distances (torch.cdist), S = D.double() @ onehot.double(), then a / b / s."""
    n = Z.shape[0]
    onehot = torch.nn.functional.one_hot(codes.long(), k).to(torch.float64)
    counts = onehot.sum(dim=0)
    m = n if queries is None else min(queries, n)
    out = torch.empty(m, dtype=torch.float64, device=Z.device)
    for s0 in range(0, m, chunk):
        q = slice(s0, min(s0 + chunk, m))
        D = torch.cdist(Z[q], Z, compute_mode=mode)
        S = D.double() @ onehot
        own = codes[q].long()
        rows = torch.arange(S.shape[0], device=Z.device)
        n_own = counts[own]
        a = S[rows, own] / (n_own - 1).clamp(min=1)
        M = S / counts.clamp(min=1)
        M[:, counts == 0] = float('inf')
        M[rows, own] = float('inf')
        b = M.min(dim=1).values
        s = (b - a) / torch.maximum(a, b)
        out[q] = torch.where(n_own > 1, torch.where(torch.isnan(s), torch.zeros_like(s), s), torch.zeros_like(s))
    return out


def measure(ops, n, d, k, rounds, torch_queries, share):
    from dca_amd import hip
    from dca_amd.cluster import lloyd
    from bench_knn import latent_like
    dev = torch.device('cuda')
    Z = latent_like(n, d, dev)
    L, p = ops.L, hip.ptr
    # the labels: k-means from k rows of the data, 20 iterations
    wk = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device=dev)
    C = ops.kmeans_seed(Z, k, 0, 0, ws=wk)[1]
    codes = lloyd(ops, Z, C, 20, wk)[0].contiguous()
    del wk
    splits = ops.silhouette_splits(n, d, k)
    ws = torch.empty(max(ops.silhouette_workspace_bytes(n, d, k, 0), 16), dtype=torch.uint8, device=dev)
    o = dict(s=torch.empty(n, dtype=torch.float64, device=dev), a=torch.empty(n, dtype=torch.float64, device=dev),
             b=torch.empty(n, dtype=torch.float64, device=dev), nearest=torch.empty(n, dtype=torch.int32, device=dev),
             counts=torch.empty(k, dtype=torch.int32, device=dev), cm=torch.empty(k, dtype=torch.float64, device=dev),
             mean=torch.empty(1, dtype=torch.float64, device=dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def kernels():
        hip.check(L.dcahip_silhouette(p(Z), d, n, d, p(codes), k, 0, p(o['s']), p(o['a']), p(o['b']), p(o['nearest']),
                                      p(o['counts']), p(o['cm']), p(o['mean']), p(ws), p(status), hip.stream()), 'silhouette')

    def call():
        return ops.silhouette(Z, codes, k)
    kk = 15
    kws = torch.empty(int(L.dcahip_knn_workspace_bytes(n, n, d, kk, 0)), dtype=torch.uint8, device=dev)
    kidx = torch.empty(n, kk, dtype=torch.int32, device=dev)
    kd2 = torch.empty(n, kk, dtype=torch.float32, device=dev)

    def knn():
        hip.check(L.dcahip_knn(p(Z), d, n, p(Z), d, n, d, kk, 0, 0, p(kidx), p(kd2), kk, p(kws), p(status), hip.stream()), 'knn')
    _timed(kernels)
    _, r = _timed(call)
    _timed(knn)
    assert int(status.item()) == 0 and torch.equal(r['s'], o['s']) and torch.equal(r['nearest'], o['nearest'])
    tk, tc, tn = [], [], []
    for _ in range(rounds):
        tk.append(_timed(kernels)[0])
        tn.append(_timed(knn)[0])
        tc.append(_timed(call)[0])
    bound_ms = 1e3 * float(n) * n * d / (PEAK_FP32_VALU / 4.0)
    res = {'n': n, 'd': d, 'k': k, 'splits': splits, 'kernels_ms': round(_med(tk), 3), 'call_ms': round(_med(tc), 3),
           'mean_silhouette': float(o['mean'].item()), 'smallest_cluster': int(o['counts'].min().item()),
           'rounds_ms': {'kernels': [round(t, 3) for t in tk], 'call': [round(t, 3) for t in tc], 'knn': [round(t, 3) for t in tn]},
           'workspace_bytes': int(ws.numel()),
           'valu_bound': {'formula': 't_bound = n * n * d / (PEAK / 4), PEAK = 157.3e12 fp32 FLOP/s of the vector pipe; one pair = d '
                                     'packed lane-operations (d/2 v_pk_add_f32 + d/2 v_pk_fma_f32); the square root, the conversion '
                                     'and the double add of a pair are NOT in the bound',
                          't_bound_ms': round(bound_ms, 3), 'fraction_reached': round(bound_ms / _med(tk), 4)},
           'knn': {'what': 'dcahip_knn, k = 15, the same points, alternating with the silhouette', 'kernels_ms': round(_med(tn), 3),
                   'fraction_of_bound': round(bound_ms / _med(tn), 4), 'silhouette_over_knn': round(_med(tk) / _med(tn), 3)}}
    del kws, kidx, kd2
    # (b) the composition with tensor operations
    chunk = max(256, min(8192, (1 << 28) // n))                 # [chunk, n] floats: about 1 GiB with its double copy
    m = None if n <= 131072 else torch_queries
    res['torch'] = {'what': 'torch.cdist per chunk of %d queries, D.double() @ onehot.double(), a / b / s with tensor operations'
                            % chunk, 'queries_measured': m or n, 'scaled': m is not None}
    for name, mode in (('direct', 'donot_use_mm_for_euclid_dist'), ('gram', 'use_mm_for_euclid_dist_if_necessary')):
        torch_silhouette(Z, codes, k, mode, chunk, queries=min(n, chunk))                # warm-up
        tt = []
        for _ in range(rounds if m is None else max(1, min(rounds, 3))):
            ms, st = _timed(lambda: torch_silhouette(Z, codes, k, mode, chunk, queries=m))
            tt.append(ms)
        scale = 1.0 if m is None else n / float(m)
        fin = torch.isfinite(st)                                  # a composition may hand back non-finite values: counted apart
        err = float((st - o['s'][:st.shape[0]])[fin].abs().max().item()) if bool(fin.any()) else None
        D0 = torch.cdist(Z[:chunk], Z, compute_mode=mode)
        res['torch'][name] = {'compute_mode': mode, 'measured_ms': round(_med(tt), 3), 'total_ms': round(_med(tt) * scale, 3),
                              'rounds_ms': [round(t, 3) for t in tt], 'worst_error_of_s_against_the_kernel': err,
                              'non_finite_s': int((~fin).sum().item()),
                              'non_finite_distances_in_the_first_chunk': int((~torch.isfinite(D0)).sum().item()),
                              'kernel_speedup': round(_med(tt) * scale / _med(tk), 2)}
        del st, D0
    # (c) the host route, scaled: a rough figure
    from sklearn.metrics import silhouette_samples
    from threadpoolctl import threadpool_limits
    hm = min(8192, n)
    Zh, ch = Z[:hm].cpu().numpy(), codes[:hm].cpu().numpy()
    with threadpool_limits(limits=THREADS):
        t0 = time.perf_counter()
        hs = silhouette_samples(Zh, ch)
        dt = time.perf_counter() - t0
    res['sklearn'] = {'what': 'sklearn.metrics.silhouette_samples on the first %d points, %d host threads (the BLAS of its '
                              'pairwise-distance chunks)' % (hm, THREADS), 'points_measured': hm, 'measured_s': round(dt, 3),
                      'scaled': True, 'rough': True, 'scaled_total_s': round(dt * (n / float(hm)) ** 2, 1),
                      'note': 'measured on %d points and multiplied by (%d / %d)^2; mean s there %.4f' % (hm, n, hm, float(hs.mean())),
                      'kernel_speedup_over_scaled_host': round(dt * (n / float(hm)) ** 2 / (_med(tk) * 1e-3), 1)}
    if share is not None:
        fn = share.scan_share
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        out = torch.empty(splits * n, dtype=torch.float64, device=dev)
        t = {0: [], 1: []}
        for mode in (0, 1):
            hip.check(fn(p(Z), n, d, splits, mode, p(out), hip.stream()), 'scan_share')
        for _ in range(rounds):
            for mode in (0, 1):
                t[mode].append(_timed(lambda: hip.check(fn(p(Z), n, d, splits, mode, p(out), hip.stream()), 'scan_share'))[0])
        full, plain = _med(t[0]), _med(t[1])
        res['share'] = {'what': 'the pair loop over one range per split (%d splits), with (full) and without (plain) sqrtf + '
                                'convert + double add' % splits, 'full_ms': round(full, 3), 'plain_ms': round(plain, 3),
                        'share_of_sqrt_convert_add': round(1.0 - plain / full, 4),
                        'plain_fraction_of_bound': round(bound_ms / plain, 4), 'full_fraction_of_bound': round(bound_ms / full, 4),
                        'rounds_ms': {'full': [round(x, 3) for x in t[0]], 'plain': [round(x, 3) for x in t[1]]}}
    del Z, ws, o
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--torch-queries', type=int, default=32768)
    ap.add_argument('--large', type=int, default=1000000)
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'silhouette_bench.json'))
    args = ap.parse_args()
    lib = build_share()
    if args.build_only:
        print(lib)
        return
    from dca_amd.ops import HipOps
    ops = HipOps()
    share = ctypes.CDLL(lib)
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'data': 'ReLU-latent-like points: 24 clusters, centres relu(N(6, 2)), spread 0.3, fp32; labels: 20 Lloyd iterations from '
                   'k-means++ seeds', 'shapes': []}
    for i, (n, d, k) in enumerate(((68579, 32, 16), (68579, 32, 64), (args.large, 32, 16))):
        res['shapes'].append(measure(ops, n, d, k, args.rounds, args.torch_queries, share if i == 0 else None))
        print(json.dumps(res['shapes'][-1]), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
