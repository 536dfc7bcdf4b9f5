"""Cost of the exact neighbour search of a latent space on the GPU (HipOps.knn -> dcahip_knn, K-NEIGHBOURS) at
(n, d, k) = (68 579, 32, 15) -- BASELINE configs[2]'s cell count -- and at (1 000 000, 32, 15), or the largest n that fits
(halved until it does, the reason recorded).  The points are what a ReLU latent looks like: non-negative, 24 clusters far
from the origin.  Per shape:

  kernels_ms   device events around dcahip_knn alone (the three launches; workspace and outputs allocated before),
               one warm-up, the median of the rounds;
  call_ms      the same around HipOps.knn (allocations and the read-back of the status word included);
  splits       the library's choice, dcahip_knn_splits;
  valu_bound   the least time the packed-fp32 vector pipe could take and the fraction of it reached:
               a (query, candidate) pair costs d / 2 packed subtractions and d / 2 packed fused multiply-adds = d packed
               lane-operations; the part issues PEAK / 4 of them per second (a packed FMA lane-operation is 4 of the
               PEAK = 157.3e12 fp32 FLOP/s of the vector pipe), so t_bound = nq n d / (PEAK / 4), fraction = t_bound / kernels;
  host         sklearn.neighbors.NearestNeighbors(algorithm='brute', n_jobs=16) on the first --host-queries queries
               against all n candidates, SCALED to all queries (the output says so), and how many of those queries got
               the same neighbour lists from the GPU.

  python tools/bench_knn.py [--rounds 5] [--host-queries 2048] [--out profiles/knn_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dca_amd import hip                                         # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402

PEAK_FP32_VALU = 157.3e12           # FLOP/s, the vector pipe of the MI355X (packed fp32 FMA)
THREADS = 16


def _timed(fn):
    """Milliseconds of fn's work on the current stream, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def latent_like(n, d, dev, seed=0):
    """[n, d] fp32 on the device: 24 clusters with centres ~ N(6, 2) clipped at 0, spread 0.3, ReLU applied."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.clamp(6.0 + 2.0 * torch.randn(24, d, generator=g, device=dev), min=0.0)
    which = torch.randint(0, 24, (n,), generator=g, device=dev)
    return torch.relu(centres[which] + 0.3 * torch.randn(n, d, generator=g, device=dev)).contiguous()


def measure(ops, n, d, k, rounds, host_queries):
    dev = torch.device('cuda')
    Z = latent_like(n, d, dev)
    L, p = ops.L, hip.ptr
    splits = ops.knn_splits(n, n, d, k)
    ws = torch.empty(int(L.dcahip_knn_workspace_bytes(n, n, d, k, 0)), dtype=torch.uint8, device=dev)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, k, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def kernels():
        hip.check(L.dcahip_knn(p(Z), d, n, p(Z), d, n, d, k, 0, 0, p(idx), p(d2), k, p(ws), p(status), hip.stream()), 'knn')

    def call():
        return ops.knn(Z, Z, k, self_offset=0)
    _timed(kernels)
    _, (cidx, cd2) = _timed(call)
    assert int(status.item()) == 0 and torch.equal(cidx, idx) and torch.equal(cd2, d2)
    tk, tc = [], []
    for _ in range(rounds):
        tk.append(_timed(kernels)[0])
        tc.append(_timed(call)[0])
    med = lambda t: sorted(t)[len(t) // 2]
    bound_ms = 1e3 * float(n) * n * d / (PEAK_FP32_VALU / 4.0)
    res = {'n': n, 'd': d, 'k': k, 'splits': splits, 'kernels_ms': round(med(tk), 3), 'call_ms': round(med(tc), 3),
           'rounds_ms': {'kernels': [round(t, 3) for t in tk], 'call': [round(t, 3) for t in tc]},
           'workspace_bytes': int(ws.numel()),
           'valu_bound': {'formula': 't_bound = nq * n * d / (PEAK / 4), PEAK = 157.3e12 fp32 FLOP/s of the vector pipe; one pair '
                                     '= d packed lane-operations (d/2 v_pk_add_f32 + d/2 v_pk_fma_f32), 4 FLOP of PEAK each',
                          't_bound_ms': round(bound_ms, 3), 'fraction_reached': round(bound_ms / med(tk), 4)}}
    # the host baseline on a query subset, scaled
    from sklearn.neighbors import NearestNeighbors
    m = min(host_queries, n)
    Zh = Z.cpu().numpy()
    nn = NearestNeighbors(n_neighbors=k + 1, algorithm='brute', n_jobs=THREADS).fit(Zh)
    t0 = time.perf_counter()
    _, hidx = nn.kneighbors(Zh[:m])
    dt = time.perf_counter() - t0
    gidx = idx[:m].cpu().numpy()
    same = 0
    for q in range(m):                                          # sklearn returns the query itself among its k + 1
        row = [j for j in hidx[q].tolist() if j != q][:k]
        same += row == gidx[q].tolist()
    res['host'] = {'what': "sklearn.neighbors.NearestNeighbors(algorithm='brute', n_jobs=%d), k + 1 neighbours (the query "
                           "itself is among them)" % THREADS, 'threads': THREADS, 'queries_measured': m,
                   'measured_s': round(dt, 3), 'scaled': True, 'scaled_to_queries': n, 'scaled_total_s': round(dt * n / m, 2),
                   'note': 'measured on the first %d queries against all %d candidates and multiplied by %d / %d' % (m, n, n, m),
                   'queries_with_identical_lists': same,
                   'speedup_of_kernels_over_scaled_host': round(dt * n / m / (med(tk) * 1e-3), 1)}
    del Z, ws, idx, d2
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-queries', type=int, default=2048)
    ap.add_argument('--large', type=int, default=1000000)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'knn_bench.json'))
    args = ap.parse_args()
    ops = HipOps()
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'data': 'ReLU-latent-like points: 24 clusters, centres relu(N(6, 2)), spread 0.3, fp32', 'shapes': []}
    res['shapes'].append(measure(ops, 68579, 32, 15, args.rounds, args.host_queries))
    n, why = args.large, None
    while True:
        try:
            big = measure(ops, n, 32, 15, max(1, min(args.rounds, 3)), args.host_queries)
            break
        except torch.cuda.OutOfMemoryError as e:
            why = 'n = %d did not fit in device memory (%s); halved' % (n, str(e).split('.')[0])
            torch.cuda.empty_cache()
            n //= 2
    big['requested_n'] = args.large
    if why:
        big['reason_for_smaller_n'] = why
    res['shapes'].append(big)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
