"""Cost of one Lloyd iteration of k-means of a latent space on the GPU (HipOps.kmeans_step -> dcahip_kmeans_step, K-MEANS) at
(n, d) = (68 579, 32) -- BASELINE configs[2]'s cell count -- and (1 000 000, 32), k in {16, 64}.  The points are what a ReLU
latent looks like (tools/bench_knn.latent_like).  Per shape, in one process:

  (a) step_ms       one iteration of dcahip_kmeans_step (two launches): device events around --iters consecutive
                    iterations from the k-means++ seeds (HipOps.kmeans_bind: the arguments checked once, then the
                    entry point alone; the centres updated in place, no host read in between), divided by their number; one warm-up window, the median of the rounds;
  (b) composed_ms   the same iteration composed from the entry points the library had before K-MEANS: ops.knn(X, C, 1)
                    (three launches and the read of its status word) followed by ops.group_moments on X with
                    DCAHIP_NLL_MSE | DCAHIP_GROUP_NO_SF (the per-cluster sums in double; it also sums the squares, and the
                    division that gives the new centres is NOT included) -- the centres held fixed, --iters times between
                    the same events; alternated with (a) round by round;
  (c) sklearn_ms    scikit-learn's KMeans(algorithm='lloyd', init=<the same rows>, n_init=1, tol=0, max_iter=--host-iters)
                    on 16 host threads: fit time / n_iter_;
  a_over_b          (a) / (b): below 1 the fused step is the faster one.

  python tools/bench_kmeans.py [--rounds 5] [--iters 200] [--out profiles/kmeans_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_knn import latent_like, _timed                       # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402

THREADS = 16
NLL_MSE, GROUP_NO_SF = 8, 16


def measure(ops, Z, k, rounds, iters, host_iters):
    dev = Z.device
    n, d = Z.shape
    ws = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device=dev)
    rows, C0 = ops.kmeans_seed(Z, k, 0, 0, ws=ws)
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    labels, d2 = torch.empty(n, **i32), torch.empty(n, dtype=torch.float32, device=dev)
    counts, sums, inertia = torch.zeros(k, **i32), torch.zeros(k, d, **f64), torch.zeros(1, **f64)
    info, status = torch.zeros(3, **i32), torch.zeros(1, **i32)

    def fused():
        C = C0.clone()
        labels.fill_(-1)
        info.zero_()
        step = ops.kmeans_bind(Z, C, C, labels, d2, counts, sums, inertia, info, ws, status)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for it in range(1, iters + 1):
            step(it)
        b.record()
        b.synchronize()
        ops.kmeans_raise(status)
        return a.elapsed_time(b) / iters

    idx, kd2 = torch.empty(n, 1, **i32), torch.empty(n, 1, dtype=torch.float32, device=dev)
    s1, s2 = torch.zeros(k, d, **f64), torch.zeros(k, d, **f64)
    gws = torch.zeros(ops.group_moments_workspace_doubles(n, d, k), **f64)

    def composed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            ops.knn(Z, C0, 1, out=(idx, kd2))
            ops.group_moments(Z, d, None, idx, n, d, k, NLL_MSE | GROUP_NO_SF, s1, s2, d, gws)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    fused()
    composed()
    # the two compute the same assignment and the same sums from the same centres
    C = C0.clone()
    labels.fill_(-1)
    ops.kmeans_step(Z, C, C, labels, d2, counts, sums, inertia, info, 1, ws, status)
    s1.zero_()
    ops.knn(Z, C0, 1, out=(idx, kd2))
    ops.group_moments(Z, d, None, idx, n, d, k, NLL_MSE | GROUP_NO_SF, s1, s2, d, gws)
    torch.cuda.synchronize()
    assert torch.equal(idx[:, 0], labels) and torch.equal(kd2[:, 0], d2)
    sums_rel = float(((s1 - sums).abs().max() / sums.abs().max()).item())
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(fused())
        tb.append(composed())
    med = lambda t: sorted(t)[len(t) // 2]
    res = {'n': n, 'd': d, 'k': k, 'iters_per_window': iters, 'step_ms': round(med(ta), 4), 'composed_ms': round(med(tb), 4),
           'a_over_b': round(med(ta) / med(tb), 4),
           'rounds_ms': {'step': [round(t, 4) for t in ta], 'composed': [round(t, 4) for t in tb]},
           'launches': {'step': 2, 'composed': 4}, 'workspace_bytes': int(ws.numel()),
           'same_labels_and_d2_bits': True, 'sums_max_rel_difference': sums_rel}
    from sklearn.cluster import KMeans
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = None
    Zh = Z.cpu().numpy()
    init = Zh[rows.cpu().numpy()]
    km = KMeans(n_clusters=k, algorithm='lloyd', init=init, n_init=1, tol=0, max_iter=host_iters)
    t0 = time.perf_counter()
    if threadpool_limits is not None:
        with threadpool_limits(limits=THREADS):
            km.fit(Zh)
    else:
        km.fit(Zh)
    dt = time.perf_counter() - t0
    res['sklearn'] = {'what': "sklearn.cluster.KMeans(algorithm='lloyd', init=<the rows dcahip_kmeans_seed drew>, n_init=1, "
                              "tol=0, max_iter=%d), fit time / n_iter_" % host_iters,
                      'threads': THREADS if threadpool_limits is not None else int(os.environ.get('OMP_NUM_THREADS', 0)),
                      'fit_s': round(dt, 3), 'n_iter': int(km.n_iter_), 'sklearn_ms': round(1e3 * dt / km.n_iter_, 3),
                      'speedup_of_step_over_sklearn': round(1e3 * dt / km.n_iter_ / med(ta), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--host-iters', type=int, default=30)
    ap.add_argument('--sizes', type=str, default='68579,1000000')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'kmeans_bench.json'))
    args = ap.parse_args()
    ops = HipOps()
    import sklearn
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'sklearn': sklearn.__version__,
           'data': 'ReLU-latent-like points: 24 clusters, centres relu(N(6, 2)), spread 0.3, fp32', 'shapes': []}
    for n in (int(s) for s in args.sizes.split(',')):
        Z = latent_like(n, 32, torch.device('cuda'))
        for k in (16, 64):
            res['shapes'].append(measure(ops, Z, k, args.rounds, args.iters, args.host_iters))
        del Z
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
