"""Cost of Louvain clustering of the neighbour graph on the GPU (dca_amd.community.louvain -> dcahip_graph_symmetrize,
dcahip_louvain_begin / dcahip_louvain_sweep, K-LOUVAIN) at (n, d, k) = (68 579, 32, 15) -- BASELINE configs[2]'s cell count --
and (1 000 000, 32, 15).  The points are what a ReLU latent looks like (tools/bench_knn.latent_like), the graph is
dcahip_knn's.  Per shape, in one process, device events, the median of --rounds:

  symmetrize_ms     dcahip_graph_symmetrize (the call alone, the read of 2m not included)
  sweep_first_ms    sweep 0 of level 0, from singletons (four launches)
  sweep_late_ms     sweep --late of level 0 (the labels as the sweeps before it left them; `late_done` says whether the level
                    had already ended there, in which case the figure is the cost of a no-op)
  torch_sweep_ms    sweep 0 composed from torch device operations in the same process: unique over 64-bit (vertex, community)
                    keys, index_add for k_{i,c}, scatter_reduce amax / amin for the choice, the three sums -- with DOUBLE
                    scores (torch has no 128-bit integers: not exact; `torch_moved` against `moved` says how far it agrees)
  levels            per level of one whole run: vertices, entries, sweeps, sweeps_ms, aggregate_ms (relabel + coarse graph,
                    torch device operations)
  run_ms            community.louvain on the device indices, everything included (host reads of the state too)
  sweep_bytes       what a sweep must move at least: per entry its column and the neighbour's label in the decision and again
                    in the sums (16 bytes), per vertex two row pointers twice, label, degree, total, the new label written
                    and read, the new total zeroed and added (60 bytes);  sweep_first_gbs = sweep_bytes / sweep_first_ms
  networkx          networkx.community.louvain_communities on the host on a --nx-n subsample's own graph (a rough figure:
                    another graph, one seed), with our modularity on the same subsample

  python tools/bench_louvain.py [--rounds 5] [--sizes 68579,1000000] [--out profiles/louvain_bench.json]"""
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
from dca_amd import community, hip                              # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402

med = lambda t: sorted(t)[len(t) // 2]


def torch_sweep(rowptr, col, rows, labels, ki, tot, twom, g):
    """Sweep 0 (moves to lower ids) from torch operations, double scores.  Returns (labels_new, moved, inside, tot2)."""
    n = labels.numel()
    lab = labels.long()
    cl = col.long()
    off = cl != rows
    key = rows[off] * n + lab[cl[off]]
    ukey, inv = torch.unique(key, return_inverse=True)
    kic = torch.zeros(ukey.numel(), dtype=torch.int64, device=key.device).index_add_(0, inv, torch.ones_like(inv))
    ur = torch.div(ukey, n, rounding_mode='floor')
    uc = ukey - ur * n
    own = lab[ur]
    M = float(twom) * community.R
    kid, totd = ki.double(), tot.double()
    kia = torch.zeros(n, dtype=torch.float64, device=key.device)
    kia[ur[uc == own]] = kic[uc == own].double()
    stay = kia * M - g * kid * (totd[lab] - kid)
    adm = uc < own
    ur, uc, kic = ur[adm], uc[adm], kic[adm]
    score = kic.double() * M - g * kid[ur] * totd[uc]
    best = torch.full((n,), -float('inf'), dtype=torch.float64, device=key.device).scatter_reduce(0, ur, score, 'amax')
    at = score == best[ur]
    best_c = torch.full((n,), n, dtype=torch.int64, device=key.device).scatter_reduce(0, ur[at], uc[at], 'amin')
    move = best > stay
    new = torch.where(move, best_c, lab)
    inside = (new[rows] == new[cl]).sum()
    tot_new = torch.zeros(n, dtype=torch.int64, device=key.device).index_add_(0, new, ki.long())
    return new, (new != lab).sum(), inside, (tot_new * tot_new).sum()


def measure(ops, n, d, k, rounds, late):
    dev = torch.device('cuda')
    Z = latent_like(n, d, dev)
    knn_ms, (idx, _) = _timed(lambda: ops.knn(Z, Z, k, self_offset=0))
    del Z
    L, p = ops.L, hip.ptr
    ws = torch.empty(max(ops.graph_symmetrize_workspace_bytes(n, k), 16), dtype=torch.uint8, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    colbuf = torch.empty(2 * n * k, dtype=torch.int32, device=dev)
    deg = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def sym():
        hip.check(L.dcahip_graph_symmetrize(p(idx), k, n, k, p(rowptr), p(colbuf), 2 * n * k, p(deg), p(ws), p(status),
                                            hip.stream()), 'graph_symmetrize')
    sym()
    t_sym = [_timed(sym)[0] for _ in range(rounds)]
    twom = int(rowptr[n].item())
    col = colbuf[:twom]
    g = 1024
    t_first, t_late, late_done, moved = [], [], None, None
    for _ in range(rounds + 1):
        lev = ops.louvain_level(rowptr, col, None, twom, g, 1000)
        torch.cuda.synchronize()
        t_first.append(_timed(lambda: lev.sweep(0))[0])
        moved = lev.read(0)['moved']
        for s in range(1, late):
            lev.sweep(s)
        late_done = bool(lev.read(late - 1)['done'])
        t_late.append(_timed(lambda: lev.sweep(late))[0])
    t_first, t_late = t_first[1:], t_late[1:]                  # the first round warms up
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), rowptr[1:] - rowptr[:-1])
    lev = ops.louvain_level(rowptr, col, None, twom, g, 1000)
    args = (rowptr, col, rows, lev.labels, lev.ki, lev.tot, twom, g)
    torch_sweep(*args)
    t_torch, out = [], None
    for _ in range(rounds):
        ms, out = _timed(lambda: torch_sweep(*args))
        t_torch.append(ms)
    torch_moved = int(out[1].item())
    del rows, out, args
    # the public call once to warm up, one whole run level by level, then the public call timed
    community.louvain(idx, ops=ops)
    levels, r, c, w, tw = [], rowptr, col, None, twom
    while len(levels) < 32:
        def sweeps():
            return community.run_level(ops, r, c, w, tw, g, 1000)
        ms_s, (labels, q_int, ns) = _timed(sweeps)
        ms_a, (cu, nc) = _timed(lambda: community.relabel(labels))
        if nc == r.numel() - 1:
            levels.append({'vertices': int(r.numel() - 1), 'entries': int(c.numel()), 'sweeps': int(ns),
                           'sweeps_ms': round(ms_s, 3), 'aggregate_ms': round(ms_a, 3), 'merged': False})
            break
        ms_b, (r2, c2, w2) = _timed(lambda: community.aggregate(r, c, w, cu, nc))
        levels.append({'vertices': int(r.numel() - 1), 'entries': int(c.numel()), 'sweeps': int(ns),
                       'sweeps_ms': round(ms_s, 3), 'aggregate_ms': round(ms_a + ms_b, 3), 'merged': True})
        r, c, w = r2, c2, w2
    community.louvain(idx, ops=ops)
    t_run, res = [], None
    for _ in range(rounds):
        ms, res = _timed(lambda: community.louvain(idx, ops=ops))
        t_run.append(ms)
    sweep_bytes = 16 * twom + 60 * n
    tot_s, tot_a = sum(l['sweeps_ms'] for l in levels), sum(l['aggregate_ms'] for l in levels)
    return {'n': n, 'd': d, 'k': k, 'two_m': twom, 'knn_ms': round(knn_ms, 3), 'symmetrize_ms': round(med(t_sym), 4),
            'sweep_first_ms': round(med(t_first), 4), 'sweep_late_ms': round(med(t_late), 4), 'late': late,
            'late_done': late_done, 'moved': int(moved), 'torch_sweep_ms': round(med(t_torch), 3), 'torch_moved': torch_moved,
            'torch_over_kernel': round(med(t_torch) / med(t_first), 1), 'levels': levels,
            'aggregate_share_of_levels': round(tot_a / (tot_s + tot_a), 4), 'run_ms': round(med(t_run), 3),
            'rounds_ms': {'symmetrize': [round(t, 4) for t in t_sym], 'sweep_first': [round(t, 4) for t in t_first],
                          'sweep_late': [round(t, 4) for t in t_late], 'torch_sweep': [round(t, 3) for t in t_torch],
                          'run': [round(t, 3) for t in t_run]},
            'clusters': int(len(res.sizes)), 'modularity': round(res.modularity, 6), 'n_levels': res.n_levels,
            'n_sweeps': res.n_sweeps, 'level_sizes': res.level_sizes, 'sweep_bytes': sweep_bytes,
            'sweep_first_gbs': round(sweep_bytes / med(t_first) * 1e-6, 1)}


def host_networkx(ops, m, d, k):
    import networkx as nx
    dev = torch.device('cuda')
    Z = latent_like(m, d, dev, seed=1)
    idx, _ = ops.knn(Z, Z, k, self_offset=0)
    ours = community.louvain(idx, ops=ops)
    G = nx.from_scipy_sparse_array(community.knn_adjacency(idx.cpu().numpy()))
    t0 = time.perf_counter()
    comms = nx.community.louvain_communities(G, weight='weight', seed=0)
    dt = time.perf_counter() - t0
    return {'what': 'networkx.community.louvain_communities(weight="weight", seed=0) on the host, one thread, on the graph of '
                    'a %d-point sample: a rough figure' % m, 'networkx': nx.__version__, 'n': m, 'k': k,
            'seconds': round(dt, 2), 'clusters': len(comms),
            'modularity': round(nx.community.modularity(G, comms, weight='weight'), 6),
            'ours_modularity': round(ours.modularity, 6), 'ours_clusters': int(len(ours.sizes))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--late', type=int, default=16)
    ap.add_argument('--sizes', type=str, default='68579,1000000')
    ap.add_argument('--nx-n', type=int, default=10000)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'louvain_bench.json'))
    args = ap.parse_args()
    ops = HipOps()
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'data': 'ReLU-latent-like points: 24 clusters, centres relu(N(6, 2)), spread 0.3, fp32; the graph of dcahip_knn',
           'shapes': []}
    for n in (int(s) for s in args.sizes.split(',')):
        res['shapes'].append(measure(ops, n, 32, 15, args.rounds, args.late))
        torch.cuda.empty_cache()
    if args.nx_n > 0:
        try:
            res['networkx'] = host_networkx(ops, args.nx_n, 32, 15)
        except ImportError:
            res['networkx'] = None
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
