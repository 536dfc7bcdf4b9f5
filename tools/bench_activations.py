"""Cost of the hidden activation in a C3 training step (bench.py's c3 network: ZINB-conddisp 64-32-64 on 20 000 genes, batch
norm): relu against hard_sigmoid, exponential, swish and gelu at batch 4096 (the K-STACK step launches) and at the
reference's batch of 32 (the single-workgroup chains).  Steps run as bench.py runs them -- the fit loop's shuffled order,
replayed from hipGraphs -- on one engine per activation, the activations interleaved round by round; ms per step is the
median over the rounds.  Fewer cells than c3 (the step does not depend on them) keep the set-up short.
  python tools/bench_activations.py [--cells 16384] [--rounds 5] [--out profiles/activations_bench.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import EpochRunner, graph_kernel_nodes               # noqa: E402
from dca_amd import prep, synth                                 # noqa: E402
from dca_amd.engine import Engine                               # noqa: E402
from dca_amd.ops import HipOps                                  # noqa: E402

NAMES = ('relu', 'hard_sigmoid', 'exponential', 'swish', 'gelu')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=16384)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda')
    n, G = args.cells, args.genes
    ops = HipOps()
    Y = synth.generate_counts(n, G, device=dev)
    counts = prep.cell_counts(ops, Y, n, G)
    sf = counts / counts.median()
    X, norm = prep.transform(ops, Y, n, G, sf, True, True, None, return_norm=True)
    res = {'workload': 'c3 network (zinb-conddisp 64-32-64, batch norm), %d x %d synthetic' % (n, G),
           'device': torch.cuda.get_device_name(0), 'ms_per_step': {}, 'relative_to_relu': {}}
    for B, steps in ((4096, 32), (32, 512)):
        runners = {}
        for name in NAMES:
            eng = Engine('zinb-conddisp', G, G, (64, 32, 64), True, 0.0, activation=name)
            eng.init_params(0)
            eng.attach_device_data(X, Y, sf, norm=norm)
            eng.reserve(B)
            eng.clip = 5.0
            eng.set_lr(1e-4)
            r = EpochRunner(eng, n, B, dev, max_epochs=(steps * (args.rounds + 1) * B) // n + 4)
            r.new_run(r.max_epochs)
            r.use_graph = False
            r.run(4)                                            # eager warm-up
            r.use_graph = True
            r.capture_all()
            r.run(steps)                                        # one untimed round through the graphs
            runners[name] = r
            (b, k), g = next(iter(r.graphs.items()))            # kernel launches per step: the same for every activation
            nodes = graph_kernel_nodes(g)
            res.setdefault('kernels_per_step', {}).setdefault('B%d' % B, {})[name] = None if nodes is None else nodes / k
        times = {name: [] for name in NAMES}
        for _ in range(args.rounds):
            for name in NAMES:
                torch.cuda.synchronize()
                t = time.perf_counter()
                runners[name].run(steps)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t) * 1e3 / steps)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        res['ms_per_step']['B%d' % B] = {k: round(v, 4) for k, v in med.items()}
        res['relative_to_relu']['B%d' % B] = {k: round(v / med['relu'], 4) for k, v in med.items()}
        res.setdefault('rounds_ms_per_step', {})['B%d' % B] = {k: [round(x, 4) for x in v] for k, v in times.items()}
        del runners
        torch.cuda.synchronize()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
