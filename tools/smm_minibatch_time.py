"""Times the SMM-SVAE training step at the C5 minibatch shape (N = 64, K = 16, L = 8, Dy = 8, S = 10, U = 50; experiments.py:26,
154-176) on one GPU, in one process: the autograd step (direct_step=False) eagerly, the six-launch direct step eagerly, the direct
step replayed from a HIP graph with one and with four steps per replay, and - the yardstick - the GMM direct step replayed at the same
shape.  The variants take turns in rounds (warm-up first); prints one JSON line with the per-step median and spread of each.
--graphed-only: only the graphed SMM step (one step per replay), for a rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, K, Ld, Dy, S, U = 64, 16, 8, 8, 10, 50


def make(smm, direct=True):
    from vmp_for_svae_amd.models import vae
    from vmp_for_svae_amd.training import SVAETrainer
    vae.reset_variables()
    return SVAETrainer(K, Ld, U, Dy, nb_samples=S, lr=3e-4, stddev_init_nn=0.1, seed=1, smm=smm, dof=5.0, direct_step=direct)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000, help='timed steps per variant')
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--graphed-only', action='store_true')
    a = ap.parse_args()
    from vmp_for_svae_amd.training import GraphedSVAEStep
    y = torch.randn(N, Dy, device='cuda')
    variants = {}
    if a.graphed_only:
        g1 = GraphedSVAEStep(make(True), y)
        variants['smm_graphed_1'] = (lambda: g1(g1.y), 1)
    else:
        tr_a, tr_d = make(True, direct=False), make(True)
        variants['smm_autograd_eager'] = (lambda: tr_a.step(y), 1)
        variants['smm_direct_eager'] = (lambda: tr_d.step(y), 1)
        g1 = GraphedSVAEStep(make(True), y)
        variants['smm_graphed_1'] = (lambda: g1(g1.y), 1)
        g4 = GraphedSVAEStep(make(True), y, steps_per_replay=4)
        variants['smm_graphed_4'] = (lambda: g4(g4.ys), 4)
        gg = GraphedSVAEStep(make(False), y)
        variants['gmm_graphed_1'] = (lambda: gg(gg.y), 1)
    assert g1.table_mode and g1.tr._direct_ok(y, None, None, None, None)
    for fn, n in variants.values():
        for _ in range(max(1, a.warmup // n)):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    per_round = max(1, a.steps // a.rounds)
    for _ in range(a.rounds):
        for k, (fn, n) in variants.items():
            calls = max(1, per_round // n)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (calls * n) * 1e6)
    out = {'shape': dict(N=N, K=K, L=Ld, Dy=Dy, S=S, U=U), 'steps_per_variant': per_round * a.rounds, 'rounds': a.rounds}
    for k, ts in times.items():
        ts = sorted(ts)
        out[k + '_us'] = round(ts[len(ts) // 2], 2)
        out[k + '_spread_us'] = [round(ts[0], 2), round(ts[-1], 2)]
    if 'gmm_graphed_1_us' in out:
        out['smm_over_gmm_graphed'] = round(out['smm_graphed_1_us'] / out['gmm_graphed_1_us'], 3)
        out['direct_over_autograd_eager'] = round(out['smm_direct_eager_us'] / out['smm_autograd_eager_us'], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
