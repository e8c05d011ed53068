"""Times the test-time evaluation: the materialised path (svae.inference with nb_samples_te samples, then losses.*: experiments.evaluate)
against the streaming path (losses.streaming_metrics) where both fit, streaming alone at the sizes the materialised path cannot hold,
and the imputation measurement.  One process; warm-up runs, then the median of >= 5 timed regions (hipEvents around the whole call)
with the spread (min .. max), and the peak allocation of each call.  Prints one JSON line per measurement.

    python tools/eval_time.py [--quick] [--reps 5] [--budget-mib 256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    peak = 0
    for _ in range(reps):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    ts = np.array(ts)
    return {'median_ms': float(np.median(ts)), 'min_ms': float(ts.min()), 'max_ms': float(ts.max()), 'reps': reps, 'peak_mib': peak / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='N = 2e4 and 1e5 only, P = 5')
    ap.add_argument('--reps', type=int, default=5, help='timed regions per figure (at least 5)')
    ap.add_argument('--budget-mib', type=int, default=256)
    args = ap.parse_args()
    from vmp_for_svae_amd import experiments, losses
    from vmp_for_svae_amd.models import vae
    from vmp_for_svae_amd.training import SVAETrainer
    K, Ld, U, Dy, S = 16, 8, 50, 8, 100                                 # the C5 shape at nb_samples_te = 100
    budget = args.budget_mib << 20
    args.reps = max(5, args.reps)
    vae.reset_variables()
    tr = SVAETrainer(K, Ld, U, Dy, nb_samples=10, seed=0, stddev_init_nn=0.3)
    g = torch.Generator(device='cuda').manual_seed(0)

    def data(N):
        cen = torch.randn(K, Dy, device='cuda', generator=g) * 3
        lab = torch.randint(0, K, (N,), device='cuda', generator=g)
        y = cen[lab] + torch.randn(N, Dy, device='cuda', generator=g)
        return y.contiguous(), torch.nn.functional.one_hot(lab, K).float()[:, :8].contiguous()

    def report(what, N, r, **extra):
        print(json.dumps(dict(what=what, N=N, K=K, S=S, L=Ld, Dy=Dy, budget_mib=args.budget_mib, **r, **extra)), flush=True)

    N = 20_000
    y, lab = data(N)
    report('materialised', N, timed(lambda: experiments.evaluate(tr, y, lab, S), args.reps))
    report('streaming', N, timed(lambda: experiments.evaluate(tr, y, lab, S, streaming=True, max_workspace_bytes=budget), args.reps),
           rows_per_chunk=losses.plan_eval_chunks(N, K, S, Ld, Dy, budget))
    for mib in (64, 1024):                                              # does the chunk's x staying in the last-level cache show?
        report('streaming', N, timed(lambda: experiments.evaluate(tr, y, lab, S, streaming=True, max_workspace_bytes=mib << 20), args.reps),
               rows_per_chunk=losses.plan_eval_chunks(N, K, S, Ld, Dy, mib << 20), note='budget %d MiB' % mib)
    P = 5 if args.quick else 20
    mask = losses.generate_missing_data_mask(y, 0.1, seed=0)
    report('imputation materialised P=%d' % P, N, timed(lambda: experiments.evaluate_imputation(tr, y, mask, P, S), max(5, args.reps)))
    report('imputation streaming P=%d' % P, N, timed(lambda: experiments.evaluate_imputation(tr, y, mask, P, S, streaming=True,
                                                                                             max_workspace_bytes=budget), max(5, args.reps)))
    del y, lab, mask
    torch.cuda.empty_cache()
    for N in ((100_000,) if args.quick else (100_000, 1_000_000)):
        y, lab = data(N)
        report('streaming', N, timed(lambda: experiments.evaluate(tr, y, lab, S, streaming=True, max_workspace_bytes=budget), args.reps),
               rows_per_chunk=losses.plan_eval_chunks(N, K, S, Ld, Dy, budget))
        del y, lab


if __name__ == '__main__':
    main()
