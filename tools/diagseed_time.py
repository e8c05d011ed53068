"""Time the seeded start of the diagonal-covariance mixture on wide rows (csrc/vmp_diagseed.hip) at N = 1e6 for (D, K) in {(16,16),
(32,16), (64,16), (64,64)}:
  - the K + 1 launches of diag_seed_centers, against their HBM floor (K + 1) (4 N D + 8 N) bytes at 8 TB/s (a round reads x and w and
    writes w) and against
  - a torch restatement of D^2-seeding on the same device (K rounds of ((x - c)^2).sum(1), minimum, argmin of E / w; the
    exponentials of all rounds drawn beforehand, outside the timed region);
  - the one launch of diag_seed_assign, against nearest_center_r (torch.cdist in fp64), with the peak memory either allocates;
  - the peak memory DiagLoop.from_seed allocates next to x, with an explicit prior and with the default one (whose column means are
    default_diag_prior's x.double().mean(0), the constructor's, not the seeding's).
Device time from events around a batch of calls enqueued back to back, median of `--reps` batches after a warm-up.  Writes a table
to --out.

    python tools/diagseed_time.py --out profiles/diagseed_time.txt"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 16), (32, 16), (64, 16), (64, 64)]
HBM = 8e12


def make(N, D, K, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    c = torch.randn(K, D, generator=g) * 3
    z = torch.randint(0, K, (N,), generator=g)
    return (c[z] + torch.randn(N, D, generator=g)).cuda()


def torch_seeding(x, K, E):
    """D^2-seeding by the exponential race in torch fp32: E (K,N) = the exponentials of every round"""
    w = torch.ones(x.shape[0], device=x.device)
    idx = []
    for j in range(K):
        i = torch.argmin(torch.where(w > 0, E[j] / w, float('inf')))
        idx.append(i)
        d2 = ((x - x[i]) ** 2).sum(1)
        w = d2 if j == 0 else torch.minimum(w, d2)
    return torch.stack(idx), w


def timed(fn, iters, reps, warm):
    for _ in range(warm):
        fn(iters)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(iters)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def peak_mb(fn):
    """MB allocated at the peak of fn() above what is allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2.0 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'diagseed_time.txt'))
    args = ap.parse_args()
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    N = args.N
    lines = ['diagonal-covariance mixture seeded start: us per call at N = %d on %s (median [min, max] of %d batches of %d calls)'
             % (N, torch.cuda.get_device_name(0), args.reps, args.iters),
             '%-8s %26s %9s %8s %30s %8s | %22s %30s %8s | %9s %9s | %14s %14s'
             % ('(D,K)', 'K+1 launches us', 'HBM floor', 'fraction', 'torch D^2-seeding us', 'torch/k', 'assign launch us',
                'nearest_center_r us', 'ncr/k', 'assign MB', 'ncr MB', 'from_seed MB', '(default prior)')]
    for D, K in SHAPES:
        x = make(N, D, K)
        E = -torch.log(torch.rand(K, N, device='cuda').clamp_min(1e-30))
        t = timed(lambda n: [_mix.diag_seed_centers(x, K, 1) for _ in range(n)], args.iters, args.reps, 2)
        t_ref = timed(lambda n: [torch_seeding(x, K, E) for _ in range(n)], 2, 3, 1)
        del E
        cen = _mix.diag_seed_centers(x, K, 1)[0]
        t_a = timed(lambda n: [_mix.diag_seed_assign(x, cen) for _ in range(n)], args.iters, args.reps, 2)
        t_n = timed(lambda n: [_mix.nearest_center_r(x, cen) for _ in range(n)], 2, 3, 1)
        L.release_workspaces()
        m_a = peak_mb(lambda: _mix.diag_seed_assign(x, cen))
        m_n = peak_mb(lambda: _mix.nearest_center_r(x, cen))
        prior = _mix.default_diag_prior(x, K)
        L.release_workspaces()
        m_s = peak_mb(lambda: _mix.DiagLoop.from_seed(x, K, 1, prior=prior))
        L.release_workspaces()
        m_d = peak_mb(lambda: _mix.DiagLoop.from_seed(x, K, 1))
        floor = (K + 1) * (4.0 * N * D + 8.0 * N) / HBM * 1e6
        lines.append('%-8s %10.1f [%6.1f,%7.1f] %9.1f %8.3f %12.1f [%7.1f,%8.1f] %8.1f | %8.1f [%5.1f,%6.1f] %12.1f [%7.1f,%8.1f] %8.1f | %9.1f %9.1f | %14.1f %14.1f'
                     % ('(%d,%d)' % (D, K), t[0], t[1], t[2], floor, floor / t[0], t_ref[0], t_ref[1], t_ref[2], t_ref[0] / t[0],
                        t_a[0], t_a[1], t_a[2], t_n[0], t_n[1], t_n[2], t_n[0] / t_a[0], m_a, m_n, m_s, m_d))
        print(lines[-1], flush=True)
        del x, cen, prior
        torch.cuda.empty_cache()
    lines.append('memory: MB allocated at the peak of the call next to x (N D 4 bytes = %.0f MB at D = 64); (N,K) fp32 = %.0f MB at K = 64; '
                 'an (N,D) or (N,K) fp64 buffer at 64 would be %.0f MB' % (N * 64 * 4 / 2.0 ** 20, N * 64 * 4 / 2.0 ** 20, N * 64 * 8 / 2.0 ** 20))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:2]))


if __name__ == '__main__':
    main()
