"""Time one iteration of the diagonal-covariance mixture fit (csrc/vmp_diagfit.hip) at N = 1e6 for (D, K) in {(16,16), (32,16),
(64,16), (64,64)}, with and without r_out, against
  (a) the HBM floor of the bytes that form must move - 4 D N read, plus 4 K N written when r is stored - at 8 TB/s, and
  (b) the same iteration written in torch fp32 on the same device: the E-step on x - m in row chunks, the moments as r.T @ x and
      r.T @ x^2.
Device time from events around a batch of iterations enqueued back to back (the kernel path enqueues them in one call), median of
`--reps` batches after a warm-up; the torch iteration is timed the same way.  Writes a table to --out.

    python tools/diagfit_time.py --out profiles/diagfit_time.txt"""
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
    x = (c[z] + torch.randn(N, D, generator=g)).cuda()
    r0 = torch.zeros(N, K)
    r0[torch.arange(N), z] = 1.0
    r0 = (0.9 * r0 + 0.1 / K).cuda()
    return x, r0


def torch_iteration(x, x2, stats, prior, r, chunk):
    """stats (Nk, sx, sxx) -> theta -> r (written into `r`) -> the new stats, all fp32"""
    a0, b0, m0, g0, h0 = prior
    Nk, sx, sxx = stats
    D = x.shape[1]
    beta, alpha, a = b0 + Nk, a0 + Nk, g0 + Nk / 2
    xbar = sx / Nk.clamp_min(1e-30)[:, None]
    NS = (sxx - sx * xbar).clamp_min(0)
    m = (b0[:, None] * m0 + sx) / beta[:, None]
    b = h0 + 0.5 * (NS + (b0 * Nk / beta)[:, None] * (xbar - m0) ** 2)
    dg = torch.special.digamma
    c = dg(alpha) - dg(alpha.sum()) + 0.5 * (dg(a)[:, None] - torch.log(b)).sum(1) - D / (2 * beta)
    lbar = a[:, None] / b
    for i in range(0, x.shape[0], chunk):
        dev = x[i:i + chunk, None, :] - m[None, :, :]
        r[i:i + chunk] = torch.softmax(c[None, :] - 0.5 * (lbar[None, :, :] * dev * dev).sum(2), 1)
    return r.sum(0), r.t() @ x, r.t() @ x2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'diagfit_time.txt'))
    args = ap.parse_args()
    from vmp_for_svae_amd.models import _mix
    N = args.N
    lines = ['diagonal-covariance mixture fit: us per iteration at N = %d on %s (median [min, max] of %d batches of %d iterations)'
             % (N, torch.cuda.get_device_name(0), args.reps, args.iters),
             '%-8s %-6s %22s %12s %10s %26s %8s' % ('(D,K)', 'r_out', 'kernel us', 'HBM floor us', 'fraction', 'torch fp32 us', 'speed-up')]
    for D, K in SHAPES:
        x, r0 = make(N, D, K)
        loop = _mix.DiagLoop(x, r0)
        loop.run(3)
        x2 = x * x
        prior = loop.prior
        rbuf = torch.empty(N, K, device='cuda')
        chunk = max(1024, (1 << 26) // (K * D))                      # 256 MB per (chunk, K, D) fp32 temporary
        state = {'s': (r0.sum(0), r0.t() @ x, r0.t() @ x2)}

        def torch_run(n):
            for _ in range(n):
                state['s'] = torch_iteration(x, x2, state['s'], prior, rbuf, chunk)

        t_ref = timed(torch_run, 2, 3, 1)
        for want_r in (False, True):
            if want_r:
                def run(n):
                    for _ in range(n):
                        loop._iterate(1, True, False)
            else:
                def run(n):
                    loop._iterate(n, False, False)
            t = timed(run, args.iters, args.reps, 2)
            floor = (4.0 * D * N + (4.0 * K * N if want_r else 0.0)) / HBM * 1e6
            lines.append('%-8s %-6s %8.1f [%6.1f,%7.1f] %12.1f %10.3f %10.1f [%6.1f,%7.1f] %8.1f'
                         % ('(%d,%d)' % (D, K), 'yes' if want_r else 'no', t[0], t[1], t[2], floor, floor / t[0], t_ref[0], t_ref[1], t_ref[2],
                            t_ref[0] / t[0]))
            print(lines[-1], flush=True)
        del loop, x, x2, r0, rbuf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:2]))


if __name__ == '__main__':
    main()
