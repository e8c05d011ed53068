"""Time the scoring pass of the diagonal-covariance mixture (csrc/vmp_diagscore.hip) at N = 1e6 for (D, K) in {(16,16), (32,16),
(64,16), (64,64)} in three forms - sum_out only; logp + resp; masked with 30 % missing and x_out - against
  (a) the same function written in torch fp32 on the same device (log1p on x - m in row chunks, logsumexp; the masked form with
      torch.where and a resp @ m fill),
  (b) vmp_mixture_diag_pass in its bound-only form at the same shape: the same cell count without the logarithm, and
  (c) the HBM floor of the bytes the form must move (4 D N read; + 4 N + 4 K N written; masked: + D N read and 4 D N written) at 8 TB/s.
Device time from events around a batch of launches enqueued back to back, median of `--reps` batches after a warm-up; the torch
function is timed the same way with fewer launches.  Writes a table to --out.

    python tools/diagscore_time.py --out profiles/diagscore_time.txt"""
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
    return x, (0.9 * r0 + 0.1 / K).cuda(), (torch.rand(N, D, generator=g) < 0.3).cuda()


def torch_score(x, pack, D, chunk, miss=None, want_resp=False, out=None):
    """sum_n logp_n (and resp, and the fill) from the pack's words, fp32"""
    m, g, h = pack[:, :D], pack[:, D:2 * D], pack[:, 2 * D:3 * D]
    logw, ah, c = pack[:, 3 * D], pack[:, 3 * D + 1], pack[:, 3 * D + 2]
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        xc = x[i:i + chunk]
        dev = xc[:, None, :] - m[None]
        lt = torch.log1p(g[None] * dev * dev)
        if miss is None:
            l = c[None] - ah[None] * lt.sum(2)
        else:
            o = ~miss[i:i + chunk, None, :]
            l = logw[None] + torch.where(o, h[None], 0.0).sum(2) - ah[None] * torch.where(o, lt, 0.0).sum(2)
        logp = torch.logsumexp(l, 1)
        total += logp.double().sum()
        if want_resp or miss is not None:
            resp = torch.exp(l - logp[:, None])
            if miss is not None:
                out[i:i + chunk] = torch.where(miss[i:i + chunk], resp @ m, xc)
    return total


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'diagscore_time.txt'))
    args = ap.parse_args()
    from vmp_for_svae_amd.models import _mix
    N = args.N
    lines = ['diagonal-covariance mixture scoring pass: us per launch at N = %d on %s (median [min, max] of %d batches of %d launches)'
             % (N, torch.cuda.get_device_name(0), args.reps, args.iters),
             '%-8s %-12s %24s %10s %9s %28s %8s %12s %8s' % ('(D,K)', 'form', 'kernel us', 'HBM floor', 'fraction', '(a) torch fp32 us', '(a)/k',
                                                        '(b) fit pass', 'k/(b)')]
    for D, K in SHAPES:
        x, r0, miss = make(N, D, K)
        loop = _mix.DiagLoop(x, r0)
        loop.run(3)
        pack = loop.predictive_pack()
        xo = torch.empty_like(x)
        chunk = max(1024, (1 << 26) // (K * D))                      # 256 MB per (chunk, K, D) fp32 temporary
        t_fit = timed(lambda n: [_mix.mixture_diag_pass(x, loop.pack, want_r=False, want_stats=False, want_bound=True) for _ in range(n)],
                      args.iters, args.reps, 2)
        forms = (('sum only', dict(want_logp=False, want_sum=True), None, False, 4.0 * D * N),
                 ('logp + resp', dict(want_resp=True), None, True, 4.0 * D * N + 4.0 * N + 4.0 * K * N),
                 ('masked fill', dict(miss=miss, want_fill=True), miss, False, 9.0 * D * N + 4.0 * N))
        for name, kw, mk, wr, nbytes in forms:
            t = timed(lambda n: [_mix.mixture_diag_score(x, pack, **kw) for _ in range(n)], args.iters, args.reps, 2)
            t_ref = timed(lambda n: [torch_score(x, pack, D, chunk, mk, wr, xo) for _ in range(n)], 2, 3, 1)
            floor = nbytes / HBM * 1e6
            lines.append('%-8s %-12s %9.1f [%6.1f,%7.1f] %10.1f %9.3f %11.1f [%7.1f,%8.1f] %8.1f %12.1f %8.2f'
                         % ('(%d,%d)' % (D, K), name, t[0], t[1], t[2], floor, floor / t[0], t_ref[0], t_ref[1], t_ref[2], t_ref[0] / t[0],
                            t_fit[0], t[0] / t_fit[0]))
            print(lines[-1], flush=True)
        del loop, x, xo, r0, miss
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:2]))


if __name__ == '__main__':
    main()
