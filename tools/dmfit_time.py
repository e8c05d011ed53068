"""Time one iteration of the diagonal mixture fit on partly observed and weighted rows (csrc/vmp_diagmfit.hip) at N = 1e6 for (D, K) in
{(16,16), (64,64)}: the weights-only, mask-only and combined forms of the pass (r left in the kernel), next to
  (a) the complete-row pass vmp_mixture_diag_pass (csrc/vmp_diagfit.hip, which this feature does not change) on the same x, and
  (b) the same masked and weighted iteration written in torch fp32 on the same device, in row chunks,
with the bytes each form must move (x 4 D, mask D, weights 4 per row).  Expectation to report against, not a gate: the weights-only form
adds 4 B/row of traffic and one multiply per (row, k) over the complete-row pass; the masked form adds D B/row and a third MFMA chain.
Device time from events around a batch of iterations enqueued back to back, median of `--reps` batches after a warm-up.

    python tools/dmfit_time.py --out profiles/dmfit_time.txt"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from diagfit_time import make, timed  # noqa: E402

SHAPES = [(16, 16), (64, 64)]
HBM = 8e12


def torch_iteration(x, obs, w, stats, prior, r, chunk):
    """stats (Nk, sx, sxx) of the completed rows -> theta -> r (written into `r`) -> the new stats, all fp32; obs (N,D) fp32 1 = observed
    or None, w (N,) or None"""
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
    hl = -0.5 * torch.log(lbar)
    for i in range(0, x.shape[0], chunk):
        dev = x[i:i + chunk, None, :] - m[None, :, :]
        if obs is not None:
            dev = dev * obs[i:i + chunk, None, :]
        l = c[None, :] - 0.5 * (lbar[None, :, :] * dev * dev).sum(2)
        if obs is not None:
            l = l + (1.0 - obs[i:i + chunk]) @ hl.t()
        r[i:i + chunk] = torch.softmax(l, 1)
    wr = r if w is None else r * w[:, None]
    Nk = wr.sum(0)
    if obs is None:
        return Nk, wr.t() @ x, wr.t() @ (x * x)
    xo = x * obs
    M = wr.t() @ (1.0 - obs)
    return Nk, wr.t() @ xo + M * m, wr.t() @ (xo * xo) + M * (m * m + 1.0 / lbar)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dmfit_time.txt'))
    args = ap.parse_args()
    from vmp_for_svae_amd.models import _mix
    N = args.N
    lines = ['diagonal mixture fit on masked / weighted rows: us per iteration at N = %d on %s, r left in the kernel (median [min, max] of '
             '%d batches of %d iterations); 30 %% of the entries missing, weights 0..3' % (N, torch.cuda.get_device_name(0), args.reps, args.iters),
             '%-8s %-14s %8s %24s %12s %10s %26s' % ('(D,K)', 'form', 'B/row', 'kernel us', 'HBM floor us', 'x parent', 'torch fp32 us')]
    for D, K in SHAPES:
        x, r0 = make(N, D, K)
        g = torch.Generator(device='cpu').manual_seed(1)
        miss = (torch.rand(N, D, generator=g) < 0.3).cuda()
        w = torch.randint(0, 4, (N,), generator=g).float().cuda()
        chunk = max(1024, (1 << 26) // (K * D))
        rbuf = torch.empty(N, K, device='cuda')
        parent = _mix.DiagLoop(x, r0)
        parent.run(3)
        t_parent = timed(lambda n: parent._iterate(n, False, False), args.iters, args.reps, 2)
        lines.append('%-8s %-14s %8d %8.1f [%6.1f,%7.1f] %12.1f %10s' % ('(%d,%d)' % (D, K), 'complete rows', 4 * D, t_parent[0], t_parent[1],
                                                                       t_parent[2], 4.0 * D * N / HBM * 1e6, '1.00'))
        print(lines[-1], flush=True)
        for form, mk, wk in (('weights', None, w), ('mask', miss, None), ('mask+weights', miss, w)):
            loop = _mix.DiagFitLoop(x, r0, miss=mk, weights=wk)
            loop.run(3)
            t = timed(lambda n: loop._iterate(n, False, False), args.iters, args.reps, 2)
            obs = None if mk is None else (~mk).float()
            xz = x if mk is None else x * obs
            state = {'s': tuple(s.float() for s in (loop.stats[:, 0], loop.stats[:, 1:1 + D], loop.stats[:, 1 + D:]))}

            def torch_run(n):
                for _ in range(n):
                    state['s'] = torch_iteration(xz, obs, wk, state['s'], loop.prior, rbuf, chunk)

            t_ref = timed(torch_run, 2, 3, 1)
            nbytes = 4 * D + (D if mk is not None else 0) + (4 if wk is not None else 0)
            lines.append('%-8s %-14s %8d %8.1f [%6.1f,%7.1f] %12.1f %10.2f %10.1f [%6.1f,%7.1f]'
                         % ('(%d,%d)' % (D, K), form, nbytes, t[0], t[1], t[2], nbytes * float(N) / HBM * 1e6, t[0] / t_parent[0], t_ref[0],
                            t_ref[1], t_ref[2]))
            print(lines[-1], flush=True)
            del loop, obs, xz
        del parent, x, r0, rbuf, miss, w
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
