"""Time of the streaming pass of the variational lower bound (vmp_mixture_bound_pass) on complete rows and on a 25 % mask, against
its two yardsticks at the same shape in the same process: the mixture score with the sum only (vmp_mix_score: reads the bytes the
unmasked pass reads) and the fit pass on partly observed rows (vmp_mixture_fit_pass: the masked pass does a strict subset of its work).

    python tools/bound_time.py [--n 1000000] [--d 8] [--k 16] [--reps 50] [--blocks 7] [--warmup 10] [--out FILE]

Device events around alternating blocks of calls after a warm-up of every path; median, minimum and maximum over the blocks - the
spread of a yardstick is what a difference has to exceed.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10 ** 6)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--reps', type=int, default=50, help='calls per timed block')
    ap.add_argument('--blocks', type=int, default=7, help='timed blocks per path (alternating)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frac', type=float, default=0.25, help='share of missing entries of the masked paths')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('bound_time.py needs a GPU: a time taken anywhere else says nothing')
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    V._lib.lib()
    N, D, K = a.n, a.d, a.k
    rng = np.random.Generator(np.random.PCG64(0))
    centres = rng.standard_normal((K, D)) * 4
    x = (centres[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)
    miss = (rng.random((N, D)) < a.frac).astype(np.uint8)
    r0 = np.exp(rng.standard_normal((N, K))).astype(np.float32)
    r0 /= r0.sum(1, keepdims=True)
    xd, md, rd = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda(), torch.as_tensor(r0).cuda()
    loop = _mix.VMPLoop(xd, rd, V._lib.VMP_GMM, miss=md)                     # a posterior of these rows: three iterations of the masked fit
    loop.run(3)
    theta = loop.theta()
    fpack, spack = _mix.fit_pack(*theta), _mix.score_pack_niw(*theta)

    paths = {
        'yardstick: vmp_mix_score, sum only': lambda: _mix.mixture_score(xd, spack, want_logp=False),
        'bound pass, complete rows': lambda: _mix.mixture_bound(xd, None, fpack),
        'bound pass, complete rows, + lse': lambda: _mix.mixture_bound(xd, None, fpack, want_rows=True),
        'yardstick: vmp_mixture_fit_pass (r + stats)': lambda: _mix.mixture_fit_pass(xd, md, fpack),
        'bound pass, %.0f %% mask' % (100 * a.frac): lambda: _mix.mixture_bound(xd, md, fpack),
        'bound pass, %.0f %% mask, + lse' % (100 * a.frac): lambda: _mix.mixture_bound(xd, md, fpack, want_rows=True),
        'bound_terms (K-sized)': lambda: _mix.bound_terms(loop.prior, theta),
        'lower_bound (pack + pass + terms), %.0f %% mask' % (100 * a.frac): lambda: _mix.lower_bound(xd, theta, prior=loop.prior, miss=md),
    }
    names = list(paths)
    bound_full, bound_mask = paths[names[1]]()[0].item(), paths[names[4]]()[0].item()
    for f in paths.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.blocks):                               # alternate the paths: drift hits all of them alike
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)          # us per call
    lines = ['lower-bound pass timing: GMM N=%d D=%d K=%d, %d blocks x %d calls per path after %d warm-up calls, device events, us per call '
             '(call time incl. launches and the host wrapper)' % (N, D, K, a.blocks, a.reps, a.warmup),
             'device: %s' % torch.cuda.get_device_name(0),
             'data term: complete rows %.6f, masked %.6f (rows of the masked posterior; finite: %s)'
             % (bound_full, bound_mask, np.isfinite([bound_full, bound_mask]).all())]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append('%-58s median %10.1f   min %10.1f   max %10.1f   spread %5.1f %%'
                     % (name, med[name], min(ts), max(ts), 100 * (max(ts) - min(ts)) / med[name]))
    for new, old in ((names[1], names[0]), (names[4], names[3])):
        so = times[old]
        lines.append('%s / %s: %.2fx (yardstick spread %.1f %% of its median)'
                     % (new, old, med[new] / med[old], 100 * (max(so) - min(so)) / med[old]))
    for name, nbytes in ((names[1], 4 * N * D), (names[4], 5 * N * D)):
        bw = nbytes / (med[name] * 1e-6)
        lines.append('%s: %.1f MB it must move -> %.2f TB/s = %.1f %% of the 8 TB/s HBM peak' % (name, nbytes / 1e6, bw / 1e12, 100 * bw / HBM_PEAK))
    lines.append('box-to-box spread: figures from one machine; boxes of the pool differ by a few per cent on the same code (README)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
