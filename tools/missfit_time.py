"""Time of one iteration of the Gaussian-mixture fit on partly observed rows (VMPLoop(..., miss=).step(): vmp_mix_finalize,
vmp_mixture_fit_pack, vmp_mixture_fit_pass and its reduction) at 25 % and at 0 % missing entries, with - on the same x, in the same
run - mixture_impute (x_out + resp) and one complete-data VMPLoop.step() as the yardsticks, and the streaming launch of the masked
iteration alone.

    python tools/missfit_time.py [--n 1000000] [--d 8] [--k 16] [--reps 30] [--warmup 5] [--out profiles/missfit_time.txt]

Device events around alternating blocks of calls after a warm-up of every path; medians over the blocks.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10 ** 6)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--reps', type=int, default=30, help='calls per timed block')
    ap.add_argument('--blocks', type=int, default=7, help='timed blocks per path (alternating)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'missfit_time.txt'), help="'' to print only")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('missfit_time.py needs a GPU: a time taken anywhere else says nothing')
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    V._lib.lib()
    N, D, K = a.n, a.d, a.k
    rng = np.random.Generator(np.random.PCG64(0))
    centres = rng.standard_normal((K, D)) * 6
    x = centres[rng.integers(0, K, N)] + rng.standard_normal((N, D))
    r0 = np.exp(rng.standard_normal((N, K)))
    dev = lambda v: torch.as_tensor(np.asarray(v, np.float32)).cuda()
    x, r0 = dev(x), dev(r0 / r0.sum(1, keepdims=True))
    m25 = torch.as_tensor((rng.random((N, D)) < 0.25).astype(np.uint8)).cuda()
    m0 = torch.zeros(N, D, dtype=torch.uint8, device='cuda')
    loops = {'25': _mix.VMPLoop(x, r0, V._lib.VMP_GMM, miss=m25), '0': _mix.VMPLoop(x, r0, V._lib.VMP_GMM, miss=m0),
             'plain': _mix.VMPLoop(x, r0, V._lib.VMP_GMM)}
    for lp in loops.values():
        lp.run(3)                                                       # every path is timed on a fitted posterior
    ipack = loops['plain'].impute_pack()

    paths = {
        'masked VMPLoop.step(), 25 % missing': loops['25'].step,
        'masked VMPLoop.step(),  0 % missing': loops['0'].step,
        'masked streaming launch + reduction alone, 25 % missing': loops['25'].estep,
        'mixture_impute 25 % missing, x_out + resp': lambda: _mix.mixture_impute(x, m25, ipack, want_logp=False, want_resp=True),
        'complete-data VMPLoop.step()': loops['plain'].step,
    }
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
    lines = ['masked mixture fit timing: N=%d D=%d K=%d, %d blocks x %d calls per path after %d warm-up calls, device events, us per call'
             % (N, D, K, a.blocks, a.reps, a.warmup),
             'device: %s' % torch.cuda.get_device_name(0),
             'missing fraction of the 25 %% mask: %.4f' % m25.float().mean().item()]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append('%-58s median %10.1f   min %10.1f   max %10.1f' % (name, med[name], min(ts), max(ts)))
    it = med['masked VMPLoop.step(), 25 % missing']
    lines.append('ratio masked step (25 %%) / mixture_impute (x_out + resp): %.2fx' % (it / med['mixture_impute 25 % missing, x_out + resp']))
    lines.append('ratio masked step (25 %%) / complete-data step:            %.2fx' % (it / med['complete-data VMPLoop.step()']))
    lines.append('ratio masked step (0 %%) / masked step (25 %%):              %.2fx' % (med['masked VMPLoop.step(),  0 % missing'] / it))
    nbytes = 4 * N * D + N * D + 4 * N * K + 4 * N * D                   # x, mask in; r, x_fill out
    bw = nbytes / (med['masked streaming launch + reduction alone, 25 % missing'] * 1e-6)
    lines.append('masked streaming launch: %.1f MB it must move -> %.2f TB/s = %.1f %% of the 8 TB/s HBM peak (call time incl. launch)'
                 % (nbytes / 1e6, bw / 1e12, 100 * bw / HBM_PEAK))
    lines.append('box-to-box spread: figures from one machine; boxes of the pool differ by a few per cent on the same code (README)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
