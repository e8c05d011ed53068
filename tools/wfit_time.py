"""Time of one iteration of the Gaussian-mixture fit on weighted rows (VMPLoop(..., weights=).step(): vmp_mix_finalize,
vmp_mixture_fit_pack, vmp_mixture_wfit_pass with its reduction and its one-wave sum) on complete rows and under a mask at 25 % and
0 % missing entries, with - on the same x, in the same run - the masked step (25 %, 0 %) and the complete-data step as the yardsticks,
and lower_bound() of a weighted loop (one K-sized launch: the pass left its data term) against that of a masked loop (a pass over x).

    python tools/wfit_time.py [--n 1000000] [--d 8] [--k 16] [--reps 30] [--warmup 5] [--out profiles/wfit_time.txt]

Device events around alternating blocks of calls after a warm-up of every path; medians over the blocks.  lower_bound() ends in a
scalar read-back, so its time includes one host synchronisation per call.  Needs a GPU."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wfit_time.txt'), help="'' to print only")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('wfit_time.py needs a GPU: a time taken anywhere else says nothing')
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
    w = dev(rng.choice(np.array([0.0, 0.25, 1.0, 3.0, 7.5]), size=N, p=[0.2, 0.2, 0.2, 0.2, 0.2]))
    G = V._lib.VMP_GMM
    loops = {'w': _mix.VMPLoop(x, r0, G, weights=w), 'w25': _mix.VMPLoop(x, r0, G, weights=w, miss=m25),
             'w0': _mix.VMPLoop(x, r0, G, weights=w, miss=m0), '25': _mix.VMPLoop(x, r0, G, miss=m25),
             '0': _mix.VMPLoop(x, r0, G, miss=m0), 'plain': _mix.VMPLoop(x, r0, G)}
    for lp in loops.values():
        lp.run(3)                                                       # every path is timed on a fitted posterior

    paths = {
        'weighted VMPLoop.step(), complete rows': loops['w'].step,
        'weighted masked VMPLoop.step(), 25 % missing': loops['w25'].step,
        'weighted masked VMPLoop.step(),  0 % missing': loops['w0'].step,
        'weighted streaming launch + reduction + sum alone, complete': loops['w'].estep,
        'masked VMPLoop.step(), 25 % missing': loops['25'].step,
        'masked VMPLoop.step(),  0 % missing': loops['0'].step,
        'complete-data VMPLoop.step()': loops['plain'].step,
        'lower_bound() of the weighted loop (complete rows)': loops['w'].lower_bound,
        'lower_bound() of the masked loop, 25 % missing': loops['25'].lower_bound,
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
    lines = ['weighted mixture fit timing: N=%d D=%d K=%d, %d blocks x %d calls per path after %d warm-up calls, device events, us per call'
             % (N, D, K, a.blocks, a.reps, a.warmup),
             'device: %s' % torch.cuda.get_device_name(0),
             'missing fraction of the 25 %% mask: %.4f   zero weights: %.4f' % (m25.float().mean().item(), (w == 0).float().mean().item())]
    med, spread = {}, {}
    for name, ts in times.items():
        med[name], spread[name] = statistics.median(ts), max(ts) / min(ts)
        lines.append('%-60s median %10.1f   min %10.1f   max %10.1f' % (name, med[name], min(ts), max(ts)))
    wc, w25, w0 = (med['weighted VMPLoop.step(), complete rows'], med['weighted masked VMPLoop.step(), 25 % missing'],
                   med['weighted masked VMPLoop.step(),  0 % missing'])
    m25t, m0t = med['masked VMPLoop.step(), 25 % missing'], med['masked VMPLoop.step(),  0 % missing']
    lines.append('ratio masked step (0 %%) / weighted step on complete rows:     %.2fx   (the weighted step factors nothing)' % (m0t / wc))
    lines.append('ratio weighted step on complete rows / complete-data step:    %.2fx' % (wc / med['complete-data VMPLoop.step()']))
    lines.append('ratio weighted masked step / masked step, 25 %% missing:       %.3fx   (max / min of the masked step: %.3f)'
                 % (w25 / m25t, spread['masked VMPLoop.step(), 25 % missing']))
    lines.append('ratio weighted masked step / masked step,  0 %% missing:       %.3fx   (max / min of the masked step: %.3f)'
                 % (w0 / m0t, spread['masked VMPLoop.step(),  0 % missing']))
    lines.append('ratio lower_bound() masked loop / weighted loop:              %.2fx'
                 % (med['lower_bound() of the masked loop, 25 % missing'] / med['lower_bound() of the weighted loop (complete rows)']))
    nbytes = 4 * N * D + 4 * N + 4 * N * K                              # x, w in; r out
    bw = nbytes / (med['weighted streaming launch + reduction + sum alone, complete'] * 1e-6)
    lines.append('weighted streaming launch, complete rows: %.1f MB it must move -> %.2f TB/s = %.1f %% of the 8 TB/s HBM peak (call time incl. launches)'
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
