"""Time and effect of starting a mixture fit from the data (models/_mix.py seed_centers / seed_assign; csrc/vmp_seed.hip) next to the
host-side random r_init of gmm.inference (torch.rand on a CPU generator, normalised, copied to the device), on the benchmark's
synthetic data (bench.py synth), and what each start costs the fit: iterations and final held-out score of
VMPLoop.run_until(x_val, 1e-4) from both.

    python tools/seed_time.py [--n 1000000] [--d 8] [--k 16] [--reps 10] [--warmup 3] [--out profiles/seed_time.txt]

Device events around alternating blocks of calls after a warm-up of every path, medians over 7 blocks (tools/missfit_time.py); the
host-side initialisation is timed with a host clock around work that ends in a device synchronise.  Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10 ** 6)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--val', type=int, default=1 << 16, help='held-out rows')
    ap.add_argument('--reps', type=int, default=10, help='calls per timed block')
    ap.add_argument('--blocks', type=int, default=7, help='timed blocks per path (alternating)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seed_time.txt'), help="'' to print only")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('seed_time.py needs a GPU: a time taken anywhere else says nothing')
    import bench
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm
    V._lib.lib()
    N, D, K = a.n, a.d, a.k
    xa, _ = bench.synth(N + a.val, D, K, a.seed)
    x, x_val = torch.as_tensor(xa[:N]).cuda(), torch.as_tensor(xa[N:]).cuda()
    centers, _, _ = _mix.seed_centers(x, K, a.seed)
    loop = _mix.VMPLoop.from_seed(x, K, V._lib.VMP_GMM, a.seed)
    loop.run(3)

    def host_init():
        r = gmm._dirichlet_init(N, K, a.seed, x.device)
        torch.cuda.synchronize()
        return r

    paths = {
        'seed_centers (K + 1 launches)': lambda: _mix.seed_centers(x, K, a.seed),
        'seed_assign (1 launch)': lambda: _mix.seed_assign(x, centers),
        'one VMPLoop.step()': loop.step,
    }
    for f in paths.values():
        for _ in range(a.warmup):
            f()
    host_init()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    host = []
    for _ in range(a.blocks):                               # alternate the paths: drift hits all of them alike
        for name, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)          # us per call
        t0 = time.perf_counter()
        host_init()
        host.append((time.perf_counter() - t0) * 1e6)
    lines = ['mixture initialisation timing: N=%d D=%d K=%d, %d blocks x %d calls per path after %d warm-up calls, device events, us per call'
             % (N, D, K, a.blocks, a.reps, a.warmup),
             'device: %s' % torch.cuda.get_device_name(0)]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append('%-58s median %10.1f   min %10.1f   max %10.1f' % (name, med[name], min(ts), max(ts)))
    lines.append('%-58s median %10.1f   min %10.1f   max %10.1f   (host clock, one call per block, ends in a synchronise)'
                 % ('host-side random r_init (torch.rand on the CPU + copy)', statistics.median(host), min(host), max(host)))
    dev_init = med['seed_centers (K + 1 launches)'] + med['seed_assign (1 launch)']
    step = med['one VMPLoop.step()']
    lines.append('device-side start (centres + assignment): %.1f us = %.2f iterations;  host-side start: %.1f iterations'
                 % (dev_init, dev_init / step, statistics.median(host) / step))
    round_bytes = N * (4 * D + 4 + 4)                                       # x, w in; w out (no mask)
    per_round = med['seed_centers (K + 1 launches)'] / (K + 1)
    lines.append('a round moves %.1f MB (x and w in, w out; the first reads no w, the last writes none): %.1f us per launch -> %.2f TB/s = %.1f %% '
                 'of the 8 TB/s HBM peak (call time incl. launches)' % (round_bytes / 1e6, per_round, round_bytes / (per_round * 1e-6) / 1e12,
                                                                     100 * round_bytes / (per_round * 1e-6) / HBM_PEAK))
    for name, mk in (('k-means++ start', lambda: _mix.VMPLoop.from_seed(x, K, V._lib.VMP_GMM, a.seed)),
                     ('random start', lambda: _mix.VMPLoop(x, gmm._dirichlet_init(N, K, a.seed, x.device), V._lib.VMP_GMM))):
        hist = mk().run_until(x_val, 1e-4)
        lines.append('run_until(x_val, 1e-4) from the %-16s %4d iterations, final held-out score %.4f nats per row (first check %.4f)'
                     % (name + ':', hist[-1][0], hist[-1][1], hist[0][1]))
    lines.append('box-to-box spread: figures from one machine; boxes of the pool differ by a few per cent on the same code (README)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
