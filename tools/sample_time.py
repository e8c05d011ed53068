"""Time of the streaming mixture sampling (models/_mix.mixture_sample / mixture_draw: vmp_mixture_sample) at 25 % missing entries with
1 and 8 draws per row and in the unconditional form, with the streaming imputation (mixture_impute: vmp_mixture_impute) on the same x,
mask and parameters, in the same run, as the yardstick, and the bytes each pass must move.

    python tools/sample_time.py [--n 1000000] [--d 8] [--k 16] [--reps 20] [--warmup 5] [--out profiles/sample_time.txt]

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
    ap.add_argument('--reps', type=int, default=20, help='calls per timed block')
    ap.add_argument('--blocks', type=int, default=7, help='timed blocks per path (alternating)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_time.txt'), help="'' to print only")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('sample_time.py needs a GPU: a time taken anywhere else says nothing')
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    V._lib.lib()
    N, D, K = a.n, a.d, a.k
    rng = np.random.Generator(np.random.PCG64(0))
    centres = rng.standard_normal((K, D)) * 6
    A = rng.standard_normal((K, D, D)) / np.sqrt(D)
    sigma = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(D)
    x = centres[rng.integers(0, K, N)] + rng.standard_normal((N, D))
    w = rng.random(K) + 0.1
    dev = lambda v: torch.as_tensor(np.asarray(v, np.float32)).cuda()
    x, mu, sigma, nu, log_pi = dev(x), dev(centres), dev(sigma), dev(rng.uniform(2, 10, K)), dev(np.log(w / w.sum()))
    m25 = torch.as_tensor((rng.random((N, D)) < 0.25).astype(np.uint8)).cuda()
    ipack = _mix.impute_pack_t(log_pi, mu, sigma, nu)
    seed = 20260101

    paths = {
        'mixture_impute 25 % missing, x_out + logp (yardstick)': lambda: _mix.mixture_impute(x, m25, ipack),
        'mixture_sample 25 % missing, draws = 1': lambda: _mix.mixture_sample(x, m25, ipack, seed),
        'mixture_sample 25 % missing, draws = 1, with z': lambda: _mix.mixture_sample(x, m25, ipack, seed, want_z=True),
        'mixture_sample 25 % missing, draws = 8': lambda: _mix.mixture_sample(x, m25, ipack, seed, draws=8),
        'mixture_draw (nothing observed), n = N': lambda: _mix.mixture_draw(N, ipack, seed),
    }
    YARD = 'mixture_impute 25 % missing, x_out + logp (yardstick)'
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
    lines = ['mixture sampling timing: N=%d D=%d K=%d, %d blocks x %d calls per path after %d warm-up calls, device events, us per call'
             % (N, D, K, a.blocks, a.reps, a.warmup),
             'device: %s' % torch.cuda.get_device_name(0),
             'missing fraction of the 25 %% mask: %.4f' % m25.float().mean().item()]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append('%-58s median %10.1f   min %10.1f   max %10.1f' % (name, med[name], min(ts), max(ts)))
    for name in list(paths)[1:]:
        lines.append('ratio to mixture_impute: %-50s %.2fx' % (name, med[name] / med[YARD]))
    moved = ((YARD, 4 * N * D + N * D + 4 * N * D + 4 * N),                                            # x, mask in; x_out, logp out
             ('mixture_sample 25 % missing, draws = 1', 4 * N * D + N * D + 4 * N * D),                   # x, mask in; x_out out
             ('mixture_sample 25 % missing, draws = 8', 4 * N * D + N * D + 8 * 4 * N * D),
             ('mixture_draw (nothing observed), n = N', 4 * N * D))
    for name, nbytes in moved:
        bw = nbytes / (med[name] * 1e-6)
        lines.append('%s: %.1f MB it must move -> %.2f TB/s = %.1f %% of the 8 TB/s HBM peak (call time incl. launch)'
                     % (name, nbytes / 1e6, bw / 1e12, 100 * bw / HBM_PEAK))
    lines.append('box-to-box spread: figures from one machine; boxes of the pool differ by a few per cent on the same code (README)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
