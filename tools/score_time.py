"""Time of the streaming mixture score (student_t.mixture_logprob: vmp_mix_score_pack_t + vmp_mix_score) against the composition
it replaces - student_t.logprob_smm_mixture + torch.logsumexp, the only way to get the same N numbers before - on the same inputs
in the same process, and the streaming kernel's share of the HBM peak on the bytes it must move.

    python tools/score_time.py [--n 1000000] [--d 8] [--k 16] [--reps 50] [--warmup 10] [--out FILE]

Device events around alternating blocks of calls after a warm-up of both paths; medians over the blocks.  Needs a GPU."""
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
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('score_time.py needs a GPU: a time taken anywhere else says nothing')
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.distributions import student_t
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
    pack = _mix.score_pack_t(log_pi, mu, sigma, nu)

    paths = {
        'composition: logprob_smm_mixture + torch.logsumexp': lambda: torch.logsumexp(student_t.logprob_smm_mixture(x, mu, sigma, nu, log_pi), dim=1),
        'student_t.mixture_logprob (pack + streaming pass)': lambda: student_t.mixture_logprob(x, mu, sigma, nu, log_pi),
        'streaming pass alone, logp': lambda: _mix.mixture_score(x, pack, want_sum=False),
        'streaming pass alone, logp + sum': lambda: _mix.mixture_score(x, pack),
        'streaming pass alone, sum only': lambda: _mix.mixture_score(x, pack, want_logp=False),
        'streaming pass alone, logp + resp + sum': lambda: _mix.mixture_score(x, pack, want_resp=True),
    }
    new, old = paths['student_t.mixture_logprob (pack + streaming pass)'](), paths['composition: logprob_smm_mixture + torch.logsumexp']()
    diff = ((new.double() - old.double()).abs() / old.double().abs().clamp_min(1)).max().item()
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
    lines = ['mixture score timing: N=%d D=%d K=%d, %d blocks x %d calls per path after %d warm-up calls, device events, us per call'
             % (N, D, K, a.blocks, a.reps, a.warmup),
             'device: %s' % torch.cuda.get_device_name(0),
             'max |new - composition| / max(1, |composition|) over the %d rows: %.3e' % (N, diff)]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append('%-58s median %10.1f   min %10.1f   max %10.1f' % (name, med[name], min(ts), max(ts)))
    lines.append('speed-up of mixture_logprob over the composition: %.1fx'
                 % (med['composition: logprob_smm_mixture + torch.logsumexp'] / med['student_t.mixture_logprob (pack + streaming pass)']))
    for name, nbytes in (('streaming pass alone, sum only', 4 * N * D), ('streaming pass alone, logp', 4 * N * D + 4 * N)):
        bw = nbytes / (med[name] * 1e-6)
        lines.append('%s: %.1f MB it must move -> %.2f TB/s = %.1f %% of the 8 TB/s HBM peak (call time incl. launch; the kernel is bound by '
                     'its arithmetic, not by HBM)' % (name, nbytes / 1e6, bw / 1e12, 100 * bw / HBM_PEAK))
    lines.append('box-to-box spread: figures from one machine; boxes of the pool differ by a few per cent on the same code (README)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
