"""Ill-conditioned data at converged fits: the generator, the cases and the fp64 truths shared by tests/test_mix_hard_truth.py (CPU: the
conditions that keep the comparison honest, asserted on the truth alone) and tests/test_mix_hard_gpu.py (the kernels against the
truth).  Not a test module.

Every other parity test of the mixture family draws isotropic unit-variance clusters five standard deviations apart and takes one or
two iterations from a random soft r0: every covariance the kernels factor there has a condition number of a few units.  Here the
clusters are elongated and randomly oriented (covariance condition `cond`), the columns are on scales `decades` decades apart, and
the step that is compared starts from the posterior a fit has CONVERGED to: components that have lost their rows, log rho of
hundreds, and rows that sit between two components.

  hard()        the generator
  CASES         the cases of the plain loop, by name; DIAG_CASES those of the diagonal fit
  converged()   T_ITER fp64 iterations of oracle.mixtures from r0, (r, u) rounded to fp32, one same-input step from them in fp64 and in
                the reference's own fp32, and the fp32 oracle's error on every compared quantity
  bar_r(), bar_theta()   the project's rule (tests/test_mix_gpu.py, tests/mix_pass_truth.py): r 1e-5 absolute or the fp32 oracle's
                own error where THAT is larger; alpha, beta, m, C, v 1e-5 relative or twice the fp32 oracle's; u 2e-5 relative
  masked(), weighted(), diag()   the inputs of the other loops, started from the same fp32-rounded posterior, and the truths of
                mix_missfit_truth / mix_wfit_truth / mix_diag_truth on them"""
import functools

import numpy as np
import torch

KAPPA = 5.0
T_ITER = 40
NAMES = ('alpha', 'beta', 'm', 'C', 'v')


def hard(N, D, K, cond, decades, spread, seed, offset=None):
    """(x, r0) fp32.  K centres spread * N(0, I); per cluster a random orthogonal Q (QR of a Gaussian matrix) and standard deviations
    cond ** (-j / (2 (D - 1))), j = 0 .. D-1 (covariance condition `cond`); the whole table multiplied column-wise by
    10 ** (decades (j / (D - 1) - 0.5)); r0 as tests/test_mix_gpu._synth draws it.  offset = (column, value): that constant added to
    one column after the scaling."""
    rng = np.random.Generator(np.random.PCG64(seed))
    j = np.arange(D) / max(D - 1, 1)
    c = spread * rng.standard_normal((K, D))
    z = rng.integers(0, K, size=N)
    sd = float(cond) ** (-0.5 * j)
    x = np.empty((N, D))
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        rows = np.nonzero(z == k)[0]
        x[rows] = c[k] + (rng.standard_normal((len(rows), D)) * sd) @ Q.T
    x *= 10.0 ** (decades * (j - 0.5))
    if offset is not None:
        x[:, offset[0]] += offset[1]
    r0 = np.exp(3.0 * rng.standard_normal((N, K)))
    r0 /= r0.sum(1, keepdims=True)
    return x.astype(np.float32), r0.astype(np.float32)


# name -> hard()'s arguments.  N, D, K, cond and decades are the smallest at which each kernel form is reached (asserted on
# vmp_mix_pass_plan by the GPU file); `spread` and `seed` are tuned per case until the posterior the step starts from keeps enough soft
# rows (tests/test_mix_hard_truth.py).
CASES = {
    'xdl_d8k16': dict(N=2049, D=8, K=16, cond=1e4, decades=3, spread=0.5, seed=2),
    'xdl_d2k3': dict(N=2049, D=2, K=3, cond=1e6, decades=0, spread=1.0, seed=2),
    'tiled_d5k17': dict(N=1031, D=5, K=17, cond=1e4, decades=2, spread=0.5, seed=3),
    'tiled_d3k33': dict(N=1031, D=3, K=33, cond=1e4, decades=2, spread=1.0, seed=4),
    'mom2_d8k16': dict(N=65537, D=8, K=16, cond=1e4, decades=3, spread=0.5, seed=5),
    'auto_d4k5': dict(N=2049, D=4, K=5, cond=1e4, decades=3, spread=2.5, seed=11, offset=(1, 1e3)),
    'fit_d5k7': dict(N=1031, D=5, K=7, cond=1e4, decades=2, spread=1.0, seed=7),
}
# The Gaussian fit of the D = 8 tables collapses: between its 5th and its 8th iteration from r0 all but one or two of the 16 components
# lose every row, and every row that is left is one-hot - whatever spread and seed (measured for spread 0.3 .. 3).  A comparison of r
# would then compare zeros and ones.  These cases stop the GAUSSIAN fit before that, at the last iteration that still has soft rows;
# the Student-t fit of the same tables runs all T_ITER iterations.  (name, smm) -> iterations, T_ITER where absent.
ITERATIONS = {('xdl_d8k16', False): 5, ('mom2_d8k16', False): 4, ('mom2_d8k16', True): 4}
LOOP_CASES = ('xdl_d8k16', 'xdl_d2k3', 'tiled_d5k17', 'tiled_d3k33', 'mom2_d8k16', 'auto_d4k5')
ACCURATE_CASES = ('xdl_d8k16', 'tiled_d5k17')
FIT_CASE = 'fit_d5k7'                  # the masked and the weighted loop
SURFACE_CASE = 'xdl_d8k16'             # score, impute, bound; the free-running loops
AUTO_CASE = 'auto_d4k5'                # columns decades apart and one far from zero, as weight next to acceleration
FLAVOURS = ('gmm', 'smm')


@functools.lru_cache(maxsize=None)
def data(name):
    return hard(**CASES[name])


def _step(x, r, u, smm):
    """one oracle step over row chunks: (r, u or None, theta[:5])"""
    from oracle import mixtures
    if smm:
        r1, u1, th, _ = mixtures.smm_inference_step_chunked(x, r, u, KAPPA)
        return r1, u1, th[:5]
    r1, _, th, _ = mixtures.gmm_inference_step_chunked(x, r)
    return r1, None, th


def _rel(a, b):
    """tests/test_mix_gpu.relerr without the log: max |a - b| / max |b|"""
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def converged_uncached(name, smm):
    """dict: x, r0 (fp32 arrays); rT, uT (fp32 arrays: the posterior after T_ITER (ITERATIONS) fp64 iterations, rounded); r1, u1 (fp64 tensors: one
    step from them); theta0 = the M-step of (rT, uT), theta1 = the M-step of (r1, u1) (what finalize gives after that step), fp64;
    e32: the fp32 oracle's error on r1 (absolute), u1 and the five tensors of theta0 / theta1 (relative), the larger of the two thetas;
    finite32: every fp32 output is finite"""
    x, r0 = data(name)
    N, K = r0.shape
    xo = torch.as_tensor(x).double()
    r, u = torch.as_tensor(r0).double(), (torch.ones(N, K, dtype=torch.float64) if smm else None)
    for _ in range(ITERATIONS.get((name, smm), T_ITER)):
        r, u, _ = _step(xo, r, u, smm)
    rT, uT = r.float(), (u.float() if smm else None)
    r1, u1, th0 = _step(xo, rT.double(), uT.double() if smm else None, smm)
    th1 = _step(xo, r1, u1, smm)[2]
    x32 = torch.as_tensor(x)
    s1, v1, t0 = _step(x32, rT, uT, smm)
    t1 = _step(x32, s1, v1, smm)[2]
    e32 = dict(r=float((s1.double() - r1).abs().max()))
    if smm:
        e32['u'] = _rel(v1, u1)
    for n_, a0, b0, a1, b1 in zip(NAMES, t0, th0, t1, th1):
        e32[n_] = max(_rel(a0, b0), _rel(a1, b1))
    fin = all(bool(torch.isfinite(t).all()) for t in [s1] + ([v1] if smm else []) + list(t0) + list(t1))
    return dict(x=x, r0=r0, rT=rT.numpy(), uT=uT.numpy() if smm else None, r1=r1, u1=u1, theta0=th0, theta1=th1, e32=e32, finite32=fin)


converged = functools.lru_cache(maxsize=None)(converged_uncached)      # computed once per case and flavour, shared, never modified


# The fp32 oracle's error is a property of the host that computes it as well as of the case (the order of torch's fp32 sums is the
# host's): on r of mom2_d8k16 smm it measured 5.2e-5 on one host and 8.4e-4 on another, with thread counts 1 .. 16 moving it by no
# more than a third on either.  The caps of
# tests/test_mix_hard_truth.py (r 1e-4, theta 1e-5) therefore bound the bars too: a host whose fp32 oracle is worse than the cap
# does not get a wider bar for the kernel.
CAP_R, CAP_THETA = 1e-4, 1e-5


def bar_r(tr):
    return max(1e-5, min(tr['e32']['r'], CAP_R))


def bar_theta(tr, name):
    return max(1e-5, 2.0 * min(tr['e32'][name], CAP_THETA))


# the kernel form each loop case is there for: (PassPlan::form, kt_mt) of vmp_mix_pass_plan for the fused pass; kt_mt of the XDL form
# is the number of bf16 terms per moment operand (3 below 65 536 rows, 2 from there on), of the tiled form the component tiles per lane
TILED, XDL = 1, 2
FORMS = {'xdl_d8k16': (XDL, 3), 'xdl_d2k3': (XDL, 3), 'auto_d4k5': (XDL, 3), 'mom2_d8k16': (XDL, 2),
         'tiled_d5k17': (TILED, 2), 'tiled_d3k33': (TILED, 4)}


def soft_rows(r):
    """number of rows with 0.01 <= max_k r <= 0.99"""
    top = torch.as_tensor(r).max(1).values
    return int(((top >= 0.01) & (top <= 0.99)).sum())


def condition_numbers(C):
    ev = torch.linalg.eigvalsh(torch.as_tensor(C).double())
    return ev[:, -1] / ev[:, 0]


def marginal_variances(theta):
    """per-column variance of the fitted mixture: sum_k pi_k (C_k / v_k + m_k m_k^T)_jj - mean_j^2, pi = alpha / sum alpha"""
    alpha, _, m, C, v = [torch.as_tensor(t).double() for t in theta]
    pi = alpha / alpha.sum()
    mean = (pi[:, None] * m).sum(0)
    second = (pi[:, None] * (torch.diagonal(C, dim1=-2, dim2=-1) / v[:, None] + m * m)).sum(0)
    return second - mean * mean


def theta32(name):
    """the converged Gaussian posterior (the M-step of rT), rounded to fp32: what the score / impute / bound surfaces are handed"""
    return tuple(t.float() for t in converged(name, False)['theta0'])


# ---- the other loops, from the same fp32-rounded posterior -------------------------------------------------------------------------
MISS_FRAC = 0.3


@functools.lru_cache(maxsize=None)
def mask(name, seed=11):
    """(N,D) uint8, about MISS_FRAC missing; row 0 fully missing, row 1 fully observed"""
    x, _ = data(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    miss = (rng.random(x.shape) < MISS_FRAC).astype(np.uint8)
    miss[0], miss[1] = 1, 0
    return miss


@functools.lru_cache(maxsize=None)
def masked(name=FIT_CASE):
    """(x with NaN in its missing slots, r_init = the converged rT, mask, mix_missfit_truth.bars after one iteration)"""
    import mix_missfit_truth as M
    x, _ = data(name)
    miss = mask(name)
    xm = x.copy()
    xm[miss != 0] = np.nan
    rT = converged(name, False)['rT']
    return xm, rT, miss, M.bars(xm, miss, rT, 1)


@functools.lru_cache(maxsize=None)
def weighted(name=FIT_CASE, seed=13):
    """(x, r_init = the converged rT, weights, mix_wfit_truth.bars after one iteration): integer counts 1..3, about a fifth zeros;
    every second row of weight 0 holds NaN throughout"""
    import mix_wfit_truth as W
    x, _ = data(name)
    w = W.make_weights(x.shape[0], seed, zeros=0.2, integer=True)
    xw = x.copy()
    gone = np.nonzero(w == 0)[0][::2]
    xw[gone] = np.nan
    rT = converged(name, False)['rT']
    return xw, rT, w, W.bars(xw, None, w, rT, 1)


# the weighted fit keeps shedding components up to its 40th iteration; the masked truth walks 256 mask patterns per iteration and
# stops two iterations after its collapse
BOUND_ITERATIONS = {'plain': 10, 'masked': 7, 'weighted': 40}


@functools.lru_cache(maxsize=None)
def free_inputs(kind, name=SURFACE_CASE):
    """(x, r0, miss or None, w or None) of the free-running loops"""
    import mix_wfit_truth as W
    x, r0 = data(name)
    miss = w = None
    if kind == 'masked':
        miss = mask(name)
        x = x.copy()
        x[miss != 0] = np.nan
    if kind == 'weighted':
        w = W.make_weights(x.shape[0], 13, integer=True)
    return x, r0, miss, w


@functools.lru_cache(maxsize=None)
def bound_sequence(kind, name=SURFACE_CASE):
    """the fp64 lower bound after each of the first BOUND_ITERATIONS iterations of the plain / masked / weighted fit from r0.  It is NOT
    monotone on these tables: the reference replaces log det P by 0 where det P <= 1e-20 (gmm.py:117-131), which every heavy component
    of a table with columns decades apart meets (det C ~ N_k^D prod_j var_j), so the iteration no longer ascends this bound - at
    (2049, 8, 16) it climbs from -2.4e4 to +6.2e3 in the iteration in which nine components empty and drops to -1.8e4 in the next.
    Returns (bounds, bars): the bar of each iteration is the bound tests' own, max(1e-5, 3 x the error of the same iteration run in
    fp32 from the same inputs), relative to max(1, |bound|) (mix_bound_truth.sequence; the weighted fit: mix_wfit_truth in both dtypes)."""
    import mix_bound_truth as B
    import mix_missfit_truth as M
    import mix_wfit_truth as W
    x, r0, miss, w = free_inputs(kind, name)
    n = BOUND_ITERATIONS[kind]
    if w is None:
        seq = B.sequence(x, miss, r0, n)
        return [q['bound'] for q in seq], [q['bar'] for q in seq]
    K, D = r0.shape[1], x.shape[1]
    prior = M.default_prior(K, D)
    m = np.zeros(x.shape, np.uint8)
    out, bars = [], []
    st64, st32 = W.seed_stats(x, m, w, r0), W.seed_stats(x, m, w, r0, torch.float32)
    for _ in range(n):
        it64, it32 = W.one_iteration(x, m, w, st64, prior), W.one_iteration(x, m, w, st32, prior, torch.float32)
        st64, st32 = it64['stats'], it32['stats']
        b64, b32 = it64['data'] - W.kl_terms(it64['theta'], prior), it32['data'] - W.kl_terms(it32['theta'], prior)
        out.append(b64)
        bars.append(B.bar_of(B.rel(b32, b64)))
    return out, bars


# name -> (N, D, K, spread, seed) of the diagonal fit, `spread` tuned for soft rows: centres closer than about 0.8 make the fit
# collapse to one component, centres 3 apart leave every row one-hot.  At D = 17, spread 1 keeps 17 % of the rows soft through all
# T_ITER iterations (two of the five components empty).  At D = 64 no spread does (2.0: 8 soft rows after 40 iterations, 3.0: none
# from the 4th on), so that case stops at DIAG_ITERATIONS, as the D = 8 Gaussian cases do: 74 soft rows, 11 of 16 components empty.
DIAG_CASES = {'diag_d64k16': (1031, 64, 16, 2.0, 21), 'diag_d17k5': (1031, 17, 5, 1.0, 22)}
DIAG_ITERATIONS = {'diag_d64k16': 6}
DIAG_DECADES = 3


def hard_diag(N, D, K, spread, seed):
    """(x, r0) fp32: centres spread * N(0, I), per-coordinate sd uniform in [0.5, 1.5] and a Dirichlet r0 (as mix_diag_truth.make_data),
    every column multiplied by a scale out of DIAG_DECADES decades (shuffled over the columns), and every fourth column almost
    constant: a level of the column's scale plus noise of 1e-3 of it"""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((K, D)) * spread
    sd = rng.uniform(0.5, 1.5, (K, D))
    z = rng.integers(0, K, N)
    x = c[z] + sd[z] * rng.standard_normal((N, D))
    r0 = rng.dirichlet(np.ones(K), N).astype(np.float32)
    scale = 10.0 ** (DIAG_DECADES * (rng.permutation(D) / max(D - 1, 1) - 0.5))
    flat = np.arange(D) % 4 == 3
    x[:, flat] = 1.0 + 1e-3 * rng.standard_normal((N, int(flat.sum())))
    return (x * scale).astype(np.float32), r0


@functools.lru_cache(maxsize=None)
def diag(name):
    """(x, r_init = r after T_ITER (DIAG_ITERATIONS) fp64 iterations of mix_diag_truth.iterate, rounded to fp32, prior,
    mix_diag_truth.bars after one iteration from it)"""
    import mix_diag_truth as G
    x, r0 = hard_diag(*DIAG_CASES[name])
    K = r0.shape[1]
    prior = G.default_prior(x, K)
    rT = G.iterate(x, r0, prior, DIAG_ITERATIONS.get(name, T_ITER))['r'].float().numpy()
    return x, rT, prior, G.bars(x, rT, prior, 1)
