"""fp64 truth of the Gaussian-mixture fit on weighted rows (include/vmp_hip.h "Mixture fitting on weighted rows") for
tests/test_mix_wfit_*.py, built on mix_missfit_truth: its e_step as it is (a weight does not enter a row's own responsibilities), its
moments with r * w, the weighted data term of the lower bound, and the iteration.

  keep()          the rows that count: w > 0.  A row of weight 0 is REMOVED - what it holds is replaced by zeros before anything is
                  multiplied, so NaN in its observed slots reaches neither the moments nor the data term
  moments()       [Nk | Wk | sx | sxx] with every row counted w_n times
  data_term()     sum_n w_n (logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi)
  seed_stats()    moments of r_init * w on the copy of x whose missing entries hold the column's WEIGHTED mean over the observed
                  entries of the rows that count (with integer weights: the column mean of the replicated rows)
  iterate()       seed, then `iterations` x (m_step, e_step, moments, data term)
  kl_terms()      KL(q(pi) || p) + sum_k KL(q(mu, Lambda)_k || p), from mix_missfit_truth.lower_bound on one row
  lower_bound()   data_term - kl_terms
  bars()          truth, the error of the fp32 restatement and bar = max(1e-5, 3 x that error) per quantity

miss=None stands for complete rows (an all-zero mask).  dtype = torch.float32 is the restatement of mix_missfit_truth with w r formed
in fp32 before the moment products, the row's log-sum-exp in fp32 and the weighted row terms added in fp64, as the kernel does."""
import numpy as np
import torch

import mix_missfit_truth as T
from mix_missfit_truth import abs_err, rel_err  # noqa: F401  (re-exported for the tests)

WEIGHT_VALUES = (0.0, 0.25, 1.0, 3.0, 7.5)


def _mask(x, miss):
    return np.zeros(np.asarray(x).shape, np.uint8) if miss is None else (np.asarray(miss) != 0).astype(np.uint8)


def keep(w):
    return torch.as_tensor(np.asarray(w)) > 0


def moments(e, shift, w, dtype=torch.float64):
    """(K, 2 + D + D*D) fp64 weighted raw moments from an e_step dict `e`"""
    k = keep(w)
    wt = torch.as_tensor(np.asarray(w)).to(dtype)
    zero = torch.zeros((), dtype=dtype)
    rw = torch.where(k[:, None], e['r'] * wt[:, None], zero)
    xhat = torch.where(k[:, None, None], e['xhat'], zero)
    cov = torch.where(k[:, None, None, None], e['cov'], zero)
    return T.moments(rw, xhat, cov, shift, dtype)


def data_term(e, miss, w):
    """sum_n w_n (lse_n - 1/2 D_o(n) log 2 pi): the row's log-sum-exp in the dtype of `e`, the sum in fp64, rows of weight 0 dropped"""
    k = keep(w)
    n_obs = torch.as_tensor((np.asarray(miss) == 0).sum(1)).double()
    term = e['lse'].double() - 0.5 * T.LOG_2PI * n_obs
    return torch.where(k, torch.as_tensor(np.asarray(w)).double() * term, torch.zeros((), dtype=torch.float64)).sum().item()


def weighted_mean_filled(x, miss, w):
    """(x with its missing entries replaced by the column's weighted mean over the observed entries of the rows that count and its
    rows of weight 0 replaced by zeros, that mean), fp64"""
    x = torch.as_tensor(np.asarray(x)).double()
    k = keep(w)
    gone = torch.as_tensor(np.asarray(miss) != 0) | ~k[:, None]
    wd = torch.where(gone, torch.zeros((), dtype=torch.float64), torch.as_tensor(np.asarray(w)).double()[:, None].expand_as(x))
    num = (torch.where(gone, torch.zeros((), dtype=torch.float64), x) * wd).sum(0)
    den = wd.sum(0)
    mean = torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))
    out = torch.where(torch.as_tensor(np.asarray(miss) != 0), mean[None, :], x)
    return torch.where(k[:, None], out, torch.zeros((), dtype=torch.float64)), mean


def seed_stats(x, miss, w, r_init, dtype=torch.float64):
    """moments of r_init * w on the weighted-mean-filled copy of x, no covariance term; the fp32 restatement follows vmp_mix_stats as
    mix_missfit_truth.seed_stats does (up to SMALL_STATS_MAX_N rows: plain products of the fp32 operands, added in fp64)"""
    miss = _mask(x, miss)
    k = keep(w)
    xs, mean = weighted_mean_filled(x, miss, w)
    wt = torch.as_tensor(np.asarray(w)).to(dtype)
    rw = torch.where(k[:, None], torch.as_tensor(r_init).to(dtype) * wt[:, None], torch.zeros((), dtype=dtype))
    if dtype != torch.float64:
        xs = xs.to(dtype)                                     # the filled copy is an fp32 tensor on the device
        if xs.shape[0] <= T.SMALL_STATS_MAX_N:
            return T.moments(rw.double(), xs.double()[:, None, :], None, None, torch.float64)
    return T.moments(rw, xs.to(dtype)[:, None, :], None, mean[None, :], dtype)


def one_iteration(x, miss, w, stats, prior, dtype=torch.float64):
    """M-step from `stats`, E-step, weighted moments and data term: dict(theta, r, logr, x_fill, stats, data, lse)"""
    theta = T.m_step(stats, prior, dtype)
    e = T.e_step(x, miss, theta, dtype)
    st = moments(e, torch.as_tensor(theta[2]).double(), w, dtype)
    return dict(theta=theta, r=e['r'], logr=e['logr'], x_fill=e['x_fill'], stats=st, data=data_term(e, miss, w), lse=e['lse'])


def iterate(x, miss, w, r_init, iterations, prior=None, dtype=torch.float64):
    """the state after `iterations` iterations from r_init (the last one_iteration's dict)"""
    K, D = torch.as_tensor(r_init).shape[1], torch.as_tensor(x).shape[1]
    prior = T.default_prior(K, D) if prior is None else prior
    miss = _mask(x, miss)
    out = dict(stats=seed_stats(x, miss, w, r_init, dtype))
    for _ in range(iterations):
        out = one_iteration(x, miss, w, out['stats'], prior, dtype)
    return out


def kl_terms(theta, prior=None):
    """KL(q(pi) || p) + sum_k KL(q(mu, Lambda)_k || p): the data term of one all-observed row of zeros minus its lower bound"""
    D = torch.as_tensor(theta[2]).shape[1]
    x1, m1 = np.zeros((1, D), np.float32), np.zeros((1, D), np.uint8)
    e = T.e_step(x1, m1, theta, torch.float64, with_const=True)
    return e['lse'].sum().item() - T.lower_bound(x1, m1, theta, prior)


def lower_bound(x, miss, w, theta, prior=None):
    """weighted data term (E-step at `theta`) - KL terms, fp64"""
    miss = _mask(x, miss)
    e = T.e_step(x, miss, theta, torch.float64)
    return data_term(e, miss, w) - kl_terms(theta, prior)


def _rel(a, b):
    return abs(float(a) - float(b)) / max(1.0, abs(float(b)))


def finite_rows(truth):
    """the rows whose truth is finite: every row but those of weight 0 that hold NaN in an observed slot"""
    return torch.isfinite(truth['r']).all(1) & torch.isfinite(truth['x_fill']).all(1)


def errors(got, truth):
    """errors of a state dict `got` against the truth: absolute for r, relative to max(1, |value|) for everything else; r, logr and
    x_fill over the rows whose truth is finite"""
    ok = finite_rows(truth)
    errs = {}
    for name in ('r', 'logr', 'x_fill'):
        if got.get(name) is not None:
            g = torch.as_tensor(got[name]).detach().double().cpu()[ok]
            errs[name] = abs_err(g, truth[name][ok]) if name == 'r' else rel_err(g, truth[name][ok])
    if got.get('stats') is not None:
        errs['stats'] = rel_err(got['stats'], truth['stats'])
    if got.get('theta') is not None:
        for name, a, b in zip(('alpha', 'beta', 'm', 'C', 'v'), got['theta'], truth['theta']):
            errs[name] = rel_err(a, b)
    for name in ('data', 'bound'):
        if got.get(name) is not None:
            errs[name] = _rel(got[name], truth[name])
    return errs


def bars(x, miss, w, r_init, iterations, prior=None):
    """dict of the fp64 truth after `iterations` iterations (r, logr, x_fill, stats, theta, data, bound), the errors e_* of the fp32
    restatement run from the same inputs, and bar_* = max(1e-5, 3 x e_*)"""
    t64 = iterate(x, miss, w, r_init, iterations, prior, torch.float64)
    t32 = iterate(x, miss, w, r_init, iterations, prior, torch.float32)
    for t in (t64, t32):
        t['bound'] = t['data'] - kl_terms(t['theta'], prior)
    out = dict(t64)
    for k, e in errors(t32, t64).items():
        out['e_' + k] = e
        out['bar_' + k] = max(1e-5, 3 * e)
    return out


def make_weights(N, seed, zeros=0.2, integer=False):
    """seeded weights from WEIGHT_VALUES (integer=True: from {0, 1, 2, 3}) with about `zeros` of them 0; row 2 always has weight 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    vals = np.array((1.0, 2.0, 3.0) if integer else WEIGHT_VALUES[1:], np.float32)
    w = vals[rng.integers(0, len(vals), N)]
    w[rng.random(N) < zeros] = 0.0
    if N > 2:
        w[2] = 0.0
    if N > 1:
        w[1] = 1.0
    return w.astype(np.float32)


def make_data(N, D, K, seed, masked, integer=False):
    """(x, r0, miss or None, w): the rows of mix_missfit_truth.make_data (masked: ~25 % missing, row 0 fully missing, row 1 fully
    observed, NaN in the missing slots; otherwise complete rows and no mask) and make_weights; row 2 has weight 0 and x = NaN in an
    OBSERVED slot"""
    x, r0, miss = T.make_data(N, D, K, seed, frac=0.25 if masked else 0.0)
    if not masked:                  # make_data hides row 0 whatever `frac` is: complete rows get seeded values there
        gone = miss != 0
        x[gone] = np.random.Generator(np.random.PCG64(seed + 2)).standard_normal(int(gone.sum())).astype(np.float32)
        miss = None
    w = make_weights(N, seed + 1, integer=integer)
    if N > 2:
        if masked:
            miss[2, 0] = 0
        x[2, 0] = np.nan
    return x, r0, miss, w
