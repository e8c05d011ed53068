"""fp64 truth of the diagonal-covariance mixture fit on partly observed and weighted rows (include/vmp_hip.h "Diagonal-covariance
mixture: fitting partly observed and weighted rows") for tests/test_mix_dmfit_*.py, in torch, built on mix_diag_truth (m_step, kl_terms,
raw_stats, the error helpers).

  make_case()       mix_diag_truth.make_data plus a mask (a fraction missing at random, one all-missing row, one all-missing column) and
                    integer weights 0..3 with at least one 0
  observed_means()  weighted column means over the observed entries of the rows of positive weight (0 for a column without one)
  default_prior()   mix_diag_truth.default_prior with those means
  start_moments()   the loop's start: the moments of r0 * w on x with every dead entry replaced by its column's observed mean
  e_step()          log rho over the observed entries plus hl over the missing ones; r, log r, the weighted data term
  completed_moments()  centred moments of the completed rows: q(x_nd | z = k) = N(m_kd, 1 / lbar_kd) for d missing
  iterate()         the state after `iterations` iterations: dict(r, logr, fill, stats, theta, xbar, S, pi, data, bound, bounds, ...)
  errors(), bars()  as in mix_diag_truth, with the fill: bar = max(1e-5, 3 x the error of the same functions run in fp32)

miss is a bool array (True = missing) or None; w a float array or None.  What a missing slot or a row of weight 0 holds is selected
out before any arithmetic.  dtype = torch.float32 runs every function in fp32 from the fp32 inputs; only the rows' data terms are
formed and added in fp64, as the kernel does."""
import numpy as np
import torch

import mix_diag_truth as T

LOG_2PI = T.LOG_2PI
SHAPES = [(300, 1, 2), (130, 9, 1), (257, 17, 3), (65, 5, 64), (4099, 16, 16), (1031, 33, 33), (513, 64, 16), (2051, 64, 64)]
MODES = ('mask', 'weights', 'both')


def make_case(N, D, K, seed, mode, offset=0.0, frac=0.3):
    """(x, r0, miss or None, w or None).  Mask: `frac` missing at random, row 1 (row 0 when N = 1) all missing, the last column all
    missing.  Weights: integers 0..3, w[0] = 0 and w[N-1] = 2."""
    x, r0 = T.make_data(N, D, K, seed, offset)
    rng = np.random.Generator(np.random.PCG64(seed + 9001))
    miss = w = None
    if mode in ('mask', 'both'):
        miss = rng.random((N, D)) < frac
        miss[min(1, N - 1), :] = True
        miss[:, D - 1] = True
    if mode in ('weights', 'both'):
        w = rng.integers(0, 4, N).astype(np.float32)
        w[0] = 0.0
        w[N - 1] = 2.0
    return x, r0, miss, w


def _live(x, miss, w):
    """(N,D) bool: observed entries of rows of positive weight"""
    x = np.asarray(x)
    live = np.ones(x.shape, bool) if miss is None else ~np.asarray(miss, bool)
    if w is not None:
        live = live & (np.asarray(w) > 0)[:, None]
    return live


def observed_means(x, miss, w):
    """(D,) fp64"""
    x = np.asarray(x)
    live = _live(x, miss, w)
    ww = np.ones(x.shape[0]) if w is None else np.asarray(w, np.float64)
    num = (np.where(live, x.astype(np.float64), 0.0) * ww[:, None]).sum(0)
    den = (live * ww[:, None]).sum(0)
    return np.where(den > 0, num / np.maximum(den, 1e-300), 0.0)


def default_prior(x, K, miss=None, w=None):
    x = np.asarray(x)
    D = x.shape[1]
    mean = observed_means(x, miss, w).astype(np.float32)
    return (np.full(K, 0.05 / K, np.float32), np.full(K, 0.5, np.float32), np.tile(mean[None, :], (K, 1)),
            np.ones(K, np.float32), np.ones((K, D), np.float32))


def start_moments(x, r0, miss, w, dtype):
    """(Nk, xbar, NS) of r0 * w on the mean-filled rows (the mean rounded to fp32, as the product hands it to the kernel)"""
    x = np.asarray(x)
    mean = observed_means(x, miss, w).astype(np.float32)
    xs = np.where(_live(x, miss, w), x, mean[None, :]).astype(np.float32)
    r = np.asarray(r0, np.float32) if w is None else (np.asarray(r0, np.float32) * np.asarray(w, np.float32)[:, None])
    return T.moments(xs, r, dtype)


def _masks(x, miss, w, dtype):
    x = np.asarray(x)
    N, D = x.shape
    mm = torch.zeros(N, D, dtype=torch.bool) if miss is None else torch.as_tensor(np.asarray(miss, bool))
    ww = torch.ones(N, dtype=dtype) if w is None else torch.as_tensor(np.asarray(w)).to(dtype)
    xz = torch.where(mm, torch.zeros((), dtype=dtype), torch.as_tensor(x).to(dtype))
    return xz, mm, ww


def e_step(x, miss, w, theta, dtype):
    """(r, logr, data): r and log r unweighted; data = sum_n w_n (lse_n - 1/2 D_o(n) log 2 pi) over the rows with w_n > 0, each
    row's term formed and added in fp64 from the lse of `dtype`"""
    alpha, beta, m, a, b = [t.to(dtype) for t in theta]
    xz, mm, ww = _masks(x, miss, w, dtype)
    D = xz.shape[1]
    dg = torch.special.digamma
    c = dg(alpha) - dg(alpha.sum()) + 0.5 * (dg(a)[:, None] - torch.log(b)).sum(1) - D / (2 * beta)
    lbar = a[:, None] / b
    hl = -0.5 * torch.log(lbar)
    dev = torch.where(mm[:, None, :], torch.zeros((), dtype=dtype), xz[:, None, :] - m[None, :, :])
    logrho = c[None, :] - 0.5 * (lbar[None, :, :] * dev * dev).sum(2) + (mm.to(dtype) @ hl.t())
    lse = torch.logsumexp(logrho, 1)
    logr = logrho - lse[:, None]
    dobs = (D - mm.sum(1)).double()
    term = ww.double() * (lse.double() - 0.5 * dobs * LOG_2PI)
    finite_rows = ww > 0
    data = torch.where(finite_rows, term, torch.zeros((), dtype=torch.float64)).sum().item()
    return torch.exp(logr), logr, data


def completed_moments(x, miss, w, r, theta, dtype):
    """(Nk, xbar, NS) of the completed rows under q(x_missing | z) at theta, every row counted w_n times; rows of weight 0 selected out"""
    _, _, m, a, b = [t.to(dtype) for t in theta]
    xz, mm, ww = _masks(x, miss, w, dtype)
    dead = ~(ww > 0)
    xz = torch.where(dead[:, None], torch.zeros((), dtype=dtype), xz)
    wr = torch.where(dead[:, None], torch.zeros((), dtype=dtype), r.to(dtype) * ww[:, None])
    lbar = a[:, None] / b
    Nk = wr.sum(0)
    some = Nk > 0
    safe = Nk.clamp_min(1e-300 if dtype == torch.float64 else 1e-30)
    xc = torch.where(mm[:, None, :], m[None, :, :], xz[:, None, :])                       # (N,K,D)
    xbar = torch.where(some[:, None], (wr[:, :, None] * xc).sum(0) / safe[:, None], torch.zeros((), dtype=dtype))
    dev = xc - xbar[None, :, :]
    var = torch.where(mm[:, None, :], (1.0 / lbar)[None, :, :], torch.zeros((), dtype=dtype))
    NS = (wr[:, :, None] * (dev * dev + var)).sum(0)
    return Nk, xbar, NS


def fill(x, miss, r, theta, dtype):
    _, _, m, _, _ = [t.to(dtype) for t in theta]
    xz, mm, _ = _masks(x, miss, None, dtype)
    return torch.where(mm, r.to(dtype) @ m, xz)


def iterate(x, r0, prior, iterations, miss=None, w=None, dtype=torch.float64):
    """the state after `iterations` iterations from r0: dict(r, logr, fill, stats, theta, xbar, S, pi, data, bound, bounds, kl_pi, kl_ng)"""
    mom = start_moments(x, r0, miss, w, dtype)
    bounds, out = [], None
    for _ in range(iterations):
        theta = T.m_step(*mom, prior, dtype)
        xbar, S, pi = T.aux(*mom, theta[0])
        r, logr, data = e_step(x, miss, w, theta, dtype)
        kl_pi, kl_ng = T.kl_terms(theta, prior)
        bounds.append(data - kl_pi - kl_ng.sum().item())
        mom = completed_moments(x, miss, w, r, theta, dtype)
        out = dict(r=r, logr=logr, theta=theta, xbar=xbar, S=S, pi=pi, data=data, bound=bounds[-1], kl_pi=kl_pi, kl_ng=kl_ng)
    out['stats'] = T.raw_stats(*mom)
    out['fill'] = fill(x, miss, out['r'], out['theta'], dtype) if miss is not None else None
    out['bounds'] = bounds
    return out


def errors(got, truth):
    """mix_diag_truth.errors plus the fill: absolute for r, relative to max(1, |value|) for everything else"""
    errs = T.errors(got, truth)
    if got.get('fill') is not None:
        errs['fill'] = T.rel_err(got['fill'], truth['fill'])
    return errs


def bars(x, r0, prior, iterations, miss=None, w=None):
    """the fp64 truth after `iterations` iterations, the errors e_* of the same functions run in fp32 from the same inputs, and
    bar_* = max(1e-5, 3 x e_*)"""
    t64 = iterate(x, r0, prior, iterations, miss, w, torch.float64)
    t32 = iterate(x, r0, prior, iterations, miss, w, torch.float32)
    out = dict(t64)
    for k, e in errors(t32, t64).items():
        out['e_' + k] = e
        out['bar_' + k] = max(1e-5, 3 * e)
    return out
