"""fp64 truth of the diagonal-covariance Gaussian mixture fit (include/vmp_hip.h "Diagonal-covariance mixture fitting on wide rows") for
tests/test_mix_diag_*.py, in torch (torch.special.digamma, torch.lgamma).

  make_data()     centres N(0, 3^2), per-coordinate sd uniform in [0.5, 1.5], a Dirichlet r0, x rounded to fp32
  default_prior() alpha_0 = 0.05 / K, beta_0 = 0.5, m_0 = column means (rounded to fp32, as the product hands them to the kernels),
                  a_0 = 1, b_0 = 1
  moments()       two-pass centred moments, as oracle/mixtures.py forms them: Nk, xbar, NS = sum_n r_nk (x_n - xbar_k)^2
  m_step(), e_step(), kl_terms(), iterate()
  log_marginal()  closed-form log marginal likelihood of D independent Normal-Gamma models (K = 1)
  bars()          truth, the error of the same functions run in fp32, and bar = max(1e-5, 3 x that error) per quantity

dtype = torch.float32 runs every function in fp32 from the fp32 inputs; only the sum of the rows' log-sum-exp is taken in fp64, as
the kernel takes it."""
import math

import numpy as np
import torch

LOG_2PI = math.log(2.0 * math.pi)
NAMES = ('alpha', 'beta', 'm', 'a', 'b')
SHAPES = [(300, 1, 2), (257, 17, 3), (513, 64, 16), (65, 5, 64), (1031, 33, 33)]     # the last one also with offset +1000


def make_data(N, D, K, seed, offset=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((K, D)) * 3.0
    sd = rng.uniform(0.5, 1.5, (K, D))
    z = rng.integers(0, K, N)
    x = (c[z] + sd[z] * rng.standard_normal((N, D)) + offset).astype(np.float32)
    r0 = rng.dirichlet(np.ones(K), N).astype(np.float32)
    return x, r0


def default_prior(x, K):
    x = np.asarray(x)
    D = x.shape[1]
    mean = x.astype(np.float64).mean(0).astype(np.float32)
    return (np.full(K, 0.05 / K, np.float32), np.full(K, 0.5, np.float32), np.tile(mean[None, :], (K, 1)),
            np.ones(K, np.float32), np.ones((K, D), np.float32))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def moments(x, r, dtype):
    x, r = _t(x, dtype), _t(r, dtype)
    Nk = r.sum(0)
    some = Nk > 0
    xbar = torch.where(some[:, None], (r.t() @ x) / Nk.clamp_min(1e-300 if dtype == torch.float64 else 1e-30)[:, None], torch.zeros((), dtype=dtype))
    dev = x[:, None, :] - xbar[None, :, :]
    NS = (r[:, :, None] * dev * dev).sum(0)
    return Nk, xbar, NS


def raw_stats(Nk, xbar, NS):
    """(K, 1 + 2 D) fp64 [Nk | sx | sxx] from the centred moments"""
    Nk, xbar, NS = Nk.double(), xbar.double(), NS.double()
    return torch.cat([Nk[:, None], Nk[:, None] * xbar, NS + Nk[:, None] * xbar * xbar], 1)


def m_step(Nk, xbar, NS, prior, dtype):
    a0, b0, m0, g0, h0 = [_t(p, dtype) for p in prior]            # alpha_0, beta_0, m_0, a_0, b_0
    alpha, beta, a = a0 + Nk, b0 + Nk, g0 + Nk / 2
    m = (b0[:, None] * m0 + Nk[:, None] * xbar) / beta[:, None]
    b = h0 + 0.5 * (NS + (b0 * Nk / beta)[:, None] * (xbar - m0) ** 2)
    return alpha, beta, m, a, b


def e_step(x, theta, dtype):
    alpha, beta, m, a, b = [t.to(dtype) for t in theta]
    x = _t(x, dtype)
    D = x.shape[1]
    dg = torch.special.digamma
    c = dg(alpha) - dg(alpha.sum()) + 0.5 * (dg(a)[:, None] - torch.log(b)).sum(1) - D / (2 * beta)
    lbar = a[:, None] / b
    dev = x[:, None, :] - m[None, :, :]
    logrho = c[None, :] - 0.5 * (lbar[None, :, :] * dev * dev).sum(2)
    lse = torch.logsumexp(logrho, 1)
    logr = logrho - lse[:, None]
    data = lse.double().sum().item() - 0.5 * x.shape[0] * D * LOG_2PI
    return torch.exp(logr), logr, data


def kl_terms(theta, prior):
    """(kl_pi, kl_ng (K,D)) in fp64"""
    alpha, beta, m, a, b = [torch.as_tensor(t).double() for t in theta]
    a0, b0, m0, g0, h0 = [_t(p, torch.float64) for p in prior]
    dg, lg = torch.special.digamma, torch.lgamma
    kl_pi = (lg(alpha.sum()) - lg(alpha).sum() - lg(a0.sum()) + lg(a0).sum() + ((alpha - a0) * (dg(alpha) - dg(alpha.sum()))).sum()).item()
    lbar = a[:, None] / b
    kl_ng = ((0.5 * torch.log(beta / b0) - 0.5 + 0.5 * b0 / beta)[:, None] + 0.5 * b0[:, None] * lbar * (m - m0) ** 2
             + ((a - g0) * dg(a) - lg(a) + lg(g0))[:, None] + g0[:, None] * (torch.log(b) - torch.log(h0)) + a[:, None] * (h0 - b) / b)
    return kl_pi, kl_ng


def iterate(x, r0, prior, iterations, dtype=torch.float64):
    """the state after `iterations` iterations from r0: dict(r, logr, stats, theta, data, bound, bounds, kl_pi, kl_ng)"""
    r = _t(r0, dtype)
    bounds, out = [], None
    for _ in range(iterations):
        theta = m_step(*moments(x, r, dtype), prior, dtype)
        r, logr, data = e_step(x, theta, dtype)
        kl_pi, kl_ng = kl_terms(theta, prior)
        bounds.append(data - kl_pi - kl_ng.sum().item())
        out = dict(r=r, logr=logr, theta=theta, data=data, bound=bounds[-1], kl_pi=kl_pi, kl_ng=kl_ng)
    out['stats'] = raw_stats(*moments(x, r, dtype))
    out['bounds'] = bounds
    return out


def log_marginal(x, prior):
    """log p(x) of D independent Normal-Gamma models with the prior's component 0 (the K = 1 mixture), fp64"""
    _, b0, m0, g0, h0 = [_t(p, torch.float64) for p in prior]
    x = _t(x, torch.float64)
    N = x.shape[0]
    xbar = x.mean(0)
    NS = ((x - xbar) ** 2).sum(0)
    bN, aN = b0[0] + N, g0[0] + N / 2
    hN = h0[0] + 0.5 * (NS + b0[0] * N / bN * (xbar - m0[0]) ** 2)
    lg = torch.lgamma
    return (-0.5 * N * LOG_2PI + 0.5 * torch.log(b0[0] / bN) + g0[0] * torch.log(h0[0]) - aN * torch.log(hN) + lg(aN) - lg(g0[0])).sum().item()


def abs_err(a, b):
    return (torch.as_tensor(a).detach().double().cpu() - torch.as_tensor(b).double()).abs().max().item()


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double()
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()


def errors(got, truth):
    """errors of a state dict against the truth: absolute for r, relative to max(1, |value|) for everything else"""
    errs = {}
    if got.get('r') is not None:
        errs['r'] = abs_err(got['r'], truth['r'])
    for name in ('logr', 'stats'):
        if got.get(name) is not None:
            errs[name] = rel_err(got[name], truth[name])
    if got.get('theta') is not None:
        for name, a, b in zip(NAMES, got['theta'], truth['theta']):
            errs[name] = rel_err(a, b)
    for name in ('data', 'bound'):
        if got.get(name) is not None:
            errs[name] = rel_err(float(got[name]), float(truth[name]))
    return errs


def bars(x, r0, prior, iterations):
    """the fp64 truth after `iterations` iterations, the errors e_* of the same functions run in fp32 from the same inputs, and
    bar_* = max(1e-5, 3 x e_*)"""
    t64 = iterate(x, r0, prior, iterations, torch.float64)
    t32 = iterate(x, r0, prior, iterations, torch.float32)
    out = dict(t64)
    for k, e in errors(t32, t64).items():
        out['e_' + k] = e
        out['bar_' + k] = max(1e-5, 3 * e)
    return out
