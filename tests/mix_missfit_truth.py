"""fp64 truth of the Gaussian-mixture fit on partly observed rows (include/vmp_hip.h "Mixture fitting on partly observed rows") for
tests/test_mix_missfit_*.py, restated from the mathematics: for every row its observed / missing index sets are taken apart
explicitly, the missing block of the expected precision is inverted with torch.linalg.inv and its determinant taken with
torch.linalg.slogdet (rows that share a pattern share the two calls - nothing else is shared).  Nothing here factors a masked D x D
matrix: this file is the independent check of that device of csrc/vmp_missfit.hip.

  expectations()  K-sized: Lbar = v C^-1, c = E log pi + 1/2 E log|Lambda| - D / (2 beta)   (always fp64, rounded once: the pack builder)
  e_step()        log rho, r, log r, xhat^(k), Cov^(k), x_fill
  moments()       [Nk | Wk | sx | sxx] of the completed rows
  m_step()        the NIW update of oracle/mixtures.gmm_m_step, from raw moments            (always fp64, rounded once: vmp_mix_finalize)
  seed_stats()    moments of r_init on the column-mean-filled copy of x, no covariance term
  iterate()       seed, then `iterations` x (m_step, e_step, moments)
  lower_bound()   sum_n logsumexp_k log rho_nk - KL(q(pi) || p) - sum_k KL(q(mu, Lambda)_k || p), fp64
  bars()          truth, the error of the fp32 restatement and bar = max(1e-5, 3 x that error) per quantity

dtype = torch.float32 is the op-for-op restatement of the N-sized arithmetic in fp32: every operand rounded once, the same
operations on the same sub-matrices, the moment products formed on xhat - m_k (the shift of the kernel; x - column mean when seeding),
added in fp32 over blocks of 128 rows and in fp64 over the blocks, un-shifted in fp64 (seeding: as vmp_mix_stats does it, see
seed_stats).  The fp64 truth adds the plain products."""
import math

import numpy as np
import torch

from mix_score_truth import abs_err, rel_err  # noqa: F401  (re-exported for the tests)

LOG_2PI = math.log(2.0 * math.pi)
FLUSH_ROWS = 128
SMALL_STATS_MAX_N = 512        # csrc/vmp_common.h: up to this many rows vmp_mix_stats sums directly in fp64


def default_prior(K, D):
    """the prior gmm.inference hard-codes (reference gmm.py:252-256), standard form, fp64"""
    f = dict(dtype=torch.float64)
    return (torch.full((K,), 0.05 / K, **f), torch.full((K,), 0.5, **f), torch.zeros(K, D, **f),
            (D + 0.5) * torch.eye(D, **f).expand(K, D, D).contiguous(), torch.full((K,), 2 * D + 0.5, **f))


def _f64(ts):
    return [torch.as_tensor(t).detach().double().cpu() for t in ts]


def expectations(theta):
    """(m, Lbar = v C^-1, c, E log pi, E log|Lambda|) in fp64; E log|Lambda| as gmm.compute_expct_log_det_prec: digamma arguments
    (v + 1 + i) / 2 and log det P replaced by 0 where det P <= 1e-20"""
    alpha, beta, m, C, v = _f64(theta)
    D = m.shape[1]
    P = torch.linalg.inv(0.5 * (C + C.transpose(-1, -2)))
    P = 0.5 * (P + P.transpose(-1, -2))
    sign, lad = torch.linalg.slogdet(P)
    ld = torch.where((sign > 0) & (lad > math.log(1e-20)), lad, torch.zeros_like(lad))
    i = torch.arange(D, dtype=torch.float64)
    eld = torch.special.digamma(0.5 * (v[:, None] + 1.0 + i[None, :])).sum(1) + D * math.log(2.0) + ld
    elp = torch.special.digamma(alpha) - torch.special.digamma(alpha.sum())
    return m, v[:, None, None] * P, elp + 0.5 * eld - 0.5 * D / beta, elp, eld


def patterns(miss):
    """[(observed indices, missing indices, row indices)] of the distinct rows of the mask"""
    miss = np.asarray(miss) != 0
    D = miss.shape[1]
    code = (miss * (1 << np.arange(D))).sum(1)
    out = []
    for c in np.unique(code):
        rows = np.nonzero(code == c)[0]
        gone = miss[rows[0]]
        out.append((np.nonzero(~gone)[0], np.nonzero(gone)[0], rows))
    return out


def e_step(x, miss, theta, dtype=torch.float64, with_const=False):
    """dict(log_rho (N,K), r, logr, xhat (N,K,D), cov (N,K,D,D), x_fill (N,D)) in `dtype`.  with_const adds -D_o/2 log 2 pi to
    log rho (the lower bound needs it; r does not)."""
    m, Lbar, c, _, _ = (t.to(dtype) for t in expectations(theta))
    x = torch.as_tensor(x).to(dtype)
    N, D = x.shape
    K = m.shape[0]
    log_rho = torch.empty(N, K, dtype=dtype)
    xhat = torch.empty(N, K, D, dtype=dtype)
    cov = torch.zeros(N, K, D, D, dtype=dtype)
    for o, g, rows in patterns(miss):
        o, g, rows = torch.as_tensor(o), torch.as_tensor(g), torch.as_tensor(rows)
        xo = x[rows][:, o]                                                   # (n, D_o): the missing slots of x are never read
        d = xo[:, None, :] - m[None, :, o]                                   # (n, K, D_o)
        Loo = Lbar[:, o][:, :, o]
        q = torch.einsum('nki,kij,nkj->nk', d, Loo, d)
        xh = torch.empty(len(rows), K, D, dtype=dtype)
        xh[:, :, o] = xo[:, None, :].expand(len(rows), K, len(o))
        half_logdet = torch.zeros(K, dtype=dtype)
        if len(g):
            Lmm, Lmo = Lbar[:, g][:, :, g], Lbar[:, g][:, :, o]
            Sig = torch.linalg.inv(Lmm)                                      # Cov^(k) = Lbar_mm^-1
            t = torch.einsum('kij,nkj->nki', Lmo, d)
            St = torch.einsum('kij,nkj->nki', Sig, t)
            q = q - (t * St).sum(-1)                                         # d_o^T Lbar_oo d_o - t^T Lbar_mm^-1 t
            xh[:, :, g] = m[None, :, g] - St
            half_logdet = 0.5 * torch.linalg.slogdet(Lmm)[1]                 # sum_i log R_ii
            blk = torch.zeros(K, D, D, dtype=dtype)
            blk[:, g[:, None], g[None, :]] = Sig
            cov[rows] = blk
        lr = c[None, :] - 0.5 * q - half_logdet[None, :]
        if with_const:
            lr = lr - 0.5 * len(o) * LOG_2PI
        log_rho[rows] = lr
        xhat[rows] = xh
    lse = torch.logsumexp(log_rho, dim=1, keepdim=True)
    logr = log_rho - lse
    r = torch.exp(logr)
    gone = torch.as_tensor(np.asarray(miss) != 0)
    x_fill = torch.where(gone, torch.einsum('nk,nkd->nd', r, xhat), x)
    return dict(log_rho=log_rho, r=r, logr=logr, xhat=xhat, cov=cov, x_fill=x_fill, lse=lse[:, 0])


def _block_sum(t, dtype):
    """sum over the rows: plain in fp64; fp32: in fp32 over blocks of FLUSH_ROWS rows, in fp64 over the blocks"""
    if dtype == torch.float64:
        return t.sum(0)
    return torch.stack([t[i:i + FLUSH_ROWS].sum(0).double() for i in range(0, t.shape[0], FLUSH_ROWS)]).sum(0)


def moments(r, xhat, cov, shift, dtype=torch.float64):
    """(K, 2 + D + D*D) fp64 raw moments [Nk | Wk | sum r xhat | sum r (xhat xhat^T + cov)]; xhat (N,K,D) or (N,1,D), cov (N,K,D,D) or
    None, shift (K,D) or (1,D): what the fp32 restatement subtracts before the products are formed"""
    K = r.shape[1]
    D = xhat.shape[2]
    if dtype == torch.float64:
        dh = xhat.expand(-1, K, -1)
        sh = torch.zeros(K, D, dtype=torch.float64)
    else:
        sh = shift.to(dtype).expand(K, D)
        dh = xhat - sh[None]
    Nk = _block_sum(r, dtype).double()
    s1 = _block_sum(r[:, :, None] * dh, dtype).double()
    second = dh[:, :, :, None] * dh[:, :, None, :]
    if cov is not None:
        second = second + cov
    s2 = _block_sum(r[:, :, None, None] * second, dtype).double()
    sh = sh.double()
    sx = s1 + Nk[:, None] * sh
    sxx = s2 + s1[:, :, None] * sh[:, None, :] + sh[:, :, None] * s1[:, None, :] + Nk[:, None, None] * sh[:, :, None] * sh[:, None, :]
    return torch.cat([Nk[:, None], Nk[:, None], sx, sxx.reshape(K, D * D)], dim=1)


def m_step(stats, prior, dtype=torch.float64):
    """NIW posterior (alpha, beta, m, C, v), fp64 arithmetic, rounded to `dtype` once (vmp_mix_finalize); Bishop 10.58-10.63 with the
    reference's v_k = v_0 + N_k + 1 (gmm.py:81)"""
    a0, b0, m0, C0, v0 = _f64(prior)
    stats = torch.as_tensor(stats).double()
    K = stats.shape[0]
    D = m0.shape[1]
    Nk, sx, sxx = stats[:, 0], stats[:, 2:2 + D], stats[:, 2 + D:].reshape(K, D, D)
    xbar = sx / Nk[:, None]
    xbar = torch.where(torch.isnan(xbar), sx, xbar)
    S = sxx / Nk[:, None, None] - xbar[:, :, None] * xbar[:, None, :]
    S = torch.where(torch.isnan(S), sxx, S)
    alpha, beta = a0 + Nk, b0 + Nk
    m = (b0[:, None] * m0 + Nk[:, None] * xbar) / beta[:, None]
    e = xbar - m0
    C = C0 + Nk[:, None, None] * S + (b0 * Nk / beta)[:, None, None] * e[:, :, None] * e[:, None, :]
    v = v0 + Nk + 1.0
    return tuple(t.to(dtype) for t in (alpha, beta, m, C, v))


def mean_filled(x, miss, dtype=torch.float64):
    """x with its missing entries replaced by the column's mean over the observed entries (0 for a column with none)"""
    x = torch.as_tensor(x).double()
    gone = torch.as_tensor(np.asarray(miss) != 0)
    xz = torch.where(gone, torch.zeros((), dtype=torch.float64), x)
    mean = xz.sum(0) / (~gone).sum(0).clamp_min(1)
    return torch.where(gone, mean.to(torch.as_tensor(x).dtype)[None, :], x), mean


def seed_stats(x, miss, r_init, dtype=torch.float64):
    """moments of r_init on the mean-filled copy of x - no covariance term.  The fp32 restatement follows vmp_mix_stats, which the
    loop seeds with: up to SMALL_STATS_MAX_N rows it adds the plain products of the fp32 operands in fp64 (its small-batch kernel);
    beyond, the products are formed in fp32 on x - pivot (here: the column mean) and added as in moments()"""
    x32 = torch.as_tensor(x)
    xs, mean = mean_filled(x, miss)
    if dtype != torch.float64:
        xs = torch.where(torch.as_tensor(np.asarray(miss) != 0), mean.to(dtype)[None, :], x32.to(dtype))
        if xs.shape[0] <= SMALL_STATS_MAX_N:
            return moments(torch.as_tensor(r_init).to(dtype).double(), xs.double()[:, None, :], None, None, torch.float64)
    r = torch.as_tensor(r_init).to(dtype)
    return moments(r, xs.to(dtype)[:, None, :], None, mean[None, :], dtype)


def one_iteration(x, miss, stats, prior, dtype=torch.float64):
    """M-step from `stats`, E-step, moments of the completed rows: dict(theta, r, logr, x_fill, stats)"""
    theta = m_step(stats, prior, dtype)
    e = e_step(x, miss, theta, dtype)
    st = moments(e['r'], e['xhat'], e['cov'], torch.as_tensor(theta[2]).double(), dtype)
    return dict(theta=theta, r=e['r'], logr=e['logr'], x_fill=e['x_fill'], stats=st)


def iterate(x, miss, r_init, iterations, prior=None, dtype=torch.float64):
    """the state after `iterations` iterations from r_init (the last one_iteration's dict)"""
    K, D = torch.as_tensor(r_init).shape[1], torch.as_tensor(x).shape[1]
    prior = default_prior(K, D) if prior is None else prior
    out = dict(stats=seed_stats(x, miss, r_init, dtype))
    for _ in range(iterations):
        out = one_iteration(x, miss, out['stats'], prior, dtype)
    return out


def _log_B(W_logdet, nu, D):
    i = torch.arange(1, D + 1, dtype=torch.float64)
    return (-0.5 * nu * W_logdet - 0.5 * nu * D * math.log(2.0) - 0.25 * D * (D - 1) * math.log(math.pi)
            - torch.lgamma(0.5 * (nu[:, None] + 1.0 - i[None, :])).sum(1))


def lower_bound(x, miss, theta, prior=None):
    """sum_n logsumexp_k log rho_nk (with the -D_o/2 log 2 pi term) - KL(q(pi) || p(pi)) - sum_k KL(q(mu, Lambda)_k || p(mu, Lambda)),
    fp64: the free energy after the E-step at `theta`.  q(pi) = Dir(alpha), q(mu, Lambda)_k = N(mu | m, (beta Lambda)^-1) W(Lambda | C^-1, v)
    - (v, C^-1) read as the Wishart pair, as gmm.py:84-94 reads it - and the two expectations that enter the E-step, E[Lambda] = v C^-1
    and E log|Lambda| of expectations(), are the ones used throughout."""
    alpha, beta, m, C, v = _f64(theta)
    K, D = m.shape
    a0, b0, m0, C0, v0 = _f64(default_prior(K, D) if prior is None else prior)
    e = e_step(x, miss, theta, torch.float64, with_const=True)
    _, Lbar, _, elp, eld = expectations(theta)
    dg = torch.special.digamma
    kl_pi = (torch.lgamma(alpha.sum()) - torch.lgamma(alpha).sum() - torch.lgamma(a0.sum()) + torch.lgamma(a0).sum()
             + ((alpha - a0) * elp).sum())
    ld_W, ld_W0 = -torch.linalg.slogdet(C)[1], -torch.linalg.slogdet(C0)[1]
    dm = m - m0
    E_q_mu = 0.5 * eld + 0.5 * D * torch.log(beta / (2 * math.pi)) - 0.5 * D
    E_p_mu = (0.5 * eld + 0.5 * D * torch.log(b0 / (2 * math.pi)) - 0.5 * D * b0 / beta
              - 0.5 * b0 * torch.einsum('kd,kde,ke->k', dm, Lbar, dm))
    E_q_L = _log_B(ld_W, v, D) + 0.5 * (v - D - 1) * eld - 0.5 * v * D
    E_p_L = _log_B(ld_W0, v0, D) + 0.5 * (v0 - D - 1) * eld - 0.5 * torch.einsum('kde,ked->k', C0, Lbar)
    kl_nw = (E_q_mu - E_p_mu) + (E_q_L - E_p_L)
    return (e['lse'].sum() - kl_pi - kl_nw.sum()).item()


def bars(x, miss, r_init, iterations, prior=None):
    """dict of the fp64 truth after `iterations` iterations (r, logr, x_fill, stats, theta), the errors e_* of the fp32 restatement run
    from the same inputs, and bar_* = max(1e-5, 3 x e_*): absolute for r, relative to max(1, |value|) for logr, x_fill, the moments
    and the five tensors of theta (one bar for each)"""
    t64 = iterate(x, miss, r_init, iterations, prior, torch.float64)
    t32 = iterate(x, miss, r_init, iterations, prior, torch.float32)
    out = dict(t64)
    errs = dict(r=abs_err(t32['r'], t64['r']), logr=rel_err(t32['logr'], t64['logr']), x_fill=rel_err(t32['x_fill'], t64['x_fill']),
                stats=rel_err(t32['stats'], t64['stats']))
    for name, a, b in zip(('alpha', 'beta', 'm', 'C', 'v'), t32['theta'], t64['theta']):
        errs[name] = rel_err(a, b)
    for k, e in errs.items():
        out['e_' + k] = e
        out['bar_' + k] = max(1e-5, 3 * e)
    return out


def make_data(N, D, K, seed, frac=0.25):
    """seeded clusters, r_init ~ normalised exp(normal), and a mask with about `frac` missing whose row 0 is fully missing and row 1
    fully observed (N >= 2); the missing slots of x hold NaN"""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((K, D)) * 4.0
    x = (c[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)
    r0 = np.exp(rng.standard_normal((N, K)))
    r0 = (r0 / r0.sum(1, keepdims=True)).astype(np.float32)
    miss = (rng.random((N, D)) < frac).astype(np.uint8)
    miss[0] = 1
    if N > 1:
        miss[1] = 0
    x[miss != 0] = np.nan
    return x, r0, miss
