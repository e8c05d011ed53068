"""fp64 truth of mixture imputation (include/vmp_hip.h "Mixture imputation") for tests/test_mix_impute_*.py: the formulae restated
in torch-CPU - precision, Cholesky of the missing block of the masked precision, the two triangular solves, log-sum-exp - written
index by index in the order of the streaming kernel (csrc/vmp_impute.hip), so that the same routine run in fp32 is the op-for-op
restatement whose error against the fp64 run sets the tolerance of the kernel (bars(), as tests/mix_score_truth.py).  Op for
op up to two things torch cannot express: the kernel contracts a * b + c into one fused multiply-add, and it adds the 16 lanes of
a row in the order of the DPP rotations, not left to right.
tests/test_mix_impute_truth.py checks the fp64 run against an independent route (Sigma_oo and Sigma_mo Sigma_oo^-1 formed
explicitly with numpy.linalg)."""
import math

import numpy as np
import torch

from mix_score_truth import abs_err, make_case, rel_err  # noqa: F401  (re-exported for the tests)


def _precision(S):
    """S (K,D,D) fp64 -> S^-1 (through the Cholesky factor, symmetric), log det S"""
    S = torch.as_tensor(S, dtype=torch.float64)
    Lc = torch.linalg.cholesky(0.5 * (S + S.transpose(-1, -2)))
    eye = torch.eye(S.shape[-1], dtype=torch.float64).expand_as(S)
    W = torch.linalg.solve_triangular(Lc, eye, upper=False)
    return W.transpose(-1, -2) @ W, 2.0 * torch.log(torch.diagonal(Lc, dim1=-2, dim2=-1)).sum(-1)


def _consts(nu, D):
    """G[k, j] = lgamma((nu + j)/2) - lgamma(nu/2) - j/2 log(pi nu), j = 0..D"""
    j = torch.arange(D + 1, dtype=torch.float64)[None, :]
    nu = nu[:, None]
    return torch.lgamma(0.5 * (nu + j)) - torch.lgamma(0.5 * nu) - 0.5 * j * torch.log(math.pi * nu)


def pack_t(log_w, mu, sigma, nu):
    """explicit Student-t mixture -> (mu, Lambda, log w, nu, log det Lambda, 1 / nu, G), all fp64"""
    log_w, mu, nu = (torch.as_tensor(t, dtype=torch.float64) for t in (log_w, mu, nu))
    P, ld = _precision(sigma)
    return mu, P, log_w, nu, -ld, 1.0 / nu, _consts(nu, mu.shape[1])


def pack_niw(alpha, beta, m, C, v):
    """posterior predictive of the NIW posterior: w = alpha / sum alpha, mu = m, nu' = v + 1 - D, Sigma = C (1 + beta) / (beta nu')"""
    alpha, beta, m, v = (torch.as_tensor(t, dtype=torch.float64) for t in (alpha, beta, m, v))
    D = m.shape[1]
    nup = v + 1.0 - D
    s = nup * beta / (1.0 + beta)
    P, ld = _precision(C)
    return m, P * s[:, None, None], torch.log(alpha / alpha.sum()), nup, D * torch.log(s) - ld, 1.0 / nup, _consts(nup, D)


def evaluate(x, miss, pk, dtype=torch.float64):
    """(terms (N,K), logp (N,), resp (N,K), x_out (N,D)) in `dtype`: every operand rounded to it once, then the operations of the
    streaming kernel in its order, one (N,K) tensor per register.  What x holds in a missing slot goes through torch.where only."""
    mu, P, lw, nu, ldet, inu, G = (t.to(dtype) for t in pk)
    x = torch.as_tensor(x).to(dtype)
    miss = torch.as_tensor(miss) != 0
    N, D = x.shape
    K = mu.shape[0]
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    mk = [miss[:, d][:, None].expand(N, K) for d in range(D)]
    n_obs = (~miss).sum(1)
    dt = [torch.where(mk[d], zero, x[:, d][:, None] - mu[None, :, d]) for d in range(D)]
    lam = lambda i, j: P[None, :, max(i, j), min(i, j)]
    v, qo = [], torch.zeros(N, K, dtype=dtype)
    for i in range(D):
        s = lam(i, 0) * dt[0]
        for j in range(1, D):
            s = s + lam(i, j) * dt[j]
        v.append(torch.where(mk[i], s, zero))
        qo = qo + dt[i] * s
    A = [[torch.where(mk[i] & mk[j], lam(i, j).expand(N, K), one if i == j else zero) for j in range(i + 1)] for i in range(D)]
    rd, piv = [], []
    for j in range(D):
        s = A[j][j]
        for q in range(j):
            s = s - A[j][q] * A[j][q]
        piv.append(s)
        rd.append(1.0 / torch.sqrt(s))
        for i in range(j + 1, D):
            t = A[i][j]
            for q in range(j):
                t = t - A[i][q] * A[j][q]
            A[i][j] = t * rd[j]
    slog = torch.zeros(N, K, dtype=dtype)
    for j in range(0, D - 1, 2):
        slog = slog + torch.log(piv[j] * piv[j + 1])
    if D % 2:
        slog = slog + torch.log(piv[D - 1])
    slog = 0.5 * slog
    yy = torch.zeros(N, K, dtype=dtype)
    for i in range(D):
        s = v[i]
        for q in range(i):
            s = s - A[i][q] * v[q]
        v[i] = s * rd[i]
        yy = yy + v[i] * v[i]
    for i in range(D - 1, -1, -1):
        s = v[i]
        for q in range(i + 1, D):
            s = s - A[q][i] * v[q]
        v[i] = s * rd[i]
    xh = [mu[None, :, d] - v[d] for d in range(D)]
    q = qo - yy
    q = torch.where(q < 0, zero, q)
    g = G.t()[n_obs]                                                    # (N,K)
    h = 0.5 * (nu[None, :] + n_obs[:, None].to(dtype))
    terms = (lw[None, :] + g) + (0.5 * ldet[None, :] - slog) - h * torch.log1p(q * inu[None, :])
    terms = torch.where((n_obs == 0)[:, None], lw[None, :].expand(N, K), terms)
    # the kernel's log-sum-exp: lane i16 walks its components k = i16 + 16 t with a lane-local online form (running maximum ml,
    # s = sum e, ax = sum e xhat, rescaled when the maximum moves), then the 16 lanes of a row are combined once
    KT = (K + 15) // 16
    pad = KT * 16 - K
    ninf = torch.full((N, pad), -math.inf, dtype=dtype)
    lt = torch.cat([terms, ninf], 1).reshape(N, KT, 16)
    xt = [torch.cat([xh[d].expand(N, K), torch.zeros(N, pad, dtype=dtype)], 1).reshape(N, KT, 16) for d in range(D)]
    ml = torch.full((N, 16), -math.inf, dtype=dtype)
    s = torch.zeros(N, 16, dtype=dtype)
    ax = [torch.zeros(N, 16, dtype=dtype) for _ in range(D)]
    for t in range(KT):
        l = lt[:, t]
        mn = torch.where(l > ml, l, ml)                                 # fmaxf: a NaN term leaves the maximum alone ...
        sh = torch.where(mn == -math.inf, zero, mn)
        c, e = torch.exp(ml - sh), torch.exp(l - sh)                    # ... and poisons the sum
        s = s * c + e
        for d in range(D):
            ax[d] = ax[d] * c + torch.where(e == 0, zero, e * xt[d][:, t])
        ml = mn
    mx = ml.max(1).values
    shift = torch.where(mx == -math.inf, zero, mx)
    f = torch.exp(ml - shift[:, None])
    S = (s * f).sum(1)
    inv = torch.where(S == 0, zero, 1.0 / S)
    logp = shift + torch.log(S)
    resp = torch.exp(terms - shift[:, None]) * inv[:, None]
    xs = torch.stack([(ax[d] * f).sum(1) * inv for d in range(D)], dim=1)
    x_out = torch.where(miss, xs, x)
    return terms, logp, resp, x_out


def bars(x, miss, pk):
    """dict with the fp64 truth (logp, resp, x_out), the errors of the fp32 restatement on the same inputs (e_*) and the bars
    bar_* = max(1e-5, 3 x e_*): relative to max(1, |value|) for logp and x_out, absolute for resp"""
    _, lp, rs, xo = evaluate(x, miss, pk, torch.float64)
    _, lp32, rs32, xo32 = evaluate(x, miss, pk, torch.float32)
    e_lp, e_rs, e_x = rel_err(lp32, lp), abs_err(rs32, rs), rel_err(xo32, xo)
    return dict(logp=lp, resp=rs, x_out=xo, e_logp=e_lp, e_resp=e_rs, e_x=e_x,
                bar_logp=max(1e-5, 3 * e_lp), bar_resp=max(1e-5, 3 * e_rs), bar_x=max(1e-5, 3 * e_x))


def make_mask(N, D, seed):
    """(N,D) uint8, 1 = missing: seeded Bernoulli(0.3) per entry; where N allows, row 0 all missing, row 1 all observed, row 2 only
    entry 0 missing, row 3 only entry D-1 observed"""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = (rng.random((N, D)) < 0.3).astype(np.uint8)
    forced = [np.ones(D, np.uint8), np.zeros(D, np.uint8), np.eye(D, dtype=np.uint8)[0], 1 - np.eye(D, dtype=np.uint8)[D - 1]]
    for i, row in enumerate(forced[:N]):
        m[i] = row
    return m
