"""fp64 truth of mixture scoring (include/vmp_hip.h "Mixture scoring") for tests/test_mix_score_*.py: the formulae restated in
numpy / torch-CPU - Cholesky, triangular inverse, lgamma, log-sum-exp - plus the op-for-op fp32 restatement of the streaming
arithmetic whose error against the truth sets the tolerance of the kernel (the 3 x ref32 clause of tests/test_fullsize_gpu.py)."""
import math

import numpy as np
import torch


def _factor(S):
    """S (K,D,D) fp64 -> W = chol(S)^-1 (lower), sum_i log L_ii"""
    S = torch.as_tensor(S, dtype=torch.float64)
    Lc = torch.linalg.cholesky(0.5 * (S + S.transpose(-1, -2)))
    eye = torch.eye(S.shape[-1], dtype=torch.float64).expand_as(S)
    W = torch.linalg.solve_triangular(Lc, eye, upper=False)
    return W, torch.log(torch.diagonal(Lc, dim1=-2, dim2=-1)).sum(-1)


def pack_t(log_w, mu, sigma, nu):
    """explicit Student-t mixture (reference student_t.py:31-37) -> (m, W, c, h, a), all fp64"""
    log_w, mu, nu = (torch.as_tensor(t, dtype=torch.float64) for t in (log_w, mu, nu))
    D = mu.shape[1]
    W, sl = _factor(sigma)
    h = 0.5 * (nu + D)
    c = log_w + torch.lgamma(h) - torch.lgamma(0.5 * nu) - 0.5 * D * torch.log(math.pi * nu) - sl
    return mu, W, c, h, 1.0 / nu


def pack_niw(alpha, beta, m, C, v):
    """posterior predictive of the variational GMM (Bishop, PRML 10.81-10.82; C the inverse scale) -> (m, W, c, h, a)"""
    alpha, beta, m, v = (torch.as_tensor(t, dtype=torch.float64) for t in (alpha, beta, m, v))
    D = m.shape[1]
    W, sl = _factor(C)
    nup = v + 1.0 - D
    a = beta / (1.0 + beta)
    h = 0.5 * (nup + D)
    c = (torch.log(alpha / alpha.sum()) + torch.lgamma(h) - torch.lgamma(0.5 * nup) - 0.5 * D * torch.log(math.pi * nup)
         + 0.5 * D * torch.log(nup * a) - sl)
    return m, W, c, h, a


def evaluate(x, pk, dtype=torch.float64):
    """(terms (N,K), logp (N,), resp (N,K)) in `dtype`: every operand rounded to it once, then u = x - m, y = W u, q = |y|^2,
    term = c - h log1p(a q), max-shifted log-sum-exp - the operations of the streaming kernel, in its order"""
    m, W, c, h, a = (t.to(dtype) for t in pk)
    x = torch.as_tensor(x).to(dtype)
    u = x[:, None, :] - m[None, :, :]                                   # N,K,D
    y = torch.einsum('kij,nkj->nki', W, u)
    q = (y * y).sum(-1)
    terms = c[None, :] - h[None, :] * torch.log1p(a[None, :] * q)
    logp = torch.logsumexp(terms, dim=1)
    resp = torch.exp(terms - logp[:, None])
    return terms, logp, resp


def rel_err(got, want):
    """max |got - want| / max(1, |want|) over finite `want`; positions where `want` is infinite must match exactly"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin])
    if not fin.any():
        return 0.0
    return ((got[fin] - want[fin]).abs() / want[fin].abs().clamp_min(1.0)).max().item()


def abs_err(got, want):
    return (torch.as_tensor(got).double().cpu() - torch.as_tensor(want).double().cpu()).abs().max().item()


def bars(x, pk):
    """(truth logp, truth resp, bar for logp (relative to max(1, |value|)), bar for resp (absolute)) with
    bar = max(1e-5, 3 x the error of the fp32 restatement on the same inputs); the fp32 errors are returned too"""
    _, lp, rs = evaluate(x, pk, torch.float64)
    _, lp32, rs32 = evaluate(x, pk, torch.float32)
    e_lp, e_rs = rel_err(lp32, lp), abs_err(rs32, rs)
    return lp, rs, max(1e-5, 3 * e_lp), max(1e-5, 3 * e_rs), e_lp, e_rs


# ---- seeded inputs: well-separated clusters plus 1 % uniform background rows ---------------------------------------
def make_case(N, D, K, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.standard_normal((K, D)) * 6.0
    A = rng.standard_normal((K, D, D)) / math.sqrt(D)
    sigma = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(D)
    z = rng.integers(0, K, N)
    x = centres[z] + np.einsum('nij,nj->ni', np.linalg.cholesky(sigma)[z], rng.standard_normal((N, D)))
    bg = rng.random(N) < 0.01
    x[bg] = rng.uniform(-30.0, 30.0, (int(bg.sum()), D))
    w = rng.random(K) + 0.1
    t = dict(log_w=np.log(w / w.sum()), mu=centres + 0.1 * rng.standard_normal((K, D)), sigma=sigma, nu=rng.uniform(2.0, 10.0, K))
    v = D + rng.uniform(1.0, 40.0, K)
    niw = dict(alpha=rng.uniform(0.5, 50.0, K), beta=rng.uniform(0.5, 30.0, K), m=t['mu'], C=sigma * v[:, None, None], v=v)
    f32 = lambda d: {k: np.asarray(a, np.float32) for k, a in d.items()}
    return x.astype(np.float32), f32(t), f32(niw)
