"""The fp64 truth of tests/mix_impute_truth.py against an independent route: for every distinct missing pattern of a case, Sigma_oo
and Sigma_mo Sigma_oo^-1 formed explicitly with numpy.linalg (no precision matrix, no masked Cholesky); the fully observed rows
against the scoring truth; the fully missing rows against the closed form; one known answer (scipy.stats.multivariate_t where it is
installed).  The 1e-10 below is a condition on two fp64 routes over well-conditioned matrices (make_case: eigenvalues of sigma
>= 0.5, condition numbers of a few tens), not a kernel tolerance."""
import math

import numpy as np
import torch

import mix_impute_truth as T
import mix_score_truth as S

N, D, K, SEED = 257, 5, 7, 11            # seed 11: the first one tried; the two routes agree to ~1e-13 on it


def _case():
    x, t, q = S.make_case(N, D, K, SEED)
    return x, T.make_mask(N, D, SEED + 1), t, q


def _direct(x, miss, log_w, mu, sigma, nu):
    """numpy, row by row: marginal Student-t of the observed block and the conditional location of the missing one"""
    x, log_w, mu, sigma, nu = (np.asarray(a, np.float64) for a in (x, log_w, mu, sigma, nu))
    n, d = x.shape
    k = mu.shape[0]
    terms, xh = np.zeros((n, k)), np.zeros((n, k, d))
    for r in range(n):
        o, m = np.flatnonzero(miss[r] == 0), np.flatnonzero(miss[r] != 0)
        do = len(o)
        for c in range(k):
            xh[r, c] = mu[c]
            if do == 0:
                terms[r, c] = log_w[c]
                continue
            Soo = sigma[c][np.ix_(o, o)]
            dlt = x[r, o] - mu[c, o]
            sol = np.linalg.solve(Soo, dlt)
            qq = dlt @ sol
            terms[r, c] = (log_w[c] + math.lgamma(0.5 * (nu[c] + do)) - math.lgamma(0.5 * nu[c]) - 0.5 * do * math.log(math.pi * nu[c])
                           - 0.5 * np.linalg.slogdet(Soo)[1] - 0.5 * (nu[c] + do) * math.log1p(qq / nu[c]))
            if len(m):
                xh[r, c, m] = mu[c, m] + sigma[c][np.ix_(m, o)] @ sol
    mx = terms.max(1, keepdims=True)
    logp = mx[:, 0] + np.log(np.exp(terms - mx).sum(1))
    resp = np.exp(terms - logp[:, None])
    x_out = np.where(miss != 0, np.einsum('nk,nkd->nd', resp, xh), x)
    return logp, resp, x_out


def _agree(got, want, tol=1e-10):
    lp, rs, xo = want
    _, glp, grs, gxo = got
    assert S.rel_err(glp, lp) <= tol, S.rel_err(glp, lp)
    assert S.abs_err(grs, rs) <= tol, S.abs_err(grs, rs)
    assert S.rel_err(gxo, xo) <= tol, S.rel_err(gxo, xo)


def test_the_mask_has_the_forced_rows_and_many_patterns():
    m = T.make_mask(N, D, SEED + 1)
    assert m[0].all() and not m[1].any() and m[2].tolist() == [1, 0, 0, 0, 0] and m[3].tolist() == [1, 1, 1, 1, 0]
    assert len({tuple(r) for r in m.tolist()}) >= 16
    assert 0.2 < m.mean() < 0.4
    assert T.make_mask(1, 3, 0).tolist() == [[1, 1, 1]] and T.make_mask(2, 1, 0).tolist() == [[1], [0]]


def test_truth_equals_the_explicit_conditional_for_every_pattern_explicit_parameters():
    x, miss, t, _ = _case()
    _agree(T.evaluate(x, miss, T.pack_t(**t)), _direct(x, miss, t['log_w'], t['mu'], t['sigma'], t['nu']))


def test_truth_equals_the_explicit_conditional_for_every_pattern_niw_posterior():
    x, miss, _, q = _case()
    al, be, m, C, v = (np.asarray(q[n], np.float64) for n in ('alpha', 'beta', 'm', 'C', 'v'))
    nup = v + 1.0 - D
    sigma = C * ((1.0 + be) / (be * nup))[:, None, None]
    _agree(T.evaluate(x, miss, T.pack_niw(**q)), _direct(x, miss, np.log(al / al.sum()), m, sigma, nup))


def test_fully_observed_rows_equal_the_scoring_truth():
    x, miss, t, q = _case()
    none = np.zeros_like(miss)
    for pk_i, pk_s in ((T.pack_t(**t), S.pack_t(**t)), (T.pack_niw(**q), S.pack_niw(**q))):
        _, lp, rs, xo = T.evaluate(x, none, pk_i)
        _, lps, rss = S.evaluate(x, pk_s)
        assert S.rel_err(lp, lps) <= 1e-10 and S.abs_err(rs, rss) <= 1e-10
        assert torch.equal(xo, torch.as_tensor(x).double())
        # and inside a mixed mask: the rows without a missing entry
        full = np.flatnonzero(miss.sum(1) == 0)
        assert len(full) >= 2
        _, lpm, rsm, xom = T.evaluate(x, miss, pk_i)
        assert S.rel_err(lpm[full], lps[full]) <= 1e-10 and S.abs_err(rsm[full], rss[full]) <= 1e-10


def test_fully_missing_rows_equal_the_closed_form():
    x, miss, t, _ = _case()
    x = x.copy()
    x[miss != 0] = np.nan                                     # a missing slot never enters arithmetic
    _, lp, rs, xo = T.evaluate(x, miss, T.pack_t(**t))
    assert torch.isfinite(lp).all() and torch.isfinite(rs).all() and torch.isfinite(xo).all()
    gone = np.flatnonzero(miss.sum(1) == D)
    assert 0 in gone
    lw, mu = torch.as_tensor(t['log_w']).double(), torch.as_tensor(t['mu']).double()
    w = torch.softmax(lw, 0)
    for r in gone:
        assert abs(lp[r].item() - torch.logsumexp(lw, 0).item()) <= 1e-12
        assert (rs[r] - w).abs().max().item() <= 1e-12
        assert (xo[r] - w @ mu).abs().max().item() <= 1e-10


def test_minus_inf_weights():
    x, miss, t, _ = _case()
    t = {k: a.copy() for k, a in t.items()}
    t['log_w'][2] = -np.inf
    _, lp, rs, xo = T.evaluate(x, miss, T.pack_t(**t))
    assert torch.isfinite(lp).all() and (rs[:, 2] == 0).all() and torch.isfinite(xo).all()
    t['log_w'][:] = -np.inf
    for dt in (torch.float64, torch.float32):
        _, lp, rs, xo = T.evaluate(x, miss, T.pack_t(**t), dt)
        assert (lp == -math.inf).all() and (rs == 0).all()
        assert (xo[torch.as_tensor(miss != 0)] == 0).all() and torch.equal(xo[torch.as_tensor(miss == 0)], torch.as_tensor(x).to(dt)[torch.as_tensor(miss == 0)])


def test_a_known_answer():
    """D = 2, one component, unit weight: observing x_0 = 1 under mu = 0, sigma = [[2, 1], [1, 3]], nu = 4 gives the univariate
    Student-t with scale 2 at 1 and the conditional location 1/2; checked against scipy as well where it is installed"""
    t = dict(log_w=np.zeros(1), mu=np.zeros((1, 2)), sigma=np.array([[[2.0, 1.0], [1.0, 3.0]]]), nu=np.array([4.0]))
    x = np.array([[1.0, 123.0], [1.0, -0.5]])
    miss = np.array([[0, 1], [0, 0]], np.uint8)
    _, lp, rs, xo = T.evaluate(x, miss, T.pack_t(**t))
    want = math.lgamma(2.5) - math.lgamma(2.0) - 0.5 * math.log(math.pi * 4.0) - 0.5 * math.log(2.0) - 2.5 * math.log1p(0.5 / 4.0)
    assert abs(lp[0].item() - want) <= 1e-13
    assert abs(xo[0, 1].item() - 0.5) <= 1e-13 and xo[0, 0].item() == 1.0
    assert rs.tolist() == [[1.0], [1.0]]
    try:
        from scipy.stats import multivariate_t
    except ImportError:
        return
    assert abs(lp[0].item() - multivariate_t(loc=[0.0], shape=[[2.0]], df=4.0).logpdf([1.0])) <= 1e-12
    assert abs(lp[1].item() - multivariate_t(loc=[0.0, 0.0], shape=t['sigma'][0], df=4.0).logpdf(x[1])) <= 1e-12
