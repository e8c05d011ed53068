"""The fp64 truth of mixture sampling (tests/mix_sample_truth.py) checked on its own, on the CPU: its draws have the law they claim
(mixture moments, the conditional moments of a single component, the quartiles of a Student-t without moments - the a < 1 branch of
the gamma draw), the attempt cap is never exhausted, rows are a function of their absolute index, and over the shape sweep of
tests/test_mix_sample_gpu.py the constants TAU and BAR still follow from the fp32 restatement while the truth ALONE leaves at most 1 %
of any case undecidable - so the GPU test cannot hide a failure behind exclusions."""
import math

import numpy as np
import pytest

import mix_impute_truth as T
import mix_sample_truth as ST

N_LAW = 200000


def _t4(s2, nu):
    """variance and fourth central moment of a univariate Student-t with squared scale s2 and nu > 4 degrees of freedom"""
    return s2 * nu / (nu - 2), 3 * s2 ** 2 * nu ** 2 / ((nu - 2) * (nu - 4))


def test_unconditional_draws_have_the_mixture_moments():
    K, D, nu = 3, 3, 50.0
    rng = np.random.Generator(np.random.PCG64(11))
    mu = rng.standard_normal((K, D)) * 2
    Lc = np.tril(rng.standard_normal((K, D, D)) * 0.4) + np.eye(D)
    sigma = Lc @ Lc.transpose(0, 2, 1)
    w = np.array([0.5, 0.3, 0.2])
    tr = ST.draw(None, None, T.pack_t(np.log(w), mu, sigma, np.full(K, nu)), seed=0xC0FFEE, N=N_LAW)
    assert not tr['exhausted'].any() and tr['attempts'].max() < ST.ATTEMPTS
    x = tr['x'][0]
    mean = w @ mu
    cov = np.einsum('k,kij->ij', w, sigma * nu / (nu - 2) + mu[:, :, None] * mu[:, None, :]) - np.outer(mean, mean)
    # fourth central moment of every coordinate's marginal: sum_k w_k (delta^4 + 6 delta^2 var_k + m4_k)
    delta = mu - mean
    var_k, m4_k = _t4(np.diagonal(sigma, axis1=1, axis2=2), nu)
    m4 = (w[:, None] * (delta ** 4 + 6 * delta ** 2 * var_k + m4_k)).sum(0)
    se_mean = np.sqrt(np.diag(cov) / N_LAW)
    assert (np.abs(x.mean(0) - mean) <= 5 * se_mean).all(), (x.mean(0), mean, se_mean)
    # Var[(x_i - m_i)(x_j - m_j)] <= E[(x_i - m_i)^2 (x_j - m_j)^2] <= sqrt(m4_i m4_j)   (Cauchy-Schwarz): a bound on the standard error
    se_cov = np.sqrt(np.sqrt(np.outer(m4, m4)) / N_LAW)
    got = np.cov(x.T, bias=True)
    assert (np.abs(got - cov) <= 5 * se_cov).all(), (got, cov, se_cov)
    assert (np.abs(np.bincount(tr['z'][0], minlength=K) / N_LAW - w) <= 5 * np.sqrt(w * (1 - w) / N_LAW)).all()


def test_conditional_draws_have_the_conditional_moments_of_the_component():
    """K = 1, entries 0 and 2 observed (the same values in every row): x_1 | x_o is t_{nu+2}(xhat, (nu + q)/(nu + 2) Schur), with the
    conditional quantities formed explicitly from sigma with numpy.linalg"""
    D, nu = 3, 50.0
    rng = np.random.Generator(np.random.PCG64(12))
    mu = rng.standard_normal((1, D))
    Lc = np.tril(rng.standard_normal((D, D)) * 0.5) + np.eye(D)
    sigma = (Lc @ Lc.T)[None]
    xo = np.array([0.7, 0.0, -1.1])
    x = np.broadcast_to(xo.astype(np.float32), (N_LAW, D)).copy()
    miss = np.zeros((N_LAW, D), np.uint8)
    miss[:, 1] = 1
    tr = ST.draw(x, miss, T.pack_t(np.zeros(1), mu, sigma, np.full(1, nu)), seed=99)
    assert not tr['exhausted'].any() and tr['attempts'].max() < ST.ATTEMPTS
    assert (tr['x'][0][:, [0, 2]] == x[:, [0, 2]]).all()
    o, m = [0, 2], [1]
    S = sigma[0]
    d_o = x[0, o].astype(np.float64) - mu[0, o]
    Soo_inv = np.linalg.inv(S[np.ix_(o, o)])
    xhat = mu[0, 1] + (S[np.ix_(m, o)] @ Soo_inv @ d_o)[0]
    q = d_o @ Soo_inv @ d_o
    s2 = (nu + q) / (nu + 2) * (S[1, 1] - (S[np.ix_(m, o)] @ Soo_inv @ S[np.ix_(o, m)])[0, 0])
    var, m4 = _t4(s2, nu + 2)
    y = tr['x'][0][:, 1]
    assert abs(y.mean() - xhat) <= 5 * math.sqrt(var / N_LAW), (y.mean(), xhat)
    assert abs(y.var() - var) <= 5 * math.sqrt((m4 - var ** 2) / N_LAW), (y.var(), var)


def test_two_missing_coordinates_have_the_conditional_mean_and_covariance():
    """K = 1, D = 4, entries 1 and 3 missing under the same observed values in every row: (x_1, x_3) | x_o is
    t_{nu+2}(xhat, (nu + q)/(nu + 2) Schur) - the off-diagonal entry of the R^-T solve under a partial mask shows in the covariance"""
    D, nu = 4, 50.0
    rng = np.random.Generator(np.random.PCG64(13))
    mu = rng.standard_normal((1, D))
    Lc = np.tril(rng.standard_normal((D, D)) * 0.6) + np.eye(D)
    sigma = (Lc @ Lc.T)[None]
    x = np.broadcast_to(np.array([0.4, 0.0, -0.9, 0.0], np.float32), (N_LAW, D)).copy()
    miss = np.zeros((N_LAW, D), np.uint8)
    miss[:, [1, 3]] = 1
    tr = ST.draw(x, miss, T.pack_t(np.zeros(1), mu, sigma, np.full(1, nu)), seed=314)
    assert not tr['exhausted'].any() and (tr['x'][0][:, [0, 2]] == x[:, [0, 2]]).all()
    o, m = [0, 2], [1, 3]
    S = sigma[0]
    d_o = x[0, o].astype(np.float64) - mu[0, o]
    Soo_inv = np.linalg.inv(S[np.ix_(o, o)])
    xhat = mu[0, m] + S[np.ix_(m, o)] @ Soo_inv @ d_o
    q = d_o @ Soo_inv @ d_o
    scale = (nu + q) / (nu + 2) * (S[np.ix_(m, m)] - S[np.ix_(m, o)] @ Soo_inv @ S[np.ix_(o, m)])
    dof = nu + 2
    cov = scale * dof / (dof - 2)
    assert abs(cov[0, 1]) > 0.1 * math.sqrt(cov[0, 0] * cov[1, 1])          # the coupling is there to be seen
    y = tr['x'][0][:, m]
    assert (np.abs(y.mean(0) - xhat) <= 5 * np.sqrt(np.diag(cov) / N_LAW)).all(), (y.mean(0), xhat)
    # elliptical law: E[d_i d_j d_k d_l] = kappa (S_ij S_kl + S_ik S_jl + S_il S_jk), kappa = (dof - 2)/(dof - 4) on the covariance
    kap = (dof - 2) / (dof - 4)
    var_of = lambda i, j: kap * (cov[i, i] * cov[j, j] + 2 * cov[i, j] ** 2) - cov[i, j] ** 2
    got = np.cov(y.T, bias=True)
    for i, j in ((0, 0), (0, 1), (1, 1)):
        assert abs(got[i, j] - cov[i, j]) <= 5 * math.sqrt(var_of(i, j) / N_LAW), (i, j, got[i, j], cov[i, j])


def _t_cdf(q, nu, n=200001):
    """cdf of the standard Student-t at q > 0 by Simpson's rule on [0, q]"""
    t = np.linspace(0.0, q, n)
    f = np.exp(math.lgamma((nu + 1) / 2) - math.lgamma(nu / 2) - 0.5 * math.log(nu * math.pi)) * (1 + t * t / nu) ** (-(nu + 1) / 2)
    h = t[1] - t[0]
    return 0.5 + h / 3 * (f[0] + f[-1] + 4 * f[1:-1:2].sum() + 2 * f[2:-1:2].sum())


def test_quartiles_without_moments_cover_the_small_shape_branch():
    """nu = 0.8, nothing observed: a = 0.4 < 1, the u_b^(1/a) branch; coordinate 1 is t_0.8(mu_1, sigma_11)"""
    D, nu = 3, 0.8
    mu = np.array([[0.3, -2.0, 1.0]])
    Lc = np.array([[1.0, 0, 0], [0.5, 1.2, 0], [-0.3, 0.4, 0.8]])
    sigma = (Lc @ Lc.T)[None]
    tr = ST.draw(None, None, T.pack_t(np.zeros(1), mu, sigma, np.full(1, nu)), seed=4242, N=N_LAW)
    assert not tr['exhausted'].any() and tr['attempts'].max() < ST.ATTEMPTS
    y = (tr['x'][0][:, 1] - mu[0, 1]) / math.sqrt(sigma[0, 1, 1])
    lo, hi = 0.0, 50.0                                              # the upper quartile of the standard t_0.8 by bisection
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _t_cdf(mid, nu) < 0.75 else (lo, mid)
    q3 = 0.5 * (lo + hi)
    for p, qp in ((0.25, -q3), (0.5, 0.0), (0.75, q3)):
        frac = (y < qp).mean()
        assert abs(frac - p) <= 5 * math.sqrt(p * (1 - p) / N_LAW), (p, qp, frac)


def test_rows_are_a_function_of_their_absolute_index():
    N, D, K = 65, 3, 17
    x, miss, t, _, seed = ST.case_inputs(N, D, K)
    pk = T.pack_t(**t)
    full = ST.draw(x, miss, pk, seed, 0, 2)
    r = 23
    part = ST.draw(x[r:], miss[r:], pk, seed, r, 2)
    assert np.array_equal(full['x'][:, r:], part['x'], equal_nan=True) and np.array_equal(full['z'][:, r:], part['z'])
    other = ST.draw(x, miss, pk, seed + 1, 0, 2)
    assert (other['x'][:, miss != 0] != full['x'][:, miss != 0]).mean() > 0.99


def test_uniforms_and_normals_follow_the_documented_layout():
    from oracle import philox
    rows = np.array([0, 5, 2 ** 33 + 1], dtype=np.uint64)
    w = ST._words(77, rows, 2, ST.B_EPS)
    ctr = np.array([[5, 0, 1, ST.SAMPLE_TAG + 1]], dtype=np.uint32)
    key = np.array([[77, 0]], dtype=np.uint32)
    assert np.array_equal(w[1, 1], philox.philox4x32(ctr, key)[0])
    assert np.array_equal(ST._words(77, rows, 1, 0)[0, 2], philox.philox4x32(np.array([[1, 2, 0, ST.SAMPLE_TAG]], dtype=np.uint32), key)[0])
    eps = ST.normals(77, rows, 2, 5)
    bm = philox.box_muller8(w)                                       # (2, 3, 4, 2)
    assert np.array_equal(eps, bm.reshape(2, 3, 8)[..., :5])
    u = ST.uniform(np.array([0, 0xFFFFFFFF], dtype=np.uint32), np.float64)
    assert u[0] == 2.0 ** -25 and u[1] == 1 - 2.0 ** -24 and ST.uniform(np.array([0xFFFFFFFF], dtype=np.uint32), np.float32)[0] < 1
    assert ST.SAMPLE_TAG + 16 + ST.ATTEMPTS < 2 ** 32 and ST.SAMPLE_TAG not in (0, philox.SUBSAMPLE_TAG)
    assert not ST.SAMPLE_TAG <= philox.SUBSAMPLE_TAG < ST.SAMPLE_TAG + 256


def test_attempt_cap_bound():
    """rejection probability of one attempt: 1 - e^d Gamma(a') d^-a' / (3 c sqrt(2 pi)), largest at a' = 1: 0.0484^8 < 1e-9"""
    def reject(ap):
        d = ap - 1 / 3
        c = 1 / math.sqrt(9 * d)
        return 1 - math.exp(d + math.lgamma(ap) - ap * math.log(d)) / (3 * c * math.sqrt(2 * math.pi))
    r = [reject(ap) for ap in (1.0, 1.2, 1.5, 2.0, 4.0, 25.0, 1000.0)]
    assert r[0] < 0.0484 and all(a > b for a, b in zip(r, r[1:])) and r[-1] > 0
    assert r[0] ** ST.ATTEMPTS < 1e-9


@pytest.mark.parametrize('N,D,K', ST.SWEEP + [ST.LONG_N])
def test_the_constants_of_the_gpu_test_hold_over_its_sweep(N, D, K):
    """per case, builder and number of draws: the truth alone leaves <= 1 % of the rows undecidable at TAU, never exhausts the attempt
    cap, TAU >= 4 x the largest margin at which the fp32 restatement decides otherwise, BAR >= 4 x its error on the decidable rows"""
    x, miss, t, q, seed = ST.case_inputs(N, D, K)
    long = (N, D, K) == ST.LONG_N
    for builder, pk in (('t', T.pack_t(**t)), ('niw', T.pack_niw(**q))):
        for draws in ((1,) if long else (1, 3)):
            tr, flip, err = ST.measure(x, miss, pk, seed, draws)
            und = ST.undecidable(tr, ST.TAU).mean()
            e = err(ST.TAU)
            print('N=%d D=%d K=%d %s draws=%d: undecidable %.4f  flip margin %.3e  restatement error %.3e' % (N, D, K, builder, draws, und, flip, e))
            assert und <= 0.01, (builder, draws, und)
            assert not tr['exhausted'].any() and (tr['z'] >= 0).all()
            assert 4 * flip <= ST.TAU and 4 * e <= ST.BAR * (1 + 1e-9), (builder, draws, flip, e)
            assert (miss[0] == 1).all() and (N == 1 or (miss[1] == 0).all())
