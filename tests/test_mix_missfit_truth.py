"""The fp64 truth of the masked mixture fit (tests/mix_missfit_truth.py) against three things that do not share its code: a brute-force
route through the full covariance (marginal of the observed block, Gaussian conditioning of the missing block, written with
numpy.linalg cell by cell), the monotone rise of the variational lower bound, and - on an all-zero mask - the oracle's
complete-data GMM iteration."""
import math

import numpy as np
import torch

import mix_missfit_truth as T


def _theta(K, D, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.standard_normal((K, D, D)) / math.sqrt(D)
    v = D + rng.uniform(2.0, 30.0, K)
    C = (A @ A.transpose(0, 2, 1) + 0.5 * np.eye(D)) * v[:, None, None]
    return tuple(torch.as_tensor(t) for t in (rng.uniform(0.5, 40.0, K), rng.uniform(0.5, 30.0, K), rng.standard_normal((K, D)) * 3.0, C, v))


def test_truth_against_brute_force_through_the_covariance():
    N, D, K = 40, 4, 3
    x, _, miss = T.make_data(N, D, K, seed=11, frac=0.3)
    theta = _theta(K, D, 12)
    e = T.e_step(x, miss, theta, with_const=True)
    al, be, m, C, v = (t.numpy() for t in theta)
    m_, Lbar, c, elp, eld = (t.numpy() for t in T.expectations(theta))
    assert np.allclose(m_, m)
    log_rho = np.zeros((N, K))
    sx, sxx, fill = np.zeros((K, D)), np.zeros((K, D, D)), np.zeros((N, D))
    xh_all, cov_all = np.zeros((N, K, D)), np.zeros((N, K, D, D))
    for n in range(N):
        o, g = np.nonzero(miss[n] == 0)[0], np.nonzero(miss[n] != 0)[0]
        for k in range(K):
            Sigma = np.linalg.inv(Lbar[k])                                 # covariance of N(x | m_k, Lbar_k^-1)
            xh = m[k].copy()
            cov = np.zeros((D, D))
            quad, logdet_oo = 0.0, 0.0
            if len(o):
                Soo = Sigma[np.ix_(o, o)]
                d = x[n, o].astype(np.float64) - m[k, o]
                sol = np.linalg.solve(Soo, d)
                quad = d @ sol
                logdet_oo = np.linalg.slogdet(Soo)[1]
                xh[o] = x[n, o]
                if len(g):
                    Smo = Sigma[np.ix_(g, o)]
                    xh[g] = m[k, g] + Smo @ sol
                    cov[np.ix_(g, g)] = Sigma[np.ix_(g, g)] - Smo @ np.linalg.solve(Soo, Smo.T)
            else:
                cov = Sigma
            # E log N(x_o | mu_o, (Lambda^-1)_oo)-like term: the full-row expectation with x_m integrated out,
            # log|Lbar_mm| = log|Sigma_oo| + log|Lbar|
            half_logdet_mm = 0.5 * (logdet_oo + np.linalg.slogdet(Lbar[k])[1])
            log_rho[n, k] = elp[k] + 0.5 * eld[k] - 0.5 * D / be[k] - 0.5 * quad - half_logdet_mm - 0.5 * len(o) * math.log(2 * math.pi)
            xh_all[n, k], cov_all[n, k] = xh, cov
    r = np.exp(log_rho - log_rho.max(1, keepdims=True))
    r /= r.sum(1, keepdims=True)
    assert np.abs(e['log_rho'].numpy() - log_rho).max() < 1e-9
    assert np.abs(e['r'].numpy() - r).max() < 1e-10
    assert np.abs(e['xhat'].numpy() - xh_all).max() < 1e-9
    assert np.abs(e['cov'].numpy() - cov_all).max() < 1e-9
    gone = miss != 0
    fill = np.einsum('nk,nkd->nd', r, xh_all)
    assert np.abs(e['x_fill'].numpy()[gone] - fill[gone]).max() < 1e-9
    assert np.array_equal(e['x_fill'].numpy()[~gone], x[~gone].astype(np.float64))
    st = T.moments(e['r'], e['xhat'], e['cov'], None).numpy()
    Nk = r.sum(0)
    sx = np.einsum('nk,nkd->kd', r, xh_all)
    sxx = np.einsum('nk,nkde->kde', r, xh_all[:, :, :, None] * xh_all[:, :, None, :] + cov_all)
    want = np.concatenate([Nk[:, None], Nk[:, None], sx, sxx.reshape(K, -1)], 1)
    assert np.abs(st - want).max() < 1e-8
    # the fp32 restatement of the same moments (shifted, block sums) is the same quantity to fp32 accuracy
    st32 = T.moments(e['r'].float(), e['xhat'].float(), e['cov'].float(), theta[2], torch.float32).numpy()
    assert np.abs(st32 - want).max() / np.abs(want).max() < 1e-5


def test_seeding_fills_with_the_observed_column_mean_and_adds_no_covariance():
    N, D, K = 50, 3, 2
    x, r0, miss = T.make_data(N, D, K, seed=3, frac=0.4)
    miss[:, 2] = 1                                                         # a column without any observed entry: filled with 0
    x[:, 2] = np.nan
    xs, mean = T.mean_filled(x, miss)
    for d in range(D):
        obs = miss[:, d] == 0
        want = x[obs, d].astype(np.float64).mean() if obs.any() else 0.0
        assert abs(mean[d].item() - want) < 1e-12
        assert np.allclose(xs.numpy()[~obs, d], want) and np.array_equal(xs.numpy()[obs, d], x[obs, d].astype(np.float64))
    st = T.seed_stats(x, miss, r0).numpy()
    r = r0.astype(np.float64)
    want = np.concatenate([r.sum(0)[:, None], r.sum(0)[:, None], r.T @ xs.numpy(),
                           np.einsum('nk,nd,ne->kde', r, xs.numpy(), xs.numpy()).reshape(K, -1)], 1)
    assert np.abs(st - want).max() < 1e-9


def test_lower_bound_is_non_decreasing():
    N, D, K = 300, 4, 3
    x, r0, miss = T.make_data(N, D, K, seed=5, frac=0.3)
    assert (miss.sum(1) == D).any() and (miss.sum(1) == 0).any()
    prior = T.default_prior(K, D)
    stats = T.seed_stats(x, miss, r0)
    bound = []
    for _ in range(20):
        it = T.one_iteration(x, miss, stats, prior)
        stats = it['stats']
        bound.append(T.lower_bound(x, miss, it['theta'], prior))
    print('lower bound: ' + ' '.join('%.6f' % b for b in bound))
    assert all(math.isfinite(b) for b in bound)
    for a, b in zip(bound, bound[1:]):
        assert b >= a - 1e-9, bound
    assert bound[-1] > bound[0] + 1.0


def test_all_zero_mask_is_the_oracles_complete_data_iteration():
    from oracle import mixtures
    N, D, K = 120, 3, 4
    x, r0, _ = T.make_data(N, D, K, seed=8, frac=0.0)
    x = np.nan_to_num(x)                                                   # row 0 is forced missing by make_data: give it values
    miss = np.zeros((N, D), np.uint8)
    xo, ro = torch.as_tensor(x).double(), torch.as_tensor(r0).double()
    out = dict(stats=T.seed_stats(x, miss, r0))
    for _ in range(3):
        out = T.one_iteration(x, miss, out['stats'], T.default_prior(K, D))
        ro, logr, th, _ = mixtures.gmm_inference_step(xo, ro)
        assert (out['r'] - ro).abs().max().item() < 1e-12
        for a, b in zip(out['theta'], th):
            assert ((a - b).abs() / b.abs().clamp_min(1.0)).max().item() < 1e-12
        assert torch.equal(out['x_fill'], xo)
