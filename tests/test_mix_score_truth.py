"""The fp64 truth that tests/test_mix_score_gpu.py compares the kernels with (tests/mix_score_truth.py) against independent
statements of the same densities: scipy.stats.multivariate_t (when scipy imports), the oracle's Student-t (oracle/dists.py), and
the Gaussian limit of the GMM predictive.  No GPU."""
import math

import numpy as np
import pytest
import torch

import mix_score_truth as T


@pytest.mark.parametrize('D,K', [(1, 3), (3, 5), (8, 4)])
def test_explicit_pack_matches_scipy_multivariate_t(D, K):
    st = pytest.importorskip('scipy.stats')
    x, t, _ = T.make_case(97, D, K, seed=11 * D + K)
    terms, logp, resp = T.evaluate(x, T.pack_t(**t))
    x64 = x.astype(np.float64)
    want = np.stack([st.multivariate_t.logpdf(x64, loc=t['mu'][k].astype(np.float64), shape=t['sigma'][k].astype(np.float64),
                                              df=float(t['nu'][k])).reshape(-1) + float(t['log_w'][k]) for k in range(K)], 1)
    assert np.abs(terms.numpy() - want).max() < 1e-9 * max(1.0, np.abs(want).max())
    from scipy.special import logsumexp
    assert np.abs(logp.numpy() - logsumexp(want, axis=1)).max() < 1e-9 * max(1.0, np.abs(want).max())
    assert np.abs(resp.sum(1).numpy() - 1).max() < 1e-12


@pytest.mark.parametrize('D,K', [(2, 3), (5, 17)])
def test_explicit_pack_matches_the_oracle_student_t(D, K):
    from oracle import dists
    x, t, _ = T.make_case(61, D, K, seed=5 * D + K)
    terms, _, _ = T.evaluate(x, T.pack_t(**t))
    d = lambda a: torch.as_tensor(a).double()
    y = d(x)[:, None, None, :].expand(-1, K, 1, -1)
    want = dists.student_t_log_probability_per_samp(y, d(t['mu']), d(t['sigma']), d(t['nu'])).reshape(-1, K) + d(t['log_w'])[None, :]
    assert (terms - want).abs().max().item() < 1e-9 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('D,K', [(1, 2), (3, 4), (8, 3)])
def test_niw_pack_is_bishop_10_81(D, K):
    """component k of the predictive = St(x | m_k, L_k, nu'), L_k = nu' beta / (1 + beta) C_k^-1, i.e. scipy's multivariate_t with
    shape L_k^-1, weighted by alpha_k / sum alpha"""
    st = pytest.importorskip('scipy.stats')
    x, _, q = T.make_case(83, D, K, seed=3 * D + K)
    terms, _, _ = T.evaluate(x, T.pack_niw(**q))
    p = {k: a.astype(np.float64) for k, a in q.items()}
    for k in range(K):
        nup = p['v'][k] + 1 - D
        shape = p['C'][k] * (1 + p['beta'][k]) / (nup * p['beta'][k])
        want = st.multivariate_t.logpdf(x.astype(np.float64), loc=p['m'][k], shape=shape, df=nup).reshape(-1) \
            + math.log(p['alpha'][k] / p['alpha'].sum())
        assert np.abs(terms[:, k].numpy() - want).max() < 1e-9 * max(1.0, np.abs(want).max()), k


def test_fp32_restatement_is_close_and_the_bar_has_its_floor():
    x, t, _ = T.make_case(257, 5, 17, seed=1)
    lp, rs, bar_lp, bar_rs, e_lp, e_rs = T.bars(x, T.pack_t(**t))
    assert 0 < e_lp < 1e-4 and 0 <= e_rs < 1e-4
    assert bar_lp == max(1e-5, 3 * e_lp) and bar_rs == max(1e-5, 3 * e_rs)
    assert torch.isfinite(lp).all() and (rs.sum(1) - 1).abs().max() < 1e-12
