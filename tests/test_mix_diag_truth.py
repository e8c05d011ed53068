"""The fp64 truth of the diagonal-covariance mixture (tests/mix_diag_truth.py) checks itself: both updates are exact coordinate
ascent, so the lower bound never falls; every KL term is non-negative; an empty component keeps its prior; and at K = 1, where q is
the exact posterior, the bound is the closed-form log marginal likelihood."""
import numpy as np
import pytest
import torch

import mix_diag_truth as T

CASES = [(N, D, K, 0.0) for N, D, K in T.SHAPES] + [(1031, 33, 33, 1000.0)]


@pytest.mark.parametrize('N,D,K,offset', CASES)
def test_bound_never_falls_and_kl_terms_are_non_negative(N, D, K, offset):
    x, r0 = T.make_data(N, D, K, 10 * D + K, offset)
    out = T.iterate(x, r0, T.default_prior(x, K), 30)
    b = np.array(out['bounds'])
    # exact arithmetic: never falls.  The fp64 evaluation adds N row terms and K D KL terms, each rounded to 2^-53 of its size: a
    # converged fit may move by a few units in the last place of the bound.  1e-12 relative is ~4500 of them and far below any
    # step that changes the fit.
    assert np.isfinite(b).all() and (np.diff(b) >= -1e-12 * np.maximum(1.0, np.abs(b[:-1]))).all(), np.diff(b).min()
    assert (out['kl_ng'] >= 0).all() and out['kl_pi'] >= 0


def test_an_empty_component_keeps_its_prior():
    N, D, K = 200, 7, 4
    x, r0 = T.make_data(N, D, K, 3)
    r0[:, 2] = 0.0
    r0 /= r0.sum(1, keepdims=True)
    prior = T.default_prior(x, K)
    theta = T.m_step(*T.moments(x, r0, torch.float64), prior, torch.float64)
    for t, p in zip(theta, prior):
        assert torch.isfinite(t).all()
        assert torch.equal(t[2], torch.as_tensor(p).double()[2])
    r, logr, data = T.e_step(x, theta, torch.float64)
    assert torch.isfinite(r).all() and np.isfinite(data)


@pytest.mark.parametrize('N,D', [(300, 1), (130, 9), (64, 64)])
def test_k1_bound_is_the_log_marginal_likelihood(N, D):
    x, r0 = T.make_data(N, D, 1, 5)
    prior = T.default_prior(x, 1)
    out = T.iterate(x, r0, prior, 1)
    lm = T.log_marginal(x, prior)
    assert abs(out['bound'] - lm) <= 1e-9 * abs(lm), (out['bound'], lm)
