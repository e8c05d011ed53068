"""The truth of the variational lower bound in parts (tests/mix_bound_truth.py) against its definition
(tests/mix_missfit_truth.lower_bound), on the CPU: the parts add up, the data term is the free energy of the responsibilities, and
the sequences that the GPU loop tests compare against rise."""
import functools

import numpy as np
import pytest
import torch

import mix_bound_truth as B
import mix_missfit_truth as T

ITERATIONS = 12


@functools.lru_cache(maxsize=None)
def _thetas(N, D, K, frac):
    """theta after each of ITERATIONS fp64 iterations: computed once, shared, never modified"""
    x, r0, miss = B.loop_input(N, D, K, frac)
    m = B._mask(x, miss)
    prior = T.default_prior(K, D)
    stats = T.seed_stats(x, m, r0)
    out = []
    for _ in range(ITERATIONS):
        it = T.one_iteration(x, m, stats, prior)
        stats = it['stats']
        out.append(it['theta'])
    return x, miss, out


@pytest.mark.parametrize('N,D,K,frac', B.LOOP_INPUTS)
def test_parts_sum_to_the_definition(N, D, K, frac):
    x, miss, thetas = _thetas(N, D, K, frac)
    for theta in (thetas[0], thetas[4], thetas[-1]):
        p = B.parts(x, miss, theta)
        want = T.lower_bound(x, B._mask(x, miss), theta)
        got = p['data'] - p['kl_pi'] - p['kl_nw'].sum().item()
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
        assert p['kl_pi'] >= 0 and (p['kl_nw'] >= 0).all()                      # each is a KL divergence


def test_parts_with_a_prior_of_their_own():
    N, D, K, frac = B.LOOP_INPUTS[0]
    x, miss, thetas = _thetas(N, D, K, frac)
    rng = np.random.Generator(np.random.PCG64(3))
    A = rng.standard_normal((K, D, D))
    prior = (torch.as_tensor(rng.random(K) + 0.1), torch.as_tensor(rng.random(K) + 0.2), torch.as_tensor(rng.standard_normal((K, D))),
             torch.as_tensor(A @ A.transpose(0, 2, 1) + np.eye(D)), torch.as_tensor(rng.random(K) * 3 + D))
    p = B.parts(x, miss, thetas[2], prior)
    want = T.lower_bound(x, miss, thetas[2], prior)
    got = p['data'] - p['kl_pi'] - p['kl_nw'].sum().item()
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)


@pytest.mark.parametrize('N,D,K,frac', B.LOOP_INPUTS[:1] + B.LOOP_INPUTS[3:])
def test_data_term_is_the_free_energy_of_the_responsibilities(N, D, K, frac):
    """sum_n logsumexp_k log rho_nk = sum_nk r_nk (log rho_nk - log r_nk) at r = softmax log rho"""
    x, miss, thetas = _thetas(N, D, K, frac)
    e = T.e_step(x, B._mask(x, miss), thetas[1], torch.float64, with_const=True)
    r, logr = e['r'], e['logr']
    free = torch.where(r > 0, r * (e['log_rho'] - logr), torch.zeros_like(r)).sum().item()
    p = B.parts(x, miss, thetas[1])
    assert abs(free - p['data']) <= 1e-9 * max(1.0, abs(p['data'])), (free, p['data'])
    n_obs = (B._mask(x, miss) == 0).sum(1)
    assert torch.allclose(p['lse'], e['lse'] + 0.5 * torch.as_tensor(n_obs).double() * T.LOG_2PI, rtol=0, atol=1e-12)


@pytest.mark.parametrize('N,D,K,frac', B.LOOP_INPUTS)
def test_truth_sequences_of_the_loop_tests_are_non_decreasing(N, D, K, frac):
    x, miss, thetas = _thetas(N, D, K, frac)
    bound = [T.lower_bound(x, B._mask(x, miss), th) for th in thetas]
    print('lower bound N=%d D=%d K=%d: ' % (N, D, K) + ' '.join('%.6f' % b for b in bound))
    assert all(np.isfinite(bound))
    gains = np.diff(bound)
    print('smallest gain: %.6f' % gains.min())
    assert (gains >= 0).all(), bound


def test_fp32_restatement_and_bars():
    N, D, K, frac = B.LOOP_INPUTS[0]
    x, miss, thetas = _thetas(N, D, K, frac)
    theta32 = tuple(t.float() for t in thetas[0])
    c = B.case(x, miss, theta32)
    assert c['bar_data'] >= B.FLOOR and c['bar_bound'] >= B.FLOOR and c['bar_lse'] >= B.FLOOR
    assert c['e_data'] < 1e-5 and c['e_lse'] < 1e-4, (c['e_data'], c['e_lse'])  # fp32 on a few hundred rows: far from the truth it is not
    assert c['lse'].shape == (N,) and c['kl_nw'].shape == (K,)
    seq = B.sequence(x, miss, T.make_data(N, D, K, seed=7, frac=frac)[1], 2)
    assert len(seq) == 2 and abs(seq[0]['bound'] - T.lower_bound(x, miss, thetas[0])) < 1e-9 * abs(seq[0]['bound'])
    assert all(s['bar'] >= B.FLOOR for s in seq)
