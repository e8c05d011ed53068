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


def test_aux_is_the_centred_moments_and_the_expected_weights():
    N, D, K = 257, 17, 3
    x, r0 = T.make_data(N, D, K, 4)
    r0[:, 1] = 0.0
    r0 /= r0.sum(1, keepdims=True)
    prior = T.default_prior(x, K)
    out = T.iterate(x, r0, prior, 1)
    xd, rd = torch.as_tensor(x).double(), torch.as_tensor(r0).double()
    Nk = rd.sum(0)
    assert Nk[1] == 0 and (out['xbar'][1] == 0).all() and (out['S'][1] == 0).all()
    for k in (0, 2):
        xbar = (rd[:, k:k + 1] * xd).sum(0) / Nk[k]
        S = (rd[:, k:k + 1] * (xd - xbar) ** 2).sum(0) / Nk[k]
        assert T.rel_err(out['xbar'][k], xbar) < 1e-12 and T.rel_err(out['S'][k], S) < 1e-12
    # pi = exp(E log pi) under Dir(alpha): below the mean alpha / sum alpha, and close to it for a large alpha
    alpha = out['theta'][0]
    assert (out['pi'] < alpha / alpha.sum()).all() and T.rel_err(out['pi'][0], alpha[0] / alpha.sum()) < 1.0 / alpha[0].item()
    assert torch.equal(out['kl_k'], out['kl_ng'].sum(1)) and out['kl_sum'] == out['kl_ng'].sum().item()
    b = T.bars(x, r0, prior, 1)
    for name in ('xbar', 'S', 'pi', 'kl_pi', 'kl_k', 'kl_sum'):
        assert 0 <= b['e_' + name] < 1e-3 and b['bar_' + name] == max(1e-5, 3 * b['e_' + name])


def test_geometry_of_the_four_block_shapes():
    g = T.geometry(40003, 3, 2)
    assert (g['blocks'], g['waves'], g['rpw']) == (20, 80, 512)                        # 80 / 16 = 5 waves per reduce group
    g = T.geometry(150001, 2, 17)
    assert (g['cap'], g['blocks']) == (512, 74)                                        # more than 64 blocks
    g = T.geometry(1100003, 1, 2)
    assert (g['cap'], g['blocks'], g['waves'], g['rpw'], g['empty']) == (512, 512, 2048, 576, 138)
    g = T.geometry(600001, 16, 64)
    assert 64 * 33 == 2112 and (g['cap'], g['blocks'], g['waves'], g['rpw'], g['empty']) == (256, 256, 1024, 640, 86)
    g = T.geometry(600, 64, 64)
    assert (g['blocks'], g['rpw'], g['empty']) == (1, 192, 0)                          # three tiles a wave, 24 rows in the last
    assert T.workspace_blocks(8 * 74 * (4 * 17 * 5 + 1) + 256, 2, 17) == 74


def test_chunked_pass_truth_is_the_unchunked_truth():
    N, D, K = 1031, 33, 33
    x, r0 = T.make_data(N, D, K, 8)
    prior = T.default_prior(x, K)
    theta = [t.float() for t in T.m_step(*T.moments(x, r0, torch.float64), prior, torch.float64)]
    whole = {}
    for dtype in (torch.float64, torch.float32):
        r, logr, data = T.e_step(x, [t.to(dtype) for t in theta], dtype)
        whole[dtype] = (r, logr, data, T.raw_stats(*T.moments(x, r, dtype)))
    r64, l64, d64, s64 = whole[torch.float64]
    r32, l32, d32, s32 = whole[torch.float32]
    for chunk in (300, 1031, 65536):                                                   # four chunks, one exact, one larger than N
        out = T.pass_truth(x, theta, got_r=r32, got_logr=l32, chunk=chunk)
        assert T.rel_err(out['stats'], s64) < 1e-12 and abs(out['data'] - d64) <= 1e-12 * abs(d64)
        assert T.rel_err(out['stats32'], s32) < 1e-5 and abs(out['data32'] - d32) <= 1e-12 * abs(d32)
        # a row's r and log r do not depend on the chunking: the restatement's errors are the unchunked ones, and so are a guest's
        assert out['e_r'] == T.abs_err(r32, r64) == out['err_r'] and out['e_logr'] == T.rel_err(l32, l64) == out['err_logr']
        assert out['e_data'] == T.rel_err(out['data32'], out['data']) and out['bar_stats'] == max(1e-5, 3 * out['e_stats'])
    wrong = r64.clone()
    wrong[700, 3] += 1e-3                                                              # in the third chunk of 300
    assert abs(T.pass_truth(x, theta, got_r=wrong, chunk=300)['err_r'] - 1e-3) < 1e-9


@pytest.mark.parametrize('N,D,K', [(600, 64, 64), (40003, 3, 2), (2051, 5, 17)])
def test_integer_moments_are_exact_in_the_fp32_model_of_the_kernel(N, D, K):
    xi, z = T.int_case(N, D, K)
    assert xi.min() == 0 and xi.max() == 3 and z.min() == 0 and z.max() == K - 1
    want = T.int_stats(xi, z, K)
    assert want.dtype == np.int64 and want[:, 0].sum() == N
    assert (want[:, 1:1 + D].sum(0) == xi.sum(0)).all() and (want[:, 1 + D:].sum(0) == (xi * xi).sum(0)).all()
    r = T.one_hot(z, K).astype(np.int64)
    assert (want == np.concatenate([r.sum(0)[:, None], r.T @ xi, r.T @ (xi * xi)], 1)).all()
    got = T.int_model(xi, z, K)                                                        # asserts the bit counts on its way
    assert got.dtype == np.float64 and (got == want).all()


@pytest.mark.parametrize('N,D,K', [(1, 64, 64), (1, 1, 1), (2, 9, 17), (63, 17, 3), (64, 33, 33)])
def test_truth_is_finite_at_tiny_n(N, D, K):
    x, r0 = T.make_data(N, D, K, 100 * D + 7 * K + N % 11)
    prior = T.default_prior(x, K)
    for iterations in (1, 3):
        out = T.bars(x, r0, prior, iterations)
        for name in ('r', 'logr', 'stats', 'xbar', 'S', 'pi', 'kl_ng'):
            assert torch.isfinite(out[name]).all(), name
        assert all(torch.isfinite(t).all() for t in out['theta']) and np.isfinite([out['data'], out['bound'], out['kl_pi']]).all()
        assert all(np.isfinite(v) for k, v in out.items() if k.startswith('bar_'))
    if N == 1:                                                                         # one row: every component sits on it
        one = T.iterate(x, r0, prior, 1)
        assert (one['S'] == 0).all() and torch.equal(one['xbar'], torch.as_tensor(x).double().expand(K, D))


def test_planted_clusters_leave_no_mass_an_fp32_can_hold():
    """40 sd apart the wrong components' r is about e^-400: not zero in fp64 (that needs log r < -745), but far below half the
    smallest fp32 subnormal, 2^-150 - the correctly rounded fp32 r is exactly one-hot, and so is the fp32 restatement's"""
    x, centres, z = T.planted_clusters(600, 24, 4, 40.0, 11)
    d2 = ((x[:, None, :].astype(np.float64) - centres[None, :, :]) ** 2).sum(2)
    assert (d2.argmin(1) == z).all()                                                   # the nearest centre is the planted one
    r0 = T.one_hot(z, 4)
    prior = T.default_prior(x, 4)
    out = T.bars(x, r0, prior, 2)
    r, hot = out['r'], torch.as_tensor(r0).double()
    assert r.dtype == torch.float64 and torch.equal(r.argmax(1), torch.as_tensor(z))
    assert (r.max(1).values == 1).all() and (r.sum(1) == 1).all() and (r * (1 - hot)).max() < 2.0 ** -150
    assert torch.isfinite(out['logr']).all() and (out['logr'] + 200 * (1 - hot)).max() <= 0
    assert torch.equal(T.iterate(x, r0, prior, 2, torch.float32)['r'].double(), hot)
    assert out['e_r'] < 1e-30 and out['bar_r'] == 1e-5


def test_mpmath_terms_are_the_fp64_terms():
    N, D, K = 257, 17, 3
    x, r0 = T.make_data(N, D, K, 6)
    prior = T.default_prior(x, K)
    mom = T.moments(x, r0, torch.float64)
    theta = [t.float() for t in T.m_step(*mom, prior, torch.float64)]
    kl_pi, kl_ng = T.kl_terms(theta, prior)
    mp_pi, mp_ng = T.mp_terms([t.numpy() for t in theta], prior)
    assert T.mp_err([kl_pi], [mp_pi], 1.0) < 1e-12 and T.mp_err(kl_ng, mp_ng, 1.0) < 1e-12
    assert T.mp_err(kl_ng.sum(1), mp_ng.sum(1), 1.0) < 1e-12
    # the finalize and the pack in mpmath are the fp64 M-step and the constants of the E-step
    fin = T.mp_finalize(T.raw_stats(*mom).numpy(), prior)
    for name, t in zip(T.NAMES, T.m_step(*mom, prior, torch.float64)):
        assert T.mp_err(t, fin[name], 1.0) < 1e-12, name
    xbar, S, pi = T.aux(*mom, mom[0] + torch.as_tensor(prior[0]).double())
    assert T.mp_err(xbar, fin['xbar'], 1.0) < 1e-12 and T.mp_err(S, fin['S'], 1.0) < 1e-11 and T.mp_err(pi, fin['pi'], 1.0) < 1e-12
    pack = T.mp_pack([t.numpy() for t in theta])
    al, be, m, a, b = [t.double() for t in theta]
    dg = torch.special.digamma
    c = dg(al) - dg(al.sum()) + 0.5 * (dg(a)[:, None] - torch.log(b)).sum(1) - D / (2 * be)
    assert T.mp_err(torch.cat([m, a[:, None] / b, c[:, None]], 1), pack, 1.0) < 1e-12
    assert T.mp_err([1.0 + 2.0 ** -20], [1.0], 1.0) == 2.0 ** -20 and T.mp_err([0.0], [0.0], 2.0 ** -126) == 0.0
