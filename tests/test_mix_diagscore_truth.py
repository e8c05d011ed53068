"""The fp64 truth of the diagonal mixture's scoring pass (tests/mix_diagscore_truth.py) against independent statements of the same
mathematics, and the proof that the large-count case tells a true log1p from log(1 + t) in fp32.  No GPU."""
import math

import numpy as np
import pytest

import mix_diagscore_truth as S


@pytest.mark.parametrize('a,b,beta,m,x', [(1.0, 1.0, 0.5, 0.0, 0.3), (1.0, 1.0, 0.5, 2.0, -7.0), (2.5, 3.0, 4.5, -1.0, 0.5),
                                          (51.0, 40.0, 100.5, 3.0, 4.5), (501.0, 730.0, 1000.5, 1000.0, 1002.0), (0.4, 2.0, 0.5, 0.0, 5.0)])
def test_log_student_t_is_the_normal_gamma_integral(a, b, beta, m, x):
    theta = tuple(np.array(v, np.float64) for v in ([1.0], [beta], [[m]], [a], [[b]]))
    got = S.score(np.array([[x]]), theta)['logp'][0]                         # K = 1, log w = 0
    want = S.quad_log_st(x, m, a, b, beta)
    assert abs(got - want) < 1e-11 * max(1.0, abs(want)), (got, want)


def test_gaussian_limit_at_large_counts():
    theta, s = S.explicit_theta([1e8], 5, 3)
    x = S.rows_near(theta, s, 20, 4)
    al, be, m, a, b = [np.asarray(t, np.float64) for t in theta]
    var = b / a[:, None] * (1 + be[:, None]) / be[:, None]
    gauss = (-0.5 * np.log(2 * math.pi * var) - 0.5 * (x.astype(np.float64) - m) ** 2 / var).sum(1)
    assert np.abs(S.score(x, theta)['logp'] - gauss).max() < 1e-5            # O(1/a) per coordinate


def test_masked_row_is_the_truth_of_its_observed_columns():
    theta, s = S.explicit_theta([0, 3, 50, 400], 9, 5)
    x = S.rows_near(theta, s, 12, 6)
    rng = np.random.Generator(np.random.PCG64(7))
    miss = rng.random(x.shape) < 0.4
    miss[0] = False
    miss[1, 1:] = True                                                        # one observed coordinate
    full = S.score(x, theta, miss)
    for n in range(x.shape[0]):
        cols = np.flatnonzero(~miss[n])
        sub = (theta[0], theta[1], theta[2][:, cols], theta[3], theta[4][:, cols])
        one = S.score(x[n:n + 1, cols], sub)
        assert abs(one['logp'][0] - full['logp'][n]) < 1e-12 * max(1, abs(one['logp'][0]))
        assert np.abs(one['resp'][0] - full['resp'][n]).max() < 1e-12
        assert np.array_equal(full['filled'][n, cols], x[n, cols].astype(np.float64))
        gone = np.flatnonzero(miss[n])
        assert np.allclose(full['filled'][n, gone], full['resp'][n] @ np.asarray(theta[2], np.float64)[:, gone], rtol=0, atol=1e-12)


def test_row_with_nothing_observed():
    theta, s = S.explicit_theta([0, 3, 50], 4, 8)
    x = np.full((2, 4), np.nan, np.float32)
    out = S.score(x, theta, np.ones((2, 4), bool))
    w = np.asarray(theta[0], np.float64) / np.asarray(theta[0], np.float64).sum()
    assert np.abs(out['logp']).max() < 1e-12 and np.abs(out['resp'] - w).max() < 1e-12
    assert np.allclose(out['filled'], w @ np.asarray(theta[2], np.float64), rtol=0, atol=1e-12)


def test_degenerate_theta_gives_a_nan_pack_row():
    theta, _ = S.explicit_theta([5, 5, 5], 4, 9)
    theta[4][1, 2] = 0
    p = S.pack_array(S.pack(theta))
    assert np.isnan(p[1]).all() and np.isfinite(p[[0, 2]]).all() and p.shape == (3, 3 * 4 + 3)


def test_large_counts_tell_log1p_from_log_of_one_plus_t():
    """N_k = 1e6, D = 64: a = 5e5 multiplies the 6e-8 that rounding 1 + t costs.  The fp32 restatement with log(1 + t) misses the
    bar the one with log1p sets; measured 0.44 against 1.8e-5 absolute on a row term of about 72."""
    theta, s = S.explicit_theta([1e6], 64, 11)
    x = S.rows_near(theta, s, 200, 12)
    t = S.bars(x, theta)
    plain = S.errors(S.score(x, theta, None, np.float32, plain_log=True), t)
    print('logp: log1p %.3e  bar %.3e  log(1 + t) %.3e  (|logp| about %.1f)' % (t['e_logp'], t['bar_logp'], plain['logp'], np.abs(t['logp']).mean()))
    assert t['e_logp'] <= t['bar_logp'] < plain['logp']
    assert plain['logp'] > 100 * t['e_logp']
