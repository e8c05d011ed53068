"""The fp64 truth of the diagonal mixture fit on partly observed and weighted rows (tests/mix_dmfit_truth.py) against what it must
reduce to and what it must guarantee, on the CPU: a zero mask with unit weights is the complete-row truth, integer weights are
replicated rows, and both updates are exact coordinate ascent - the bound never falls."""
import numpy as np
import torch

import mix_diag_truth as T
import mix_dmfit_truth as M


def _close(a, b, tol):
    return T.rel_err(a, b) <= tol


def test_zero_mask_and_unit_weights_are_the_complete_row_truth():
    N, D, K = 200, 7, 4
    x, r0 = T.make_data(N, D, K, 3)
    prior = T.default_prior(x, K)
    for u, v in zip(M.default_prior(x, K, np.zeros((N, D), bool), np.ones(N, np.float32)), prior):
        assert np.array_equal(u, v)
    want = T.iterate(x, r0, prior, 5)
    for miss, w in ((np.zeros((N, D), bool), None), (None, np.ones(N, np.float32)), (np.zeros((N, D), bool), np.ones(N, np.float32))):
        got = M.iterate(x, r0, prior, 5, miss, w)
        assert T.abs_err(got['r'], want['r']) < 1e-12 and _close(got['stats'], want['stats'], 1e-12)
        for u, v in zip(got['theta'], want['theta']):
            assert _close(u, v, 1e-12)
        for u, v in zip(got['bounds'], want['bounds']):
            assert abs(u - v) <= 1e-12 * max(1.0, abs(v))


def test_integer_weights_are_replicated_rows():
    N, D, K = 150, 6, 3
    x, r0, miss, w = M.make_case(N, D, K, 5, 'both')
    # the start multiplies r0 by w in fp32, as the product does: with weights in {0, 1, 2, 4} that product is exact and the two fits
    # differ by fp64 rounding alone
    w = np.where(w == 3, np.float32(4), w)
    prior = M.default_prior(x, K, miss, w)
    rep = np.repeat(np.arange(N), w.astype(np.int64))
    assert 0 < len(rep) != N
    prior_rep = M.default_prior(x[rep], K, miss[rep], None)
    for u, v in zip(prior, prior_rep):
        assert np.allclose(u, v, rtol=0, atol=1e-6)
    a = M.iterate(x, r0, prior, 6, miss, w)
    b = M.iterate(x[rep], r0[rep], prior, 6, miss[rep], None)
    assert _close(a['stats'], b['stats'], 1e-10) and T.abs_err(a['r'][rep], b['r']) < 1e-10
    for u, v in zip(a['theta'], b['theta']):
        assert _close(u, v, 1e-10)
    for u, v in zip(a['bounds'], b['bounds']):
        assert abs(u - v) <= 1e-10 * max(1.0, abs(v))
    # a row of weight 0 changes nothing, whatever it holds
    x2 = x.copy()
    x2[w == 0] = np.nan
    c = M.iterate(x2, r0, prior, 6, miss, w)
    assert torch.equal(a['stats'], c['stats']) and a['bounds'] == c['bounds']


def test_the_bound_never_falls_over_40_iterations():
    N, D, K = 400, 9, 5
    x, r0 = T.make_data(N, D, K, 17)
    rng = np.random.Generator(np.random.PCG64(99))
    miss = rng.random((N, D)) < 0.3
    miss[7, :] = True                                              # a row that observes nothing
    miss[:, 4] = rng.random(N) < 0.5                               # a column half missing
    x = np.where(miss, np.float32(np.nan), x)                      # what a missing slot holds is never read
    for w in (None, rng.integers(0, 4, N).astype(np.float32)):
        prior = M.default_prior(x, K, miss, w)
        out = M.iterate(x, r0, prior, 40, miss, w)
        b = out['bounds']
        assert len(b) == 40 and all(np.isfinite(b))
        for u, v in zip(b, b[1:]):
            assert v >= u - 1e-9 * max(1.0, abs(u)), b
        assert b[-1] > b[0]
        assert torch.isfinite(out['stats']).all() and torch.isfinite(out['fill']).all()
        assert torch.equal(out['fill'][~torch.as_tensor(miss)].float(), torch.as_tensor(x)[~torch.as_tensor(miss)])
