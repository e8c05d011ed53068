"""The fp64 truth of the weighted Gaussian-mixture fit (tests/mix_wfit_truth.py) checked against itself, without a GPU: a weight w_n
makes row n count as w_n identical rows, so integer weights must reproduce mix_missfit_truth on the replicated rows; unit weights
are mix_missfit_truth itself; zero weights are the fit on the subset; and the weighted bound does not fall."""
import numpy as np
import pytest
import torch

import mix_missfit_truth as T
import mix_wfit_truth as W

RTOL = 1e-9


def _close(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    e = ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()
    assert e <= RTOL, (what, e)


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
@pytest.mark.parametrize('N,D,K', [(61, 3, 4), (40, 1, 2), (37, 5, 3)])
def test_integer_weights_are_replicated_rows(N, D, K, masked):
    x, r0, miss, w = W.make_data(N, D, K, 11 * N + D, masked, integer=True)
    assert w[2] == 0 and np.isnan(x[2, 0]) and (miss is None or miss[2, 0] == 0)
    rep = np.repeat(np.arange(N), w.astype(np.int64))
    assert len(rep) == int(w.sum()) and 2 not in rep
    mrep = np.zeros((len(rep), D), np.uint8) if miss is None else miss[rep]
    for its in (1, 2, 3):
        a = W.iterate(x, miss, w, r0, its)
        b = T.iterate(x[rep], mrep, r0[rep], its)
        what = 'N=%d D=%d K=%d its=%d' % (N, D, K, its)
        _close(a['r'][rep], b['r'], what + ' r')
        _close(a['x_fill'][rep], b['x_fill'], what + ' x_fill')
        _close(a['stats'], b['stats'], what + ' stats')
        for u, v, n in zip(a['theta'], b['theta'], 'alpha beta m C v'.split()):
            _close(u, v, what + ' ' + n)
        _close(W.lower_bound(x, miss, w, a['theta']), T.lower_bound(x[rep], mrep, b['theta']), what + ' bound')
        _close(a['data'] - W.kl_terms(a['theta']), T.lower_bound(x[rep], mrep, b['theta']), what + ' data - kl')


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
def test_unit_weights_are_the_unweighted_truth(masked):
    N, D, K = 53, 4, 3
    x, r0, miss, _ = W.make_data(N, D, K, 5, masked)
    x[2, 0] = 0.5                                 # every row counts here: the NaN of row 2 has to go
    w = np.ones(N, np.float32)
    mk = W._mask(x, miss)
    a = W.iterate(x, miss, w, r0, 3)
    b = T.iterate(x, mk, r0, 3)
    for name in ('r', 'logr', 'x_fill', 'stats'):
        _close(a[name], b[name], name)
    for u, v in zip(a['theta'], b['theta']):
        _close(u, v, 'theta')
    _close(W.lower_bound(x, miss, w, a['theta']), T.lower_bound(x, mk, b['theta']), 'bound')


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
def test_zero_weights_are_the_fit_on_the_subset(masked):
    N, D, K = 67, 3, 4
    x, r0, miss, w = W.make_data(N, D, K, 9, masked)
    w = (w > 0).astype(np.float32)
    sub = np.nonzero(w)[0]
    assert 0 < len(sub) < N and 2 not in sub
    msub = np.zeros((len(sub), D), np.uint8) if miss is None else miss[sub]
    a = W.iterate(x, miss, w, r0, 3)
    b = T.iterate(x[sub], msub, r0[sub], 3)
    _close(a['r'][sub], b['r'], 'r')
    _close(a['stats'], b['stats'], 'stats')
    for u, v in zip(a['theta'], b['theta']):
        _close(u, v, 'theta')
    _close(W.lower_bound(x, miss, w, a['theta']), T.lower_bound(x[sub], msub, b['theta']), 'bound')
    assert torch.isfinite(a['stats']).all()
    # the held-out rows still get the E-step's responsibilities; the one holding NaN in an observed slot gets NaN
    held = np.setdiff1d(np.arange(N), np.append(sub, 2))
    assert torch.isfinite(a['r'][held]).all() and ((a['r'][held].sum(1) - 1).abs() < 1e-12).all()
    assert torch.isnan(a['r'][2]).all()


@pytest.mark.parametrize('N,D,K,seed,masked', [(120, 2, 3, 1, False), (90, 3, 4, 2, True)])
def test_weighted_bound_does_not_fall(N, D, K, seed, masked):
    x, r0, miss, w = W.make_data(N, D, K, seed, masked)
    prior = T.default_prior(K, D)
    mk = W._mask(x, miss)
    out = dict(stats=W.seed_stats(x, mk, w, r0))
    hist = []
    for _ in range(10):
        out = W.one_iteration(x, mk, w, out['stats'], prior)
        hist.append(out['data'] - W.kl_terms(out['theta'], prior))
    assert all(np.isfinite(hist))
    for a, b in zip(hist, hist[1:]):
        assert b >= a - 1e-9 * abs(a), hist


def test_bars_report_every_quantity():
    x, r0, miss, w = W.make_data(45, 3, 3, 4, True)
    t = W.bars(x, miss, w, r0, 2)
    for name in ('r', 'logr', 'x_fill', 'stats', 'alpha', 'beta', 'm', 'C', 'v', 'data', 'bound'):
        assert 0 <= t['e_' + name] < 1e-3 and t['bar_' + name] == max(1e-5, 3 * t['e_' + name]), name
    assert not W.finite_rows(t)[2] and W.finite_rows(t).sum() == 44
