"""The diagonal mixture's scoring pass on the GPU (csrc/vmp_diagscore.hip, models/_diag.py, gmm.predictive_logprob_diag /
predictive_impute_diag) against the fp64 truth of tests/mix_diagscore_truth.py, evaluated on the theta read back from the device (the
pass is isolated from the fit): a shape sweep on fitted posteriors with and without a 30 % mask, row-count edges, mask patterns,
explicit large-count posteriors (the log1p case), hard data, bit identity, degenerate packs and the Python surface.

Tolerance (never a constant found on the kernel): per case and per quantity bar = max(1e-5, 3 x the error of the fp32 restatement
against fp64 on the same inputs) - absolute for resp, relative to max(1, |value|) for logp, the sum and the filled entries.  Achieved
errors and bars go to the parity log."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import mix_diag_truth as T
import mix_diagscore_truth as S
import parity_log

pytestmark = pytest.mark.gpu

# (M, D, K): D on both sides of 16 / 32 / 48 and at 64, K on both sides of 16 / 32 and at 64, M not a multiple of 4; 2051 rows are
# three blocks of 1024 with a ragged last tile (12 waves x 192 rows: the eleventh wave ends on a tile of 3 rows, the twelfth is empty)
SWEEP = [(300, 1, 2), (130, 9, 1), (257, 17, 3), (65, 5, 64), (129, 49, 5), (1031, 33, 33), (513, 64, 16), (2051, 64, 64)]


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _cuda(a):
    return torch.as_tensor(np.asarray(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(u, v):
    return (u is None and v is None) or torch.equal(_bits(u), _bits(v))


def _mask(M, D, frac, seed):
    return np.random.Generator(np.random.PCG64(seed)).random((M, D)) < frac


@functools.lru_cache(maxsize=None)
def _fitted(M, D, K):
    """theta (numpy, as read back from the device) after three iterations on 4 M rows of make_data, and M held-out rows drawn the same
    way: computed once, shared, never modified"""
    x, r0 = T.make_data(5 * M, D, K, 100 * D + 7 * K + M % 11)
    xf, xv = x[:4 * M], np.ascontiguousarray(x[4 * M:])
    loop = _mix().DiagLoop(_cuda(xf), _cuda(r0[:4 * M]))
    loop.run(3)
    return tuple(_np(t).copy() for t in loop.theta()), xv


@functools.lru_cache(maxsize=None)
def _truth(M, D, K, frac):
    theta, xv = _fitted(M, D, K)
    miss = _mask(M, D, frac, M + D) if frac else None
    return theta, xv, miss, S.bars(xv, theta, miss)


def _run(x, theta, miss=None, pack=None, **kw):
    M_ = _mix()
    pack = M_.diag_score_pack(*[_cuda(t) for t in theta]) if pack is None else pack
    kw = dict(dict(want_logp=True, want_resp=True, want_fill=miss is not None, want_sum=True), **kw)
    logp, resp, filled, total = M_.mixture_diag_score(x if torch.is_tensor(x) else _cuda(x), pack, miss=None if miss is None else _cuda(miss), **kw)
    return dict(logp=_np(logp), resp=_np(resp), filled=_np(filled), total=None if total is None else total.item())


def _check(what, truth, got, miss=None):
    bad = []
    for name, e in S.errors(got, truth, miss).items():
        bar, e32 = truth['bar_' + name], truth['e_' + name]
        parity_log.record('abs' if name == 'resp' else 'rel', e, bar, '%s %s (fp32 restatement: %.2e)' % (what, name, e32))
        print('%s %s: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, name, e, e32, bar))
        if not e <= bar:
            bad.append((name, e, bar, e32))
    assert not bad, (what, bad)


def _score_and_check(what, x, theta, miss=None, truth=None):
    truth = S.bars(x, theta, miss) if truth is None else truth
    got = _run(x, theta, miss)
    assert np.isfinite(got['logp']).all() and math.isfinite(got['total'])
    assert np.abs(got['resp'].astype(np.float64).sum(1) - 1).max() < 1e-6
    if miss is not None:
        obs = ~np.asarray(miss, bool)
        assert np.array_equal(got['filled'][obs].view(np.int32), np.asarray(x)[obs].view(np.int32))    # observed: bit for bit
    _check(what, truth, got, miss)
    return got


@pytest.mark.parametrize('frac', [0.0, 0.3])
@pytest.mark.parametrize('M,D,K', SWEEP)
def test_shape_sweep_on_fitted_posteriors(M, D, K, frac):
    theta, xv, miss, truth = _truth(M, D, K, frac)
    _score_and_check('M=%d D=%d K=%d%s' % (M, D, K, ' 30%% missing' if frac else ''), xv, theta, miss, truth)


@pytest.mark.parametrize('M', [1, 2, 63, 64, 65, 1025])
def test_row_count_edges(M):
    """one row, a wave's tile and either side of it, one row past a block's share of 1024"""
    theta, xv = _fitted(1031, 33, 33)
    x = xv[:M]
    _score_and_check('rows M=%d D=33 K=33' % M, x, theta)
    _score_and_check('rows M=%d D=33 K=33 masked' % M, x, theta, _mask(M, 33, 0.3, M))


@pytest.mark.parametrize('M,D,K', [(257, 17, 3), (513, 64, 16)])
def test_mask_patterns(M, D, K):
    theta, xv, _, plain = _truth(M, D, K, 0.0)
    what = 'M=%d D=%d K=%d ' % (M, D, K)
    w = theta[0].astype(np.float64) / theta[0].astype(np.float64).sum()
    # none missing: the masked kernel agrees with the unmasked one within the bar; x_out is x
    none = np.zeros((M, D), bool)
    got = _run(xv, theta, none)
    _check(what + 'none missing', plain, dict(got, filled=None))
    assert np.array_equal(got['filled'].view(np.int32), xv.view(np.int32))
    # all missing: logp = logsumexp log w = 0, resp = w, fills = sum_k w_k m_k
    got = _run(np.full((M, D), np.nan, np.float32), theta, ~none)
    assert np.abs(got['logp']).max() < 1e-6 and np.abs(got['resp'] - w).max() < 1e-6
    assert np.abs(got['filled'] - w @ theta[2].astype(np.float64)).max() < 1e-5 * max(1.0, np.abs(theta[2]).max())
    # one wholly missing column, one observed coordinate, the last coordinate alone
    col = none.copy()
    col[:, D // 2] = True
    one = ~none
    one[np.arange(M), np.arange(M) % D] = False
    last = none.copy()
    last[:, D - 1] = True                                                     # D = 64: bit 63 alone
    for name, miss in (('one column missing', col), ('one coordinate observed', one), ('last coordinate missing', last)):
        _score_and_check(what + name, xv, theta, miss)
    # what a missing slot holds changes no bit; in place = out of place
    miss = _mask(M, D, 0.3, 5)
    pack = _mix().diag_score_pack(*[_cuda(t) for t in theta])
    zeros = np.where(miss, np.float32(0), xv)
    junk = zeros.copy()
    junk[miss] = np.resize(np.array([np.nan, np.inf, -np.inf, 1e30], np.float32), int(miss.sum()))
    a, b = _run(zeros, theta, miss, pack=pack), _run(junk, theta, miss, pack=pack)
    for k in ('logp', 'resp', 'filled'):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert a['total'] == b['total']
    xin = _cuda(junk)
    out = _mix().mixture_diag_score(xin, pack, miss=_cuda(miss), want_fill=True, inplace=True)
    assert out[2] is xin and np.array_equal(_np(xin).view(np.int32), a['filled'].view(np.int32))


@pytest.mark.parametrize('D', [64, 7])
def test_explicit_large_count_posteriors(D):
    """N_k in {0 (the prior alone), 3, 1e4, 1e6, 1e8} in one theta: a_k up to 5e7 multiplies whatever log1p loses"""
    theta, s = S.explicit_theta([0, 3, 1e4, 1e6, 1e8], D, 40 + D)
    x = S.rows_near(theta, s, 257, 41 + D)
    _score_and_check('counts 0..1e8 D=%d' % D, x, theta)
    _score_and_check('counts 0..1e8 D=%d masked' % D, x, theta, _mask(257, D, 0.3, D))


def test_hard_data():
    """columns scaled from 1e-3 to 1e3, all data offset by +1000, and one row 40 sd from every component"""
    M, D, K = 257, 17, 3
    theta, xv = _fitted(M, D, K)
    scale = np.logspace(-3, 3, D).astype(np.float32)
    for name, f in (('scaled columns', lambda x: (x * scale).astype(np.float32)), ('offset +1000', lambda x: (x + 1000).astype(np.float32))):
        x, r0 = T.make_data(5 * M, D, K, 7)
        x = f(x)
        loop = _mix().DiagLoop(_cuda(x[:4 * M]), _cuda(r0[:4 * M]))
        loop.run(3)
        th = tuple(_np(t).copy() for t in loop.theta())
        _score_and_check('hard data, ' + name, np.ascontiguousarray(x[4 * M:]), th)
        _score_and_check('hard data, ' + name + ', masked', np.ascontiguousarray(x[4 * M:]), th, _mask(M, D, 0.3, 3))
    sd = np.sqrt(theta[4].astype(np.float64) / theta[3].astype(np.float64)[:, None]).max(0)
    far = (theta[2].max(0) + 40 * sd * 3)[None, :].astype(np.float32)
    got = _run(np.concatenate([xv[:3], far]), theta)
    assert np.isfinite(got['logp']).all() and np.isfinite(got['resp']).all() and abs(got['resp'][3].sum() - 1) < 1e-6
    _check('one row 40 sd away', S.bars(np.concatenate([xv[:3], far]), theta), got)


@pytest.mark.parametrize('M,D,K', [(1031, 33, 33), (513, 64, 16)])
def test_determinism(M, D, K):
    M_ = _mix()
    theta, xv = _fitted(M, D, K)
    pack = M_.diag_score_pack(*[_cuda(t) for t in theta])
    x, miss = _cuda(xv), _cuda(_mask(M, D, 0.3, 9))
    sets = 0
    for mk in (None, miss):
        full = M_.mixture_diag_score(x, pack, miss=mk, want_resp=True, want_fill=mk is not None, want_sum=True)
        again = M_.mixture_diag_score(x, pack, miss=mk, want_resp=True, want_fill=mk is not None, want_sum=True)
        assert all(_same(u, v) for u, v in zip(full, again))
        for wl, wr, wf, ws in itertools.product((False, True), repeat=4):
            if not (wl or wr or wf or ws) or (wf and mk is None):
                continue
            sets += 1
            part = M_.mixture_diag_score(x, pack, miss=mk, want_logp=wl, want_resp=wr, want_fill=wf, want_sum=ws)
            for want, u, v in zip((wl, wr, wf, ws), part, full):
                assert (u is None) == (not want) and (u is None or _same(u, v)), (wl, wr, wf, ws)
        # x as a view that starts one float off the allocation's alignment
        buf = torch.empty(M * D + 1, dtype=torch.float32, device='cuda')
        off = buf[1:].view(M, D)
        off.copy_(x)
        assert off.data_ptr() % 8 == 4
        moved = M_.mixture_diag_score(off, pack, miss=mk, want_resp=True, want_fill=mk is not None, want_sum=True)
        assert all(_same(u, v) for u, v in zip(full, moved))
    assert sets == 7 + 15                       # the non-empty subsets of {logp, resp, sum}, and of {logp, resp, fill, sum} with a mask


def test_degenerate_packs():
    M_ = _mix()
    theta, s = S.explicit_theta([5, 50, 500], 4, 9)
    x = _cuda(S.rows_near(theta, s, 70, 10))
    theta[4][1, 2] = 0                                                        # b[1,2] = 0
    pack = M_.diag_score_pack(*[_cuda(t) for t in theta])
    p = _np(pack)
    assert np.isnan(p[1]).all() and np.isfinite(p[[0, 2]]).all()
    logp, _, _, total = M_.mixture_diag_score(x, pack, want_sum=True)
    assert torch.isnan(logp).all() and math.isnan(total.item())
    logp = M_.mixture_diag_score(x, pack, miss=torch.ones(70, 4, dtype=torch.bool, device='cuda'))[0]
    assert torch.isnan(logp).all()                                            # nothing observed: the NaN row still reaches every row
    theta[4][1, 2] = 1
    theta[0][2] = 0                                                           # alpha_2 = 0: refused by the same rule
    p = _np(M_.diag_score_pack(*[_cuda(t) for t in theta]))
    assert np.isnan(p[2]).all() and np.isfinite(p[[0, 1]]).all()
    theta[0][2] = 1
    # the pack against the truth's, word for word (fp64 inside, rounded once)
    p = _np(M_.diag_score_pack(*[_cuda(t) for t in theta])).astype(np.float64)
    want = S.pack_array(S.pack(theta))
    assert (np.abs(p - want) / np.maximum(1.0, np.abs(want))).max() < 1.2e-7
    # log w = -inf through a hand-written pack: resp_k = 0; every log w = -inf: logp = -inf, resp = 0, fills 0, no NaN
    D = 4
    hand = want.astype(np.float32)
    hand[1, 3 * D] = hand[1, 3 * D + 2] = -np.inf
    miss = torch.zeros(70, D, dtype=torch.bool, device='cuda')
    miss[:, 1] = True
    for mk in (None, miss):
        logp, resp, filled, _ = M_.mixture_diag_score(x, _cuda(hand), miss=mk, want_resp=True, want_fill=mk is not None)
        assert torch.isfinite(logp).all() and (resp[:, 1] == 0).all() and ((resp.sum(1) - 1).abs() < 1e-6).all()
    hand[:, 3 * D] = hand[:, 3 * D + 2] = -np.inf
    for mk in (None, miss):
        logp, resp, filled, total = M_.mixture_diag_score(x, _cuda(hand), miss=mk, want_resp=True, want_fill=mk is not None, want_sum=True)
        assert (logp == -math.inf).all() and (resp == 0).all() and total.item() == -math.inf
        if mk is not None:
            assert (filled[:, 1] == 0).all() and torch.equal(filled[:, 0], x[:, 0])


def test_surface():
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import gmm
    M_ = _mix()
    x, r0 = T.make_data(800, 24, 4, 21)
    xf, xv = _cuda(x[:600]), _cuda(np.ascontiguousarray(x[600:]))
    miss = _cuda(_mask(200, 24, 0.3, 2))
    loop = M_.DiagLoop(xf, _cuda(r0[:600]))
    with pytest.raises(L.VmpError, match='at least one iteration'):
        loop.heldout(xv)
    loop.run(2)
    th = loop.theta()
    logp, resp = loop.heldout_logprob(xv, want_resp=True)
    assert _same(logp, gmm.predictive_logprob_diag(xv, *th)) and _same(logp, loop.heldout_logprob(xv))
    assert _same(loop.heldout_logprob(xv, miss), gmm.predictive_logprob_diag(xv, *th, miss=miss))
    xo, lp = loop.fill(xv, miss)
    xg, lg = gmm.predictive_impute_diag(xv, miss, *th)
    assert _same(xo, xg) and _same(lp, lg) and resp.shape == (200, 4)
    total = M_.mixture_diag_score(xv, loop.predictive_pack(), want_logp=False, want_sum=True)[3]
    assert loop.heldout(xv) == total.item() / 200
    assert abs(loop.heldout(xv) - logp.double().mean().item()) < 1e-6 * max(1.0, abs(loop.heldout(xv)))
    # run_until: the stopping rule and the return value of VMPLoop.run_until
    tol, every, most = 1e-3, 2, 40
    start = loop.iterations
    hist = loop.run_until(xv, tol, check_every=every, max_iterations=most)
    assert hist[-1][0] == loop.iterations and [h[0] for h in hist] == [start + every * (i + 1) for i in range(len(hist))]
    gains = [b[1] - a[1] for a, b in zip(hist, hist[1:])]
    assert all(g >= tol for g in gains[:-1])
    assert (len(hist) > 1 and gains[-1] < tol) or loop.iterations - start == most
    assert all(math.isfinite(h[1]) for h in hist)
    for name in ('score', 'impute', 'sample'):
        with pytest.raises(L.VmpError, match='not built'):
            getattr(loop, name)(xv)
