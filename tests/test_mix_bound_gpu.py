"""The variational lower bound of the Gaussian-mixture fit on the GPU (csrc/vmp_bound.hip, _mix.mixture_bound / bound_terms /
lower_bound, VMPLoop.lower_bound / run_until_bound, gmm.lower_bound) against the fp64 truth of tests/mix_bound_truth.py.

Tolerance (never a constant found on the kernel): per case bar = max(1e-5, 3 x the error of the fp32 restatement against the fp64
truth), relative to max(1, |value|), for the data term, the whole bound and the per-row log-sum-exp; the K-sized terms are fp64 in
the kernel and are held to 1e-5 relative to max(1, |value|) against the truth on the same fp32-rounded theta.  In the loop tests
the restatement runs the whole iteration in fp32 (mix_bound_truth.sequence).  Achieved errors and bars go to the parity log.

The streaming kernel has no form that is entered only above some N: a wave walks its range four rows at a time, whatever the range.
Masks have about 25 % missing; row 0 is fully missing and row 1 fully observed; the missing slots of x hold NaN."""
import functools
import math

import numpy as np
import pytest
import torch

import mix_bound_truth as B
import mix_missfit_truth as T
import parity_log

pytestmark = pytest.mark.gpu

SWEEP = [(257, 8, 3), (65, 3, 17), (4099, 2, 16), (513, 5, 33), (300, 1, 2), (2051, 8, 64)]


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _gmm():
    import vmp_for_svae_amd as V
    return V._lib.VMP_GMM


def _cuda(a):
    return None if a is None else torch.as_tensor(a).cuda()


@functools.lru_cache(maxsize=None)
def _case(N, D, K, masked):
    """inputs, theta (the truth's after one iteration, rounded to fp32) and the truth with its bars: computed once, shared, never
    modified.  masked=False: the same rows, complete (NaN-free), and no mask."""
    x, r0, miss = T.make_data(N, D, K, seed=100 * D + 7 * K + N % 11)
    if not masked:
        rng = np.random.Generator(np.random.PCG64(N + D + K))
        x = np.where(miss != 0, rng.standard_normal((N, D)).astype(np.float32), x)
        miss = None
    theta = tuple(t.float() for t in B.theta_after(x, miss, r0, 1))
    return x, miss, theta, B.case(x, miss, theta)


def _report(kind, what, err, bar, e32=None):
    parity_log.record(kind, err, bar, what if e32 is None else '%s (fp32 restatement: %.2e)' % (what, e32))
    print('%s: kernel %.3e  %sbar %.3e' % (what, err, '' if e32 is None else 'fp32 restatement %.3e  ' % e32, bar))
    return err <= bar


def _check_pass(what, truth, data=None, lse=None, bound=None, terms=None):
    bad = []
    for name, got in (('data', data), ('bound', bound)):
        if got is not None:
            assert math.isfinite(float(got)), (what, name, float(got))
            if not _report('rel', '%s %s' % (what, name), B.rel(got, truth[name]), truth['bar_' + name], truth['e_' + name]):
                bad.append(name)
    if lse is not None:
        assert torch.isfinite(lse).all(), what
        if not _report('rel', '%s lse' % what, T.rel_err(lse, truth['lse']), truth['bar_lse'], truth['e_lse']):
            bad.append('lse')
    if terms is not None:
        terms = terms.cpu()
        assert torch.isfinite(terms).all(), what
        K = truth['kl_nw'].shape[0]
        assert terms.shape == (2 + K,)
        for name, got, want in (('kl_pi', terms[0], truth['kl_pi']), ('sum kl_nw', terms[1], truth['kl_nw'].sum().item())):
            if not _report('rel', '%s %s' % (what, name), B.rel(got, want), B.FLOOR):
                bad.append(name)
        if not _report('rel', '%s kl_nw' % what, T.rel_err(terms[2:], truth['kl_nw']), B.FLOOR):
            bad.append('kl_nw')
    assert not bad, (what, bad)


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
@pytest.mark.parametrize('N,D,K', SWEEP)
def test_pass_and_terms_against_the_truth(N, D, K, masked):
    M = _mix()
    x, miss, theta, truth = _case(N, D, K, masked)
    if masked:
        assert 0.15 < miss.mean() < 0.35 and miss[0].all() and not miss[1].any() and np.isnan(x[miss != 0]).all()
    else:
        assert np.isfinite(x).all()
    xd, md, th = _cuda(x), _cuda(miss), tuple(_cuda(t) for t in theta)
    data, lse = M.mixture_bound(xd, md, M.fit_pack(*th), want_rows=True)
    assert data.shape == () and data.dtype == torch.float64 and lse.shape == (N,) and lse.dtype == torch.float32
    terms = M.bound_terms(M.default_prior(K, D, 'cuda'), th)
    bound = M.lower_bound(xd, th, miss=md)
    assert bound.shape == () and bound.dtype == torch.float64 and bound.is_cuda
    what = 'N=%d D=%d K=%d %s' % (N, D, K, 'masked' if masked else 'complete')
    _check_pass(what, truth, data=data.item(), lse=lse, bound=bound.item(), terms=terms)
    assert bound.item() == (data - (terms[0] + terms[1])).item()


def test_terms_with_a_prior_of_their_own():
    M = _mix()
    N, D, K = 513, 5, 33
    x, miss, theta, _ = _case(N, D, K, True)
    rng = np.random.Generator(np.random.PCG64(3))
    A = rng.standard_normal((K, D, D))
    prior = tuple(torch.as_tensor(np.asarray(a, np.float32)) for a in (
        rng.random(K) + 0.1, rng.random(K) + 0.2, rng.standard_normal((K, D)), A @ A.transpose(0, 2, 1) + np.eye(D), rng.random(K) * 3 + D))
    truth = B.case(x, miss, theta, prior)
    th = tuple(_cuda(t) for t in theta)
    terms = M.bound_terms(tuple(_cuda(p) for p in prior), th)
    bound = M.lower_bound(_cuda(x), th, prior=tuple(_cuda(p) for p in prior), miss=_cuda(miss))
    _check_pass('own prior N=%d D=%d K=%d' % (N, D, K), truth, bound=bound.item(), terms=terms)


@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (513, 5, 33)])
def test_all_observed_mask_agrees_with_no_mask(N, D, K):
    """two kernels - one factors an identity, one factors nothing: equal within the bar, not bit for bit"""
    M = _mix()
    x, _, theta, truth = _case(N, D, K, False)
    xd, th = _cuda(x), tuple(_cuda(t) for t in theta)
    pack = M.fit_pack(*th)
    d0, l0 = M.mixture_bound(xd, None, pack, want_rows=True)
    d1, l1 = M.mixture_bound(xd, torch.zeros(N, D, dtype=torch.uint8, device='cuda'), pack, want_rows=True)
    what = 'all observed N=%d D=%d K=%d' % (N, D, K)
    _check_pass(what + ' zero mask', truth, data=d1.item(), lse=l1)
    assert _report('rel', what + ' data vs no mask', B.rel(d1.item(), d0.item()), truth['bar_data'])
    assert _report('rel', what + ' lse vs no mask', T.rel_err(l1, l0.double().cpu()), truth['bar_lse'])


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (513, 5, 33), (4099, 2, 16)])
def test_bit_identity_across_runs_and_optional_outputs(N, D, K, masked):
    M = _mix()
    x, miss, theta, _ = _case(N, D, K, masked)
    xd, md, th = _cuda(x), _cuda(miss), tuple(_cuda(t) for t in theta)
    pack = M.fit_pack(*th)
    d0, l0 = M.mixture_bound(xd, md, pack, want_rows=True)
    d1, l1 = M.mixture_bound(xd, md, pack, want_rows=True)
    d2, l2 = M.mixture_bound(xd, md, pack)
    assert l2 is None
    assert torch.equal(d0.view(torch.int64), d1.view(torch.int64)) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    assert torch.equal(d0.view(torch.int64), d2.view(torch.int64))
    t0, t1 = M.bound_terms(M.default_prior(K, D, 'cuda'), th), M.bound_terms(M.default_prior(K, D, 'cuda'), th)
    assert torch.equal(t0.view(torch.int64), t1.view(torch.int64))
    if masked:                                                                  # a bool mask is the same mask
        d3, _ = M.mixture_bound(xd, md != 0, pack)
        assert torch.equal(d0.view(torch.int64), d3.view(torch.int64))


@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (513, 5, 33)])
def test_nan_and_inf_in_the_missing_slots_change_nothing(N, D, K):
    M = _mix()
    x, miss, theta, _ = _case(N, D, K, True)
    md, th = _cuda(miss), tuple(_cuda(t) for t in theta)
    pack = M.fit_pack(*th)
    outs = []
    for fill in (0.0, math.nan, math.inf, -math.inf):
        xf = x.copy()
        xf[miss != 0] = fill
        d, l = M.mixture_bound(_cuda(xf), md, pack, want_rows=True)
        assert torch.isfinite(d) and torch.isfinite(l).all()
        outs.append((d, l))
    for d, l in outs[1:]:
        assert torch.equal(d.view(torch.int64), outs[0][0].view(torch.int64)) and torch.equal(l.view(torch.int32), outs[0][1].view(torch.int32))


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (65, 3, 17), (4099, 2, 16)])
def test_unaligned_x_is_within_the_bar(N, D, K, masked):
    """a view offset by one float: the scalar load path against the truth"""
    M = _mix()
    x, miss, theta, truth = _case(N, D, K, masked)
    xa = _cuda(x)
    buf = torch.empty(N * D + 4, dtype=torch.float32, device='cuda')
    xu = buf[1:1 + N * D].view(N, D)
    xu.copy_(xa)
    assert xa.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    d, l = M.mixture_bound(xu, _cuda(miss), M.fit_pack(*(_cuda(t) for t in theta)), want_rows=True)
    _check_pass('unaligned N=%d D=%d K=%d %s' % (N, D, K, 'masked' if masked else 'complete'), truth, data=d.item(), lse=l)


def test_a_row_without_mass_and_a_nan_pack():
    """every term of a row -inf: the row, and with it the sum, is -inf; a NaN pack gives NaN"""
    M = _mix()
    N, D, K = 65, 3, 17
    x, miss, theta, _ = _case(N, D, K, True)
    xd, md = _cuda(x), _cuda(miss)
    pack = M.fit_pack(*(_cuda(t) for t in theta))
    gone = pack.clone()
    gone[:, -1] = -math.inf
    for m in (md, None):
        xx = xd if m is not None else torch.nan_to_num(xd)
        d, l = M.mixture_bound(xx, m, gone, want_rows=True)
        assert d.item() == -math.inf and (l == -math.inf).all()
        bad = pack.clone()
        bad[5] = math.nan
        d, l = M.mixture_bound(xx, m, bad, want_rows=True)
        assert math.isnan(d.item()) and torch.isnan(l).all()


# ---- the loop --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_case(N, D, K, frac):
    x, r0, miss = B.loop_input(N, D, K, frac)
    return x, r0, miss, B.sequence(x, miss, r0, 5)


def _loop(x, r0, miss, **kw):
    return _mix().VMPLoop(_cuda(x), _cuda(r0), _gmm(), miss=_cuda(miss), **kw)


@pytest.mark.parametrize('N,D,K,frac', B.LOOP_INPUTS)
def test_loop_lower_bound_follows_the_truth(N, D, K, frac):
    from vmp_for_svae_amd.models import gmm
    x, r0, miss, seq = _loop_case(N, D, K, frac)
    loop = _loop(x, r0, miss)
    assert (loop.miss is None) == (frac == 0)
    got, bad = [], []
    for it, s in enumerate(seq, 1):
        loop.step()
        b = loop.lower_bound()
        assert isinstance(b, float) and math.isfinite(b)
        got.append(b)
        if not _report('rel', 'loop N=%d D=%d K=%d iteration %d' % (N, D, K, it), B.rel(b, s['bound']), s['bar'], s['e']):
            bad.append(it)
        again = gmm.lower_bound(loop.x, *loop.theta(), miss=loop.miss, prior=loop.prior)
        assert again.item() == b                                                # the same launches on the same operands: the same bits
    assert not bad, bad
    for i in range(1, len(seq)):
        gain = seq[i]['bound'] - seq[i - 1]['bound']
        tol = 2 * max(seq[i]['bar'] * max(1.0, abs(seq[i]['bound'])), seq[i - 1]['bar'] * max(1.0, abs(seq[i - 1]['bound'])))
        if gain > tol:
            assert got[i] >= got[i - 1], (i, got, gain, tol)
    assert loop.iterations == 5


def test_accurate_loop_has_a_bound():
    N, D, K, frac = B.LOOP_INPUTS[3]
    x, r0, miss, seq = _loop_case(N, D, K, frac)
    loop = _loop(x, r0, None, accurate=True)
    loop.run(5)
    b = loop.lower_bound()
    assert _report('rel', 'accurate loop N=%d D=%d K=%d iteration 5' % (N, D, K), B.rel(b, seq[4]['bound']), seq[4]['bar'], seq[4]['e'])


def test_run_until_bound():
    N, D, K, frac = B.LOOP_INPUTS[0]
    x, r0, miss, _ = _loop_case(N, D, K, frac)
    loop = _loop(x, r0, miss)
    hist = loop.run_until_bound(1e30, check_every=3)                            # any gain is below this: stops at the second check
    assert [h[0] for h in hist] == [3, 6] and loop.iterations == 6
    loop = _loop(x, r0, miss)
    hist = loop.run_until_bound(1e-7, check_every=5, max_iterations=1000)
    assert 2 <= len(hist) < 200 and hist[-1][0] == loop.iterations == 5 * len(hist)
    gain = hist[-1][1] - hist[-2][1]
    assert gain < 1e-7 * max(1.0, abs(hist[-1][1]))
    assert all(b1 - b0 >= 1e-7 * max(1.0, abs(b1)) for (_, b0), (_, b1) in zip(hist[:-2], hist[1:-1]))
    second = _loop(x, r0, miss)
    for it, b in hist[:4]:
        second.run(it - second.iterations)
        assert second.iterations == it and second.lower_bound() == b
    # max_iterations ends the call, and the count carries on from the loop's own
    more = loop.run_until_bound(0.0, check_every=2, max_iterations=3)
    assert [h[0] for h in more] == [hist[-1][0] + 2, hist[-1][0] + 3] and loop.iterations == hist[-1][0] + 3


def test_refusals_that_need_a_device():
    import vmp_for_svae_amd as V
    E = V._lib.VmpError
    N, D, K, frac = B.LOOP_INPUTS[0]
    x, r0, miss, _ = _loop_case(N, D, K, frac)
    loop = _loop(x, r0, miss)
    with pytest.raises(E, match='at least one iteration'):
        loop.lower_bound()
    smm = _mix().VMPLoop(_cuda(np.nan_to_num(x)), _cuda(r0), V._lib.VMP_SMM, kappa=torch.full((K,), 5.0))
    with pytest.raises(E, match='Gaussian mixture'):
        smm.lower_bound()
    with pytest.raises(E, match='Gaussian mixture'):
        smm.run_until_bound(1e-6)
    assert smm.iterations == 0                                                  # refused before anything ran
