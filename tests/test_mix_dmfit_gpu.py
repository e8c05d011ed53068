"""The diagonal mixture fit on partly observed and weighted rows on the GPU (csrc/vmp_diagmfit.hip, models/_diag.py DiagFitLoop,
gmm.inference_diag_missing / inference_diag_weighted / lower_bound_diag) against the fp64 truth of tests/mix_dmfit_truth.py: the pass
and the loop over a shape sweep (D on both sides of 16 / 32 / 48 and at 64, K on both sides of 16 / 32 and at 64, N below and above a
wave's flush interval of 128 rows and above one block) in three modes (mask only, weights only, both), the same with all data offset by
+1000, dead entries that hold NaN, bit identity, iterate against steps, unaligned x, the monotone bound, the complete-row limit and the
scoring surface after a masked fit.

Mask: 30 % missing at random plus one all-missing row and one all-missing column.  Weights: integers 0..3 with at least one 0.
Tolerance (never a constant found on the kernel), the rule of tests/test_mix_diag_gpu.py: per case and per quantity bar = max(1e-5,
3 x the error of the same functions run in fp32 against fp64, from the same inputs for the same number of iterations) - absolute for r,
relative to max(1, |value|) for everything else.  Achieved errors and bars go to the parity log."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import mix_diag_truth as T
import mix_dmfit_truth as M
import parity_log

pytestmark = pytest.mark.gpu


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _cuda(a):
    return None if a is None else torch.as_tensor(np.asarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _data(N, D, K, mode, offset=0.0):
    x, r0, miss, w = M.make_case(N, D, K, 100 * D + 7 * K + N % 11, mode, offset)
    return x, r0, miss, w, M.default_prior(x, K, miss, w)


@functools.lru_cache(maxsize=None)
def _case(N, D, K, mode, iterations, offset=0.0):
    """inputs and the truth with its bars: computed once, shared, never modified"""
    x, r0, miss, w, prior = _data(N, D, K, mode, offset)
    return x, r0, miss, w, prior, M.bars(x, r0, prior, iterations, miss, w)


def _loop(x, r0, miss, w, prior):
    return _mix().DiagFitLoop(_cuda(x), _cuda(r0), miss=_cuda(miss), weights=_cuda(w), prior=[_cuda(p) for p in prior])


def _state(loop):
    return dict(r=loop.r, logr=loop.logr, stats=loop.stats, theta=loop.theta(), data=loop._data.item(), bound=loop.lower_bound(),
                fill=loop.filled() if loop.miss is not None else None)


def _check(what, truth, got):
    bad = []
    for name, e in M.errors(got, truth).items():
        bar, e32 = truth['bar_' + name], truth['e_' + name]
        parity_log.record('abs' if name == 'r' else 'rel', e, bar, '%s %s (fp32 restatement: %.2e)' % (what, name, e32))
        print('%s %s: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, name, e, e32, bar))
        if not e <= bar:
            bad.append((name, e, bar, e32))
    assert not bad, (what, bad)


def _bits(t):
    return None if t is None else t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(u, v):
    return (u is None and v is None) or torch.equal(_bits(u), _bits(v))


def _one_and_three(N, D, K, mode, offset=0.0):
    x, r0, miss, w, prior, truth1 = _case(N, D, K, mode, 1, offset)
    truth3 = _case(N, D, K, mode, 3, offset)[5]
    what = 'N=%d D=%d K=%d %s%s' % (N, D, K, mode, ' offset %g' % offset if offset else '')
    loop = _loop(x, r0, miss, w, prior)
    r = loop.step(want_logr=True)
    assert r.shape == (N, K) and (r.double().sum(1) - 1).abs().max().item() < 1e-6
    st = _state(loop)
    assert torch.isfinite(st['stats']).all() and math.isfinite(st['data']) and math.isfinite(st['bound'])
    _check('1 iteration ' + what, truth1, st)
    if miss is not None:                                                     # observed entries bit for bit
        obs = ~_cuda(miss)
        assert torch.equal(_bits(st['fill'])[obs], _bits(loop.x)[obs])
    if w is not None:                                                        # a row of weight 0 still gets its r
        dead = _cuda(w) == 0
        assert dead.any() and (r[dead].double().sum(1) - 1).abs().max().item() < 1e-6
    # the pass through its wrapper is the loop's own pass
    got = _mix().mixture_diag_mfit_pass(loop.x, loop.pack, miss=loop.miss, weights=loop.weights, want_logr=True, want_fill=miss is not None,
                                        want_bound=True)
    for u, v in zip(got, (loop.r, loop.logr, st['fill'], loop.stats, loop._data)):
        assert _same(u, v)
    loop.run(2)
    assert loop.iterations == 3
    _check('3 iterations ' + what, truth3, _state(loop))


@pytest.mark.parametrize('mode', M.MODES)
@pytest.mark.parametrize('N,D,K', M.SHAPES)
def test_pass_and_three_iterations_shape_sweep(N, D, K, mode):
    _one_and_three(N, D, K, mode)


@pytest.mark.parametrize('mode', M.MODES)
def test_data_offset_by_1000(mode):
    _one_and_three(1031, 33, 33, mode, 1000.0)


@pytest.mark.parametrize('N,D,K', [(1031, 33, 33), (513, 64, 16)])
def test_dead_entries_may_hold_nan(N, D, K):
    """NaN in every missing slot and in every row of weight 0: no bit of stats or data changes, nor of the other rows' outputs"""
    x, r0, miss, w, prior = _data(N, D, K, 'both')
    a = _loop(x, r0, miss, w, prior)
    xn = np.where(miss, np.float32(np.nan), x)
    xn[w == 0] = np.nan
    b = _loop(xn, r0, miss, w, prior)
    for u, v in zip(a.prior, b.prior):
        assert torch.equal(u, v)
    assert _same(a._stats, b._stats)
    live = _cuda(w) > 0
    for loops in ((a, b),):
        for lp in loops:
            lp.step(want_logr=True)
        assert _same(a._stats, b._stats) and _same(a._data, b._data) and torch.isfinite(b._stats).all() and torch.isfinite(b._data)
        assert _same(a.r[live], b.r[live]) and _same(a.logr[live], b.logr[live]) and _same(a.filled()[live], b.filled()[live])
        for lp in loops:
            lp.run(2)
        assert _same(a._stats, b._stats) and _same(a._data, b._data) and a.lower_bound() == b.lower_bound()
        for u, v in zip(a.theta(), b.theta()):
            assert torch.equal(u, v)
    # the mask-only form: NaN in the missing slots alone
    x, r0, miss, w, prior = _data(N, D, K, 'mask')
    a, b = _loop(x, r0, miss, None, prior), _loop(np.where(miss, np.float32(np.nan), x), r0, miss, None, prior)
    a.run(2)
    b.run(2)
    assert _same(a._stats, b._stats) and _same(a._data, b._data) and _same(a.r, b.r) and _same(a.filled(), b.filled())


@pytest.mark.parametrize('mode', M.MODES)
@pytest.mark.parametrize('N,D,K', [(1031, 33, 33), (513, 64, 16)])
def test_bit_identity_across_runs_and_every_output_set(N, D, K, mode):
    Mx = _mix()
    x, r0, miss, w, prior = _data(N, D, K, mode)
    loop = _loop(x, r0, miss, w, prior)
    loop.step()
    masked = miss is not None
    kw = dict(miss=loop.miss, weights=loop.weights)
    full = Mx.mixture_diag_mfit_pass(loop.x, loop.pack, want_r=True, want_logr=True, want_fill=masked, want_stats=True, want_bound=True, **kw)
    assert torch.isfinite(full[3]).all() and torch.isfinite(full[4])
    again = Mx.mixture_diag_mfit_pass(loop.x, loop.pack, want_r=True, want_logr=True, want_fill=masked, want_stats=True, want_bound=True, **kw)
    for u, v in zip(full, again):
        assert _same(u, v)
    sets = 0
    for want in itertools.product((False, True), repeat=5):
        want_r, want_logr, want_fill, want_stats, want_bound = want
        if not any(want) or (want_logr and not want_r) or (want_fill and not masked):
            continue
        part = Mx.mixture_diag_mfit_pass(loop.x, loop.pack, want_r=want_r, want_logr=want_logr, want_fill=want_fill, want_stats=want_stats,
                                         want_bound=want_bound, **kw)
        for asked, u, v in zip(want, part, full):
            assert (u is None) if not asked else _same(u, v), want
        sets += 1
    assert sets == (23 if masked else 11)


@pytest.mark.parametrize('mode', M.MODES)
@pytest.mark.parametrize('N,D,K', [(4099, 16, 16), (513, 64, 16), (1031, 33, 33)])
def test_iterate_3_is_three_steps(N, D, K, mode):
    x, r0, miss, w, prior = _data(N, D, K, mode)
    a, b = _loop(x, r0, miss, w, prior), _loop(x, r0, miss, w, prior)
    a.run(3)
    for _ in range(3):
        b.step(want_logr=True)
    assert a.iterations == b.iterations == 3
    assert _same(a.stats, b.stats) and _same(a._data, b._data)
    for u, v in zip(a.theta() + a.aux(), b.theta() + b.aux()):
        assert torch.equal(u, v)
    assert a.lower_bound() == b.lower_bound()
    assert torch.equal(a.r, b.r) and torch.equal(a.logr, b.logr)          # produced by one pass on demand
    if miss is not None:
        assert _same(a.filled(), b.filled())


@pytest.mark.parametrize('mode', M.MODES)
@pytest.mark.parametrize('N,D,K', [(257, 17, 3), (513, 64, 16), (65, 5, 64)])
def test_unaligned_x_gives_the_same_bits(N, D, K, mode):
    """x a view offset by one float: not 16-byte aligned"""
    x, r0, miss, w, prior = _data(N, D, K, mode)
    a = _loop(x, r0, miss, w, prior)
    a.run(2)
    buf = torch.empty(N * D + 8, dtype=torch.float32, device='cuda')
    xu = buf[1:1 + N * D].view(N, D)
    xu.copy_(_cuda(x))
    assert a.x.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    b = _mix().DiagFitLoop(xu, _cuda(r0), miss=_cuda(miss), weights=_cuda(w), prior=[_cuda(p) for p in prior])
    assert b.x.data_ptr() == xu.data_ptr()
    b.run(2)
    assert _same(a.stats, b.stats) and _same(a._data, b._data) and torch.equal(a.r, b.r)
    if miss is not None:
        assert _same(a.filled(), b.filled())


@pytest.mark.parametrize('N,D,K,mode,offset', [(1031, 33, 33, 'both', 0.0), (1031, 33, 33, 'mask', 1000.0), (513, 64, 16, 'both', 0.0),
                                                (513, 64, 16, 'weights', 0.0)])
def test_device_bound_does_not_fall_over_20_iterations(N, D, K, mode, offset):
    x, r0, miss, w, prior = _data(N, D, K, mode, offset)
    loop = _loop(x, r0, miss, w, prior)
    bounds = []
    for _ in range(20):
        loop.run(1)
        bounds.append(loop.lower_bound())
    assert all(math.isfinite(b) for b in bounds)
    for u, v in zip(bounds, bounds[1:]):
        assert v >= u - 1e-6 * max(1.0, abs(u)), bounds


@pytest.mark.parametrize('N,D,K', [(1031, 33, 33), (513, 64, 16), (257, 17, 3)])
def test_zero_mask_and_unit_weights_agree_with_the_complete_row_loop(N, D, K):
    """within the bars of the complete-row truth; not bitwise (another pivot rule, another pack)"""
    x, r0 = T.make_data(N, D, K, 100 * D + 7 * K + N % 11)
    prior = T.default_prior(x, K)
    truth = T.bars(x, r0, prior, 3)
    ref = _mix().DiagLoop(_cuda(x), _cuda(r0), prior=[_cuda(p) for p in prior])
    ref.run(3)
    zero, ones = np.zeros((N, D), bool), np.ones(N, np.float32)
    for name, miss, w in (('zero mask', zero, None), ('unit weights', None, ones), ('both', zero, ones)):
        loop = _loop(x, r0, miss, w, prior)
        loop.run(3)
        got = dict(r=loop.r, logr=loop.logr, stats=loop.stats, theta=loop.theta(), data=loop._data.item(), bound=loop.lower_bound())
        bad = []
        for q, e in T.errors(got, truth).items():
            parity_log.record('abs' if q == 'r' else 'rel', e, truth['bar_' + q], 'DiagFitLoop %s N=%d D=%d K=%d %s' % (name, N, D, K, q))
            if not e <= truth['bar_' + q]:
                bad.append((q, e, truth['bar_' + q]))
        assert not bad, (name, bad)
        assert abs(loop.lower_bound() - ref.lower_bound()) <= 2 * truth['bar_bound'] * max(1.0, abs(ref.lower_bound()))
        if miss is not None:
            assert _same(loop.filled(), loop.x)


def test_surface_after_a_masked_fit():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import gmm
    Mx, E = _mix(), V._lib.VmpError
    N, D, K = 300, 12, 3
    x, r0, miss, w, prior = _data(N, D, K, 'both')
    truth = _case(N, D, K, 'both', 3)[5]
    xd, rd, md, wd = _cuda(x), _cuda(r0), _cuda(miss), _cuda(w)
    dp = Mx.default_diag_prior(xd, K, miss=md, weights=wd)
    for u, v in zip(dp, prior):
        assert torch.equal(u.cpu(), torch.as_tensor(v))
    with pytest.raises(E, match='DiagLoop'):
        Mx.DiagFitLoop(xd, rd)
    with pytest.raises(E, match='no masks'):
        Mx.DiagLoop(xd, rd, miss=md)
    step, log_r, theta, aux, x_filled = gmm.inference_diag_weighted(xd, wd, K, 0, miss=md, r_init=rd)
    for _ in range(3):
        r = step()
    loop = _loop(x, r0, miss, w, prior)
    with pytest.raises(E, match='iteration'):
        loop.lower_bound()
    loop.run(3)
    assert torch.equal(r, loop.r) and torch.equal(log_r(), loop.logr) and _same(x_filled(), loop.filled())
    for u, v in zip(theta() + aux(), loop.theta() + loop.aux()):
        assert torch.equal(u, v)
    _check('gmm.inference_diag_weighted N=%d D=%d K=%d' % (N, D, K), truth, dict(r=r, logr=log_r(), theta=theta(), fill=x_filled()))
    lb = gmm.lower_bound_diag(xd, *theta(), miss=md, weights=wd)
    assert lb.shape == () and lb.dtype == torch.float64 and lb.is_cuda and lb.item() == loop.lower_bound()
    _check('gmm.lower_bound_diag masked and weighted', truth, dict(bound=lb.item()))
    # the unweighted, unmasked call is what it was
    full = Mx.DiagLoop(xd.nan_to_num(), rd)
    full.run(2)
    assert gmm.lower_bound_diag(full.x, *full.theta()).item() == full.lower_bound()
    # the mask-only and weights-only entry points, the seeded weighted start
    s2 = gmm.inference_diag_missing(xd, md, K, 1)
    assert torch.isfinite(s2[0]()).all() and torch.isfinite(s2[4]()).all()
    s3 = gmm.inference_diag_weighted(xd, wd, K, 1, init='kmeans++')
    assert torch.isfinite(s3[0]()).all()
    with pytest.raises(E, match='no mask'):
        s3[4]()
    seeded = Mx.DiagFitLoop.from_seed(xd, K, 5, weights=wd)
    seeded.run(3)
    assert math.isfinite(seeded.lower_bound())
    with pytest.raises(E, match='masked wide rows'):
        Mx.DiagFitLoop.from_seed(xd, K, 5, weights=wd, miss=md)
    # scoring and filling rows the loop was not fitted on need theta alone
    xv, _, mv, _ = M.make_case(101, D, K, 77, 'mask')
    xv, mv = _cuda(xv), _cuda(mv)
    logp = gmm.predictive_logprob_diag(xv, *loop.theta(), miss=mv)
    assert torch.equal(loop.heldout_logprob(xv, mv), logp)
    assert loop.heldout(xv, mv) == pytest.approx(logp.double().mean().item(), rel=1e-6, abs=1e-6)
    xf, lp = loop.fill(xv, mv)
    want_f, want_lp = gmm.predictive_impute_diag(xv, mv, *loop.theta())
    assert torch.equal(xf, want_f) and torch.equal(lp, want_lp)
    hist = loop.run_until_bound(1e-5, check_every=2, max_iterations=40)
    assert 2 <= len(hist) <= 20 and hist[-1][0] == loop.iterations
    for (_, u), (_, v) in zip(hist, hist[1:]):
        assert v >= u - 1e-6 * max(1.0, abs(u)), hist
    # a NaN row for a component whose b is not positive
    th = [t.clone() for t in loop.theta()]
    th[4][1, 2] = 0.0
    pack = Mx.diag_mfit_pack(*th)
    assert pack.shape == (K, 3 * D + 1) and torch.isnan(pack[1]).all() and torch.isfinite(pack[0]).all() and torch.isfinite(pack[2]).all()
