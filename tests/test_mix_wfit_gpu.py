"""The Gaussian-mixture fit on weighted rows on the GPU (csrc/vmp_wfit.hip, _mix.mixture_wfit_pass, VMPLoop(..., weights=),
gmm.inference_weighted, gmm.lower_bound(weights=)) against the fp64 truth of tests/mix_wfit_truth.py: the pass and the loop over a
shape sweep, complete and masked; replication (integer weights against the existing loops on the replicated rows); unit weights
against the existing kernels; bit identity; a 0/1 fold against the loop on the gathered rows; unaligned operands; the Python surface.

Tolerance (never a constant found on the kernel): per case and per quantity bar = max(1e-5, 3 x the error of the fp32 restatement
against the fp64 truth, both run from the same inputs for the same number of iterations) - absolute for r, relative to
max(1, |value|) for everything else.  Where two device results are compared, each with a truth of its own, the bar is the sum of the
two cases' bars.  Achieved errors and bars go to the parity log.
Weights are seeded from {0, 0.25, 1, 3, 7.5} with about 20 % zeros.  Masks have about 25 % missing, row 0 fully missing, row 1 fully
observed, NaN in the missing slots.  Row 2 always has weight 0 and NaN in an OBSERVED slot: the select of the kernel."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import mix_wfit_truth as W
import parity_log

pytestmark = pytest.mark.gpu

SWEEP = [(257, 8, 3), (65, 3, 17), (4099, 2, 16), (1031, 8, 16), (513, 5, 33), (300, 1, 2), (2051, 8, 64)]
FORMS = pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
NAMES = ('alpha', 'beta', 'm', 'C', 'v')


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _gmm():
    import vmp_for_svae_amd as V
    return V._lib.VMP_GMM


def _cuda(a):
    return None if a is None else torch.as_tensor(a).cuda()


@functools.lru_cache(maxsize=None)
def _data(N, D, K, masked, integer=False):
    return W.make_data(N, D, K, 100 * D + 7 * K + N % 11, masked, integer=integer)


@functools.lru_cache(maxsize=None)
def _case(N, D, K, masked, iterations, integer=False):
    """inputs and the truth with its bars: computed once, shared, never modified"""
    x, r0, miss, w = _data(N, D, K, masked, integer)
    return x, r0, miss, w, W.bars(x, miss, w, r0, iterations)


def _loop(x, r0, miss, w, **kw):
    return _mix().VMPLoop(_cuda(x), _cuda(r0), _gmm(), miss=_cuda(miss), weights=_cuda(w), **kw)


def _state(loop, r=True):
    return dict(r=loop.r if r else None, logr=loop.logr, x_fill=loop.x_fill if loop.miss is not None else None, stats=loop.stats,
                theta=loop.theta(), data=loop._data.item(), bound=loop.lower_bound())


def _check(what, truth, got, also=None):
    """every quantity of `got` against the truth under its bar (plus the bar of `also`, a second truth, where two device results meet)"""
    bad = []
    for name, e in W.errors(got, truth).items():
        bar, e32 = truth['bar_' + name] + (also['bar_' + name] if also else 0.0), truth['e_' + name]
        parity_log.record('abs' if name == 'r' else 'rel', e, bar, '%s %s (fp32 restatement: %.2e)' % (what, name, e32))
        print('%s %s: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, name, e, e32, bar))
        if not e <= bar:
            bad.append((name, e, bar, e32))
    assert not bad, (what, bad)


def _observed_bits_kept(x_fill, x, miss):
    o = torch.as_tensor(miss == 0)
    return torch.equal(x_fill.cpu().view(torch.int32)[o], torch.as_tensor(x).view(torch.int32)[o])


def _one_iteration(N, D, K, masked):
    M = _mix()
    x, r0, miss, w, truth = _case(N, D, K, masked, 1)
    assert w[2] == 0 and np.isnan(x[2, 0]) and (miss is None or miss[2, 0] == 0) and 0.1 < (w == 0).mean() < 0.3
    if masked:
        assert 0.15 < miss.mean() < 0.35 and miss[0].all() and not miss[1].any()
    loop = _loop(x, r0, miss, w)
    r = loop.step(want_logr=True)
    ok = W.finite_rows(truth)
    assert r.shape == (N, K) and int(ok.sum()) == N - 1
    assert (r.double().sum(1).cpu()[ok] - 1).abs().max().item() < 1e-6
    what = '1 iteration N=%d D=%d K=%d %s' % (N, D, K, 'masked' if masked else 'complete')
    st = _state(loop)
    assert torch.isfinite(st['stats']).all() and math.isfinite(st['data']) and math.isfinite(st['bound'])
    _check(what, truth, st)
    if masked:
        assert _observed_bits_kept(loop.filled(), x, miss)
    # the pass through its wrapper is the loop's own pass
    got = M.mixture_wfit_pass(_cuda(x), _cuda(w), loop.fpack, miss=_cuda(miss), want_logr=True, want_fill=masked, want_bound=True)
    for u, v in zip(got, (loop.r, loop.logr, loop.x_fill, loop.stats, loop._data)):
        assert (u is None and v is None) or torch.equal(u.view(torch.int64 if u.dtype == torch.float64 else torch.int32),
                                                         v.view(torch.int64 if v.dtype == torch.float64 else torch.int32))
    return loop


@FORMS
@pytest.mark.parametrize('N,D,K', SWEEP)
def test_pass_and_one_step_shape_sweep(N, D, K, masked):
    _one_iteration(N, D, K, masked)


@FORMS
def test_second_chunk_of_a_wave(masked):
    """A wave owns a second chunk only above N = 262144: the second flush reads the wave's fp64 words back and adds to them"""
    _one_iteration(262144 + 517, 2, 3, masked)


@FORMS
@pytest.mark.parametrize('N,D,K', [(1031, 8, 16), (513, 5, 33)])
def test_five_iterations_and_run_equals_steps(N, D, K, masked):
    x, r0, miss, w, truth = _case(N, D, K, masked, 5)
    a = _loop(x, r0, miss, w)
    a.run(5)
    _check('run(5) N=%d D=%d K=%d %s' % (N, D, K, 'masked' if masked else 'complete'), truth, _state(a))
    b = _loop(x, r0, miss, w)
    for _ in range(5):
        b.step()
    assert a.iterations == b.iterations == 5
    rows = W.finite_rows(truth).cuda()
    assert torch.equal(a.r[rows], b.r[rows]) and torch.equal(a.stats, b.stats) and torch.equal(a._data, b._data)
    assert a.lower_bound() == b.lower_bound()
    if masked:
        assert torch.equal(a.filled()[rows], b.filled()[rows])
    for u, v in zip(a.theta() + a.aux(), b.theta() + b.aux()):
        assert torch.equal(u, v)


@FORMS
@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (513, 5, 33)])
def test_integer_weights_are_the_existing_loop_on_replicated_rows(N, D, K, masked):
    M = _mix()
    x, r0, miss, w, truth = _case(N, D, K, masked, 5, True)
    rep = np.repeat(np.arange(N), w.astype(np.int64))
    assert 2 not in rep and np.isfinite(x[rep][(miss[rep] == 0) if masked else slice(None)]).all()
    xr, rr, mr = x[rep], r0[rep], (miss[rep] if masked else None)
    other = W.bars(xr, mr, np.ones(len(rep), np.float32), rr, 5)
    wl = _loop(x, r0, miss, w)
    wl.run(5)
    el = M.VMPLoop(_cuda(xr), _cuda(rr), _gmm(), miss=_cuda(mr))                     # the loop as it was: no weights
    el.run(5)
    what = 'replication N=%d (%d rows) D=%d K=%d %s' % (N, len(rep), D, K, 'masked' if masked else 'complete')
    _check(what + ' weighted', truth, dict(theta=wl.theta(), bound=wl.lower_bound()))
    _check(what + ' weighted vs existing', other, dict(theta=wl.theta(), bound=wl.lower_bound()), also=truth)
    for name, u, v in zip(NAMES, wl.theta(), el.theta()):
        e, bar = W.rel_err(u, v.double().cpu()), truth['bar_' + name] + other['bar_' + name]
        parity_log.record('rel', e, bar, what + ' %s device vs device' % name)
        assert e <= bar, (name, e, bar)
    e, bar = W._rel(wl.lower_bound(), el.lower_bound()), truth['bar_bound'] + other['bar_bound']
    parity_log.record('rel', e, bar, what + ' bound device vs device')
    assert e <= bar, (e, bar)


@FORMS
@pytest.mark.parametrize('N,D,K', [(1031, 8, 16), (513, 5, 33)])
def test_unit_weights_against_the_existing_kernels(N, D, K, masked):
    """w = 1: r against _mix.estep (complete rows) / mixture_fit_pass (masked), the moments against mixture_fit_pass under the same
    mask (all observed for complete rows), the data term against mixture_bound - other kernels, so within the bar, not bit for bit"""
    M = _mix()
    x, r0, miss, _ = _data(N, D, K, masked)
    x = x.copy()
    x[2, 0] = 0.25                                                            # every row counts here
    w = np.ones(N, np.float32)
    truth = W.bars(x, miss, w, r0, 1)
    loop = _loop(x, r0, miss, w)
    loop.step()
    what = 'unit weights N=%d D=%d K=%d %s' % (N, D, K, 'masked' if masked else 'complete')
    _check(what, truth, _state(loop))
    xd = _cuda(x)
    md = _cuda(miss) if masked else torch.zeros(N, D, dtype=torch.uint8, device='cuda')
    r_fit, _, _, st_fit = M.mixture_fit_pass(xd, md, loop.fpack)
    data, _ = M.mixture_bound(xd, _cuda(miss), loop.fpack)
    r_ref = r_fit if masked else M.estep(xd, loop.post['pack'], _gmm())[0]
    for name, kind, e in (('r', 'abs', W.abs_err(loop.r, r_ref.double().cpu())), ('stats', 'rel', W.rel_err(loop.stats, st_fit.cpu())),
                          ('data', 'rel', W._rel(loop._data.item(), data.item()))):
        parity_log.record(kind, e, truth['bar_' + name], '%s %s vs the existing kernel' % (what, name))
        assert e <= truth['bar_' + name], (name, e, truth['bar_' + name])


def _bits(t):
    return None if t is None else t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@FORMS
@pytest.mark.parametrize('N,D,K', [(1031, 8, 16), (513, 5, 33)])
def test_bit_identity_across_runs_and_every_output_set(N, D, K, masked):
    M = _mix()
    x, r0, miss, w = _data(N, D, K, masked)
    loop = _loop(x, r0, miss, w)
    loop.finalize()
    xd, wd, md = _cuda(x), _cuda(w), _cuda(miss)

    def run(**kw):
        return M.mixture_wfit_pass(xd, wd, loop.fpack, miss=md, **kw)

    full = run(want_r=True, want_logr=True, want_fill=masked, want_stats=True, want_bound=True)
    assert torch.isfinite(full[3]).all() and torch.isfinite(full[4])
    again = run(want_r=True, want_logr=True, want_fill=masked, want_stats=True, want_bound=True)
    for u, v in zip(full, again):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))
    sets = 0
    for want in itertools.product((False, True), repeat=5):
        want_r, want_logr, want_fill, want_stats, want_bound = want
        if not any(want) or ((want_logr or want_stats) and not want_r) or (want_fill and not masked):
            continue
        part = run(want_r=want_r, want_logr=want_logr, want_fill=want_fill, want_stats=want_stats, want_bound=want_bound)
        for asked, u, v in zip(want, part, full):
            assert (u is None) if not asked else torch.equal(_bits(u), _bits(v)), want
        sets += 1
    assert sets == (19 if masked else 9)
    # the loop's own step is the same pass
    loop.estep(want_logr=True)
    for u, v in zip((loop.r, loop.logr, loop.x_fill, loop.stats, loop._data), full):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))


@FORMS
@pytest.mark.parametrize('N,D,K', [(1031, 8, 16), (513, 5, 33)])
def test_a_fold_is_the_loop_on_the_gathered_rows(N, D, K, masked):
    """0/1 weights over the resident rows against the existing loop on a gathered copy; r of the held-out rows is the E-step on them"""
    M = _mix()
    x, r0, miss, w = _data(N, D, K, masked)
    fold = (w > 0).astype(np.float32)
    sub = np.nonzero(fold)[0]
    held = np.setdiff1d(np.arange(N), np.append(sub, 2))                      # row 2 holds NaN: held out, and its r is NaN
    xs, rs, ms = x[sub], r0[sub], (miss[sub] if masked else None)
    truth = W.bars(x, miss, fold, r0, 3)
    other = W.bars(xs, ms, np.ones(len(sub), np.float32), rs, 3)
    wl = _loop(x, r0, miss, fold)
    for _ in range(3):
        wl.step()                                 # step(), not run(): the E-step pack of the last finalize is compared against below
    gl = M.VMPLoop(_cuda(xs), _cuda(rs), _gmm(), miss=_cuda(ms))
    gl.run(3)
    what = 'fold N=%d (%d kept) D=%d K=%d %s' % (N, len(sub), D, K, 'masked' if masked else 'complete')
    _check(what, truth, _state(wl))
    _check(what + ' vs gathered truth', other, dict(theta=wl.theta(), bound=wl.lower_bound(), stats=wl.stats), also=truth)
    for name, u, v in zip(NAMES, wl.theta(), gl.theta()):
        e, bar = W.rel_err(u, v.double().cpu()), truth['bar_' + name] + other['bar_' + name]
        parity_log.record('rel', e, bar, what + ' %s vs the gathered loop' % name)
        assert e <= bar, (name, e, bar)
    e, bar = W.abs_err(wl.r[_cuda(sub)], gl.r.double().cpu()), truth['bar_r'] + other['bar_r']
    parity_log.record('abs', e, bar, what + ' r of the kept rows vs the gathered loop')
    assert e <= bar, (e, bar)
    e, bar = W._rel(wl.lower_bound(), gl.lower_bound()), truth['bar_bound'] + other['bar_bound']
    parity_log.record('rel', e, bar, what + ' bound vs the gathered loop')
    assert e <= bar, (e, bar)
    # held-out rows: the responsibilities of the E-step at the loop's theta - the same kernel on those rows alone gives the same
    # bits, the existing E-step kernels agree within the bar
    xh, mh = _cuda(x[held]), (_cuda(miss[held]) if masked else None)
    r_held = wl.r[_cuda(held)]
    assert torch.isfinite(r_held).all() and (r_held.double().sum(1) - 1).abs().max().item() < 1e-6
    same = M.mixture_wfit_pass(xh, torch.ones(len(held), device='cuda'), wl.fpack, miss=mh, want_stats=False)[0]
    assert torch.equal(same, r_held)
    ref = M.mixture_fit_pass(xh, mh, wl.fpack, want_stats=False)[0] if masked else M.estep(xh, wl.post['pack'], _gmm())[0]
    e = W.abs_err(r_held, ref.double().cpu())
    parity_log.record('abs', e, truth['bar_r'], what + ' r of the held-out rows vs the existing E-step')
    assert e <= truth['bar_r'], (e, truth['bar_r'])


@FORMS
@pytest.mark.parametrize('N,D,K', [(65, 3, 17), (513, 5, 33), (257, 5, 3)])
def test_unaligned_x_and_x_fill_give_the_same_bits(N, D, K, masked):
    """x a view offset by one row of an odd D (4 D bytes: not a multiple of 16), x_fill likewise: the scalar paths"""
    x, r0, miss, w = _data(N, D, K, masked)
    a = _loop(x, r0, miss, w)
    a.run(2)
    buf = torch.empty((N + 2) * D, dtype=torch.float32, device='cuda')
    xu = buf[D:D + N * D].view(N, D)
    xu.copy_(_cuda(x))
    assert a.x.data_ptr() % 16 == 0 and xu.data_ptr() % 16 != 0 and xu.is_contiguous()
    b = _mix().VMPLoop(xu, _cuda(r0), _gmm(), miss=_cuda(miss), weights=_cuda(w))
    assert b.x.data_ptr() == xu.data_ptr()
    if masked:
        fbuf = torch.empty((N + 2) * D, dtype=torch.float32, device='cuda')
        b.x_fill = fbuf[D:D + N * D].view(N, D)
        assert b.x_fill.data_ptr() % 16 != 0
    b.run(2)
    rows = torch.ones(N, dtype=torch.bool, device='cuda')
    rows[2] = False
    assert torch.equal(a.r[rows], b.r[rows]) and torch.equal(a.stats, b.stats) and torch.equal(a._data, b._data)
    if masked:
        assert torch.equal(_bits(a.filled()), _bits(b.filled()))


# ---- Python surface -----------------------------------------------------------------------------------------------------
@FORMS
def test_run_until_bound_terminates_and_does_not_fall(masked):
    N, D, K = (90, 3, 4) if masked else (120, 2, 3)
    x, r0, miss, w = W.make_data(N, D, K, 2 if masked else 1, masked)         # the cases whose fp64 bound is shown not to fall
    truth = W.bars(x, miss, w, r0, 10)
    loop = _loop(x, r0, miss, w)
    hist = loop.run_until_bound(1e-4, check_every=2, max_iterations=40)
    assert 2 <= len(hist) <= 20 and hist[-1][0] == loop.iterations and all(math.isfinite(b) for _, b in hist)
    for (_, a), (_, b) in zip(hist, hist[1:]):
        assert b >= a - truth['bar_bound'] * max(1.0, abs(a)), hist
    assert len(hist) == 20 or hist[-1][1] - hist[-2][1] < 1e-4 * max(1.0, abs(hist[-1][1]))


@FORMS
def test_gmm_inference_weighted_and_lower_bound_agree_with_the_loop(masked):
    from vmp_for_svae_amd.models import gmm
    N, D, K = 300, 4, 3
    x, r0, miss, w = W.make_data(N, D, K, 5, masked)
    truth = W.bars(x, miss, w, r0, 3)
    xd, wd, md, rd = _cuda(x), _cuda(w), _cuda(miss), _cuda(r0)
    step, log_r, theta, aux, filled = gmm.inference_weighted(xd, wd, K, 0, miss=md, r_init=rd)
    for _ in range(3):
        r = step()
    loop = _loop(x, r0, miss, w)
    for _ in range(3):
        loop.step(want_logr=True)
    rows = W.finite_rows(truth).cuda()
    assert torch.equal(r[rows], loop.r[rows]) and torch.equal(log_r()[rows], loop.logr[rows])
    for u, v in zip(theta() + aux(), loop.theta() + loop.aux()):
        assert torch.equal(u, v)
    _check('gmm.inference_weighted N=%d D=%d K=%d' % (N, D, K), truth, dict(r=r, logr=log_r(), theta=theta(), x_fill=filled() if masked else None))
    # the explicit-parameter bound: the bound-only form of the pass gives the bits the loop's own pass left behind
    lb = gmm.lower_bound(xd, *theta(), miss=md, weights=wd)
    assert lb.shape == () and lb.dtype == torch.float64 and lb.is_cuda and lb.item() == loop.lower_bound()
    _check('gmm.lower_bound(weights=)', truth, dict(bound=lb.item()))
    # the default and the seeded initialisation run too
    for init in ('random', 'kmeans++'):
        xs = xd.clone()
        xs[2, 0] = 0.0                            # the seeding is unweighted: it reads every row
        step2 = gmm.inference_weighted(xs, wd, K, 1, miss=md, init=init)[0]
        keep = torch.ones(N, dtype=torch.bool, device='cuda')
        keep[2] = False
        assert torch.isfinite(step2()[keep]).all()


def test_the_other_methods_work_on_a_weighted_loop():
    import vmp_for_svae_amd as V
    M = _mix()
    N, D, K = 300, 4, 3
    x, r0, miss, w = W.make_data(N, D, K, 5, True)
    loop = _loop(x, r0, miss, w)
    with pytest.raises(V._lib.VmpError, match='iteration'):
        loop.lower_bound()
    loop.run(3)
    x_val = _cuda(W.make_data(64, D, K, 6, False)[0]).nan_to_num()
    assert math.isfinite(loop.score(x_val))
    x_out, logp = loop.impute(_cuda(np.delete(x, 2, 0)), _cuda(np.delete(miss, 2, 0)))
    assert torch.isfinite(x_out).all() and torch.isfinite(logp).all()
    assert loop.sample(16, 3).shape == (16, D)
    assert loop.impute_draws(_cuda(np.delete(x, 2, 0)), _cuda(np.delete(miss, 2, 0)), 2, 3).shape == (2, N - 1, D)
    st = loop.stats
    assert st.shape == (K, 2 + D + D * D) and abs(st[:, 0].sum().item() - float(w.sum())) < 1e-3 * w.sum()
    assert torch.equal(st[:, 0], st[:, 1])
    complete = _loop(np.nan_to_num(x), r0, None, w)
    complete.run(1)
    with pytest.raises(V._lib.VmpError, match='miss='):
        complete.filled()
    seeded = M.VMPLoop.from_seed_weighted(_cuda(np.nan_to_num(x)), _cuda(w), K, _gmm(), 7)
    seeded.run(2)
    assert math.isfinite(seeded.lower_bound()) and torch.isfinite(seeded.r).all()
