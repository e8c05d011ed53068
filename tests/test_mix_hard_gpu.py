"""The mixture kernels on ill-conditioned data at converged fits (tests/mix_hard_truth.py): elongated, randomly oriented clusters,
columns decades apart, a column far from zero, components without rows, and a step that starts from the fp32-rounded posterior the
fp64 oracle has converged to - against that oracle's own next step in fp64.  tests/test_mix_hard_truth.py asserts, without a GPU,
that these truths keep rows soft, reach the conditioning and leave the fp32 oracle usable.

Bars: the project's rule as tests/test_mix_gpu.py and tests/mix_pass_truth.py state it - r max(1e-5, the fp32 oracle's own error on
the case) absolute, u 2e-5 relative, alpha, beta, m, C, v max(1e-5, 2 x the fp32 oracle's error) relative, log r where the truth's
r > 1e-30 as test_accurate_mode_vs_oracle; accurate=True at the literal 1e-5.  Score, impute, bound, masked, weighted and diagonal
fits: the bars of their own GPU tests (max(1e-5, 3 x the fp32 restatement's error)), unchanged.  Every error goes to the parity log."""
import math

import numpy as np
import pytest
import torch

import mix_hard_truth as H
import mix_tiled_shapes as S
import parity_log
import test_mix_gpu as T

pytestmark = pytest.mark.gpu


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _L():
    from vmp_for_svae_amd import _lib
    return _lib


def _cuda(a):
    return None if a is None else torch.as_tensor(np.asarray(a)).cuda()


def _loop(tr, smm, accurate=False):
    L = _L()
    K = tr['rT'].shape[1]
    return _mix().VMPLoop(T.dev(tr['x']), T.dev(tr['rT']), L.VMP_SMM if smm else L.VMP_GMM,
                          kappa=torch.full((K,), H.KAPPA, device='cuda') if smm else None, u_init=T.dev(tr['uT']) if smm else None,
                          accurate=accurate)


def _logr_err(logr, r1):
    big = r1 > 1e-30
    want = torch.log(r1[big])
    return (logr.double().cpu()[big] - want).abs().max().item(), 1e-4 * max(1.0, float(want.abs().max()))


def _one_step(name, flavour, accurate=False):
    """one step from the converged fp32-rounded posterior, and the finalize of the moments that step left, against the truth"""
    smm = flavour == 'smm'
    tr = H.converged(name, smm)
    c = H.CASES[name]
    what = 'hard %s %s%s ' % (name, flavour, ' accurate' if accurate else '')
    p = S.plan(_L().lib(), c['N'], c['D'], c['K'], flavour, S.FUSED)
    assert (p['form'], p['kt_mt']) == H.FORMS[name], (name, p)                  # the kernel form this case is here for
    lp = _loop(tr, smm, accurate)
    r = lp.step(want_logr=True)
    bad = []

    def hold(err, bar, n_):
        print('%s%s: kernel %.3e  bar %.3e  fp32 oracle %.3e' % (what, n_, err, bar, tr['e32'].get(n_.split(' ')[-1], float('nan'))))
        if not err <= bar:
            bad.append((n_, err, bar))

    assert torch.isfinite(r).all() and torch.isfinite(lp.logr[r > 0]).all(), what
    assert float((r.double().sum(1) - 1.0).abs().max()) <= 1e-6, what
    parity_log.record('abs', tr['e32']['r'], None, what + 'r_nk: fp32 oracle (reference dtype) vs fp64 truth')
    bar = 1e-5 if accurate else H.bar_r(tr)
    hold(T.abserr(r, tr['r1'].numpy(), what + 'r_nk', bar), bar, 'r')
    e, bar = _logr_err(lp.logr, tr['r1'])
    hold(parity_log.record('abs', e, bar, what + 'log r_nk'), bar, 'logr')
    if smm:
        assert torch.isfinite(lp.u).all(), what
        bar = 1e-5 if accurate else 2e-5
        hold(T.relerr(lp.u, tr['u1'].numpy(), what + 'u_nk', bar), bar, 'u')
    for stage, th in (('', tr['theta0']), ('next ', tr['theta1'])):             # the M-step of the input, then of this step's output
        if stage:
            lp.finalize()
        for n_, t, o in zip(H.NAMES, lp.theta(), th):
            assert torch.isfinite(t).all(), what + stage + n_
            bar = 1e-5 if accurate else H.bar_theta(tr, n_)
            hold(T.relerr(t, o.numpy(), what + stage + n_, bar), bar, stage + n_)
    assert not bad, (what, bad)


@pytest.mark.parametrize('flavour', H.FLAVOURS)
@pytest.mark.parametrize('name', H.LOOP_CASES)
def test_one_step_from_the_converged_posterior(name, flavour):
    _one_step(name, flavour)


@pytest.mark.parametrize('flavour', H.FLAVOURS)
@pytest.mark.parametrize('name', H.ACCURATE_CASES)
def test_accurate_step_from_the_converged_posterior(name, flavour):
    _one_step(name, flavour, accurate=True)


# ---- score, impute, bound at the converged theta ---------------------------------------------------------------------------------
SURFACES = (H.SURFACE_CASE, H.AUTO_CASE)


def _report(kind, what, err, bar, e32):
    parity_log.record(kind, err, bar, '%s (fp32 restatement: %.2e)' % (what, e32))
    print('%s: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, err, e32, bar))
    return err <= bar


@pytest.mark.parametrize('name', SURFACES)
def test_predictive_and_heldout_logprob_at_the_converged_theta(name):
    import mix_score_truth as Sc
    from vmp_for_svae_amd.models import gmm, smm
    x = H.data(name)[0]
    xd = _cuda(x)
    th = H.theta32(name)
    lp, rs, bar_lp, bar_rs, e_lp, e_rs = Sc.bars(x, Sc.pack_niw(*th))
    logp, total, resp = gmm.predictive_logprob(xd, *[_cuda(t) for t in th], return_resp=True)
    assert torch.isfinite(logp).all() and torch.isfinite(resp).all() and (resp.double().sum(1) - 1).abs().max().item() < 1e-6
    ok = [_report('rel', 'hard %s gmm.predictive_logprob logp' % name, Sc.rel_err(logp, lp), bar_lp, e_lp),
          _report('abs', 'hard %s gmm.predictive_logprob resp' % name, Sc.abs_err(resp, rs), bar_rs, e_rs)]
    assert abs(total.item() - logp.double().sum().item()) <= 1e-12 * abs(total.item())
    ts = tuple(t.float() for t in H.converged(name, True)['theta0'])
    al, be, m, C, v = [t.double() for t in ts]
    K = m.shape[0]
    kap = torch.full((K,), H.KAPPA)
    lp, rs, bar_lp, bar_rs, e_lp, e_rs = Sc.bars(x, Sc.pack_t(torch.log(al / al.sum()), m, C / v[:, None, None], kap.double()))
    logp, total, resp = smm.heldout_logprob(xd, *[_cuda(t) for t in ts], kap.cuda(), return_resp=True)
    assert torch.isfinite(logp).all() and torch.isfinite(resp).all() and (resp.double().sum(1) - 1).abs().max().item() < 1e-6
    ok += [_report('rel', 'hard %s smm.heldout_logprob logp' % name, Sc.rel_err(logp, lp), bar_lp, e_lp),
           _report('abs', 'hard %s smm.heldout_logprob resp' % name, Sc.abs_err(resp, rs), bar_rs, e_rs)]
    assert all(ok), (name, ok)


@pytest.mark.parametrize('name', SURFACES)
def test_predictive_impute_at_the_converged_theta(name):
    import mix_impute_truth as I
    from vmp_for_svae_amd.models import gmm
    x = H.data(name)[0]
    miss = H.mask(name)
    assert 0.25 < miss.mean() < 0.35
    th = H.theta32(name)
    tr = I.bars(x, miss, I.pack_niw(*th))
    xin = x.copy()
    xin[miss != 0] = np.nan
    x_out, logp, resp = gmm.predictive_impute(_cuda(xin), _cuda(miss), *[_cuda(t) for t in th], return_resp=True)
    assert torch.isfinite(x_out).all() and torch.isfinite(logp).all() and (resp.double().sum(1) - 1).abs().max().item() < 1e-6
    o = torch.as_tensor(miss == 0)
    assert torch.equal(x_out.cpu().view(torch.int32)[o], torch.as_tensor(x).view(torch.int32)[o])
    ok = [_report('rel', 'hard %s gmm.predictive_impute logp' % name, I.rel_err(logp, tr['logp']), tr['bar_logp'], tr['e_logp']),
          _report('abs', 'hard %s gmm.predictive_impute resp' % name, I.abs_err(resp, tr['resp']), tr['bar_resp'], tr['e_resp']),
          _report('rel', 'hard %s gmm.predictive_impute x_out' % name, I.rel_err(x_out, tr['x_out']), tr['bar_x'], tr['e_x'])]
    assert all(ok), (name, ok)


@pytest.mark.parametrize('name', SURFACES)
def test_lower_bound_at_the_converged_theta(name):
    import mix_bound_truth as B
    from vmp_for_svae_amd.models import gmm
    smm = False
    tr = H.converged(name, smm)
    x = tr['x']
    th = H.theta32(name)
    truth = B.case(x, None, th)
    lb = gmm.lower_bound(_cuda(x), *[_cuda(t) for t in th])
    assert math.isfinite(lb.item())
    ok = [_report('rel', 'hard %s gmm.lower_bound' % name, B.rel(lb.item(), truth['bound']), truth['bar_bound'], truth['e_bound'])]
    # the loop's own bound after its step, against the truth at the theta the loop holds (the M-step of rT, which
    # test_one_step_from_the_converged_posterior holds to the oracle)
    lp = _loop(tr, smm)
    lp.step()
    own = B.case(x, None, tuple(t.cpu() for t in lp.theta()))
    ok.append(_report('rel', 'hard %s loop.lower_bound()' % name, B.rel(lp.lower_bound(), own['bound']), own['bar_bound'], own['e_bound']))
    assert all(ok), (name, ok)


# ---- the masked, the weighted and the diagonal loop, one step from the same posterior -----------------------------------------------
def _hold(what, errs, truth):
    bad = []
    for n_, e in errs.items():
        bar, e32 = truth['bar_' + n_], truth['e_' + n_]
        if not _report('abs' if n_ == 'r' else 'rel', '%s %s' % (what, n_), e, bar, e32):
            bad.append((n_, e, bar))
    assert not bad, (what, bad)


def test_masked_step_from_the_converged_posterior():
    import mix_missfit_truth as M
    xm, rT, miss, truth = H.masked()
    lp = _mix().VMPLoop(_cuda(xm), _cuda(rT), _L().VMP_GMM, miss=_cuda(miss))
    r = lp.step(want_logr=True)
    assert torch.isfinite(r).all() and torch.isfinite(lp.filled()).all() and (r.double().sum(1) - 1).abs().max().item() < 1e-6
    errs = dict(r=M.abs_err(r, truth['r']), logr=M.rel_err(lp.logr, truth['logr']), x_fill=M.rel_err(lp.filled(), truth['x_fill']),
                stats=M.rel_err(lp.stats, truth['stats']))
    errs.update((n_, M.rel_err(t, o)) for n_, t, o in zip(H.NAMES, lp.theta(), truth['theta']))
    _hold('hard masked %s' % H.FIT_CASE, errs, truth)


def test_weighted_step_from_the_converged_posterior():
    import mix_wfit_truth as W
    xw, rT, w, truth = H.weighted()
    lp = _mix().VMPLoop(_cuda(xw), _cuda(rT), _L().VMP_GMM, weights=_cuda(w))
    r = lp.step(want_logr=True)
    ok = W.finite_rows(truth)
    assert int((~ok).sum()) == int(np.isnan(xw).all(1).sum()) and torch.isfinite(r.cpu()[ok]).all()
    assert (r.double().sum(1).cpu()[ok] - 1).abs().max().item() < 1e-6 and torch.isfinite(lp.stats).all()
    got = dict(r=r, logr=lp.logr, stats=lp.stats, theta=lp.theta(), data=lp._data.item(), bound=lp.lower_bound())
    _hold('hard weighted %s' % H.FIT_CASE, W.errors(got, truth), truth)


@pytest.mark.parametrize('name', sorted(H.DIAG_CASES))
def test_diagonal_step_from_the_converged_posterior(name):
    import mix_diag_truth as G
    x, rT, prior, truth = H.diag(name)
    lp = _mix().DiagLoop(_cuda(x), _cuda(rT), prior=[_cuda(p) for p in prior])
    r = lp.step(want_logr=True)
    assert torch.isfinite(r).all() and (r.double().sum(1) - 1).abs().max().item() < 1e-6
    got = dict(r=r, logr=lp.logr, stats=lp.stats, theta=lp.theta(), data=lp._data.item(), bound=lp.lower_bound())
    assert torch.isfinite(got['stats']).all() and math.isfinite(got['bound']) and all(torch.isfinite(t).all() for t in got['theta'])
    _hold('hard %s' % name, G.errors(got, truth), truth)


TRACKED = 10


# ---- free-running ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'masked', 'weighted', 'diagonal'])
def test_forty_free_running_iterations_stay_finite_and_the_bound_does_not_fall(kind):
    """The slack is the floor of what test_run_until_bound_terminates_and_does_not_fall grants (its bar is max(1e-5, ...)):
    1e-5 max(1, |bound|).  The diagonal fit ascends its bound and is held to that alone.  The full-covariance fits do not, in fp64
    either (mix_hard_truth.bound_sequence: the reference's det <= 1e-20 guard; measured on an MI355X: -2.40e4, +6.16e3, -1.84e4 in
    iterations 5 .. 7 of the plain loop, the fp64 truth the same to six digits): over the first BOUND_ITERATIONS iterations the
    device's bound may fall by what the fp64 iteration's falls plus that slack at either end, from then on not at all - and over the
    first TRACKED iterations the device's bound itself is held to the fp64 iteration's under the bound tests' own bar
    (max(1e-5, 3 x the fp32 restatement's error), relative to max(1, |bound|))."""
    import mix_diag_truth as G
    M, L = _mix(), _L()
    name = H.SURFACE_CASE
    x, r0, miss, w = H.free_inputs(kind if kind != 'diagonal' else 'plain')
    xd, rd = _cuda(x), _cuda(r0)
    if kind == 'diagonal':
        lp = M.DiagLoop(xd, rd, prior=[_cuda(p) for p in G.default_prior(x, r0.shape[1])])
        fp64, bars = [], []
    else:
        lp = M.VMPLoop(xd, rd, L.VMP_GMM, miss=_cuda(miss), weights=_cuda(w))
        fp64, bars = H.bound_sequence(kind)
    bounds = []
    for _ in range(H.T_ITER):
        r = lp.step()
        bounds.append(lp.lower_bound())
    assert torch.isfinite(r).all() and (r.double().sum(1) - 1).abs().max().item() < 1e-6
    assert all(math.isfinite(b) for b in bounds), bounds
    # the device's bound against the fp64 iteration's, at the floor of the bound tests' bar, while the two iterations can be
    # expected to walk the same path (the first TRACKED iterations: the collapse of the fit lies inside them)
    off = [abs(b - t) / max(1.0, abs(t)) for b, t in zip(bounds[:TRACKED], fp64[:TRACKED])]
    track = max(off + [0.0])
    parity_log.record('rel', track, max(bars[:TRACKED] + [1e-5]), 'hard %s free-running %s: bound vs the fp64 iteration, first %d iterations' % (name, kind, TRACKED))
    worst = 0.0
    for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
        granted = max(0.0, fp64[i] - fp64[i + 1]) if i + 1 < len(fp64) else 0.0
        worst = max(worst, (a - b - granted) / (max(1.0, abs(a)) + (max(1.0, abs(b)) if granted else 0.0)))
    parity_log.record('rel', worst, 1e-5, 'hard %s free-running %s: largest fall of the bound beyond the fp64 iteration\'s' % (name, kind))
    print('free-running %s: bound %s ... %.6e, largest fall beyond fp64 %.3e, off the fp64 bound by %.3e' % (
        kind, ['%.5e' % b for b in bounds[:10]], bounds[-1], worst, track))
    print('free-running %s: fp64 %s' % (kind, ['%.5e' % b for b in fp64[:10]]))
    print('free-running %s: off %s bars %s' % (kind, ['%.2e' % e for e in off], ['%.2e' % e for e in bars[:TRACKED]]))
    assert all(e <= bar for e, bar in zip(off, bars)), (kind, off, bars[:TRACKED])
    assert worst <= 1e-5, (kind, worst, bounds, fp64)
