"""Mixture scoring on the GPU (csrc/vmp_score.hip): the two pack builders and the streaming score kernel against the fp64 truth of
tests/mix_score_truth.py, over a shape sweep that crosses the 64-row tile edge, ragged tails and the 16-component tile edges; the
deterministic row sum; unaligned x; the -inf / far-row / NaN edge cases; and the Python surface (student_t.mixture_logprob,
gmm.predictive_logprob, smm.heldout_logprob, VMPLoop.score / run_until).

Tolerance (never a constant found on the kernel): bar = max(1e-5, 3 x the error of the op-for-op fp32 torch-CPU restatement against
the fp64 truth on the same inputs) - relative to max(1, |value|) for logp, absolute for resp.  Achieved errors and bars go to the
parity log (tests/parity_log.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import mix_score_truth as T
import parity_log

pytestmark = pytest.mark.gpu

# every N, D, K of the sweep at least twice; every (D odd, K > 16) pairing once
SWEEP = [(1, 1, 17), (63, 1, 33), (64, 1, 64), (65, 3, 17), (257, 3, 33), (4099, 3, 64), (1, 5, 17), (63, 5, 33), (64, 5, 64),
         (65, 2, 1), (257, 2, 3), (4099, 8, 16), (64, 8, 1), (257, 8, 3), (4099, 2, 16), (65, 8, 64), (63, 2, 17), (1, 8, 33)]


def test_the_sweep_covers_what_it_claims():
    for axis, values in ((0, (1, 63, 64, 65, 257, 4099)), (1, (1, 2, 3, 5, 8)), (2, (1, 3, 16, 17, 33, 64))):
        for v in values:
            assert sum(1 for c in SWEEP if c[axis] == v) >= 2, (axis, v)
        assert {c[axis] for c in SWEEP} == set(values)
    for D in (1, 3, 5):
        for K in (17, 33, 64):
            assert sum(1 for c in SWEEP if c[1] == D and c[2] == K) == 1, (D, K)


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _cuda(d):
    return {k: torch.as_tensor(a).cuda() for k, a in d.items()}


@functools.lru_cache(maxsize=None)
def _case(N, D, K):
    """inputs, both truth packs and their bars: computed once, shared, never modified"""
    x, t, q = T.make_case(N, D, K, seed=1000 * D + 10 * K + N % 7)
    return x, t, q, T.bars(x, T.pack_t(**t)), T.bars(x, T.pack_niw(**q))


def _pack(builder, t, q):
    M = _mix()
    if builder == 't':
        c = _cuda(t)
        return M.score_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    c = _cuda(q)
    return M.score_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])


def _check(logp, resp, truth, what):
    lp, rs, bar_lp, bar_rs, e_lp, e_rs = truth
    if logp is not None:
        e = T.rel_err(logp, lp)
        parity_log.record('rel', e, bar_lp, '%s logp (fp32 restatement: %.2e)' % (what, e_lp))
        print('%s logp: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, e, e_lp, bar_lp))
        assert e <= bar_lp, (what, 'logp', e, bar_lp, e_lp)
    if resp is not None:
        e = T.abs_err(resp, rs)
        parity_log.record('abs', e, bar_rs, '%s resp (fp32 restatement: %.2e)' % (what, e_rs))
        print('%s resp: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, e, e_rs, bar_rs))
        assert e <= bar_rs, (what, 'resp', e, bar_rs, e_rs)
        assert (resp.double().sum(1) - 1).abs().max().item() < 1e-6, what


@pytest.mark.parametrize('builder', ['t', 'niw'])
@pytest.mark.parametrize('N,D,K', SWEEP)
def test_shape_sweep(N, D, K, builder):
    M = _mix()
    x, t, q, truth_t, truth_q = _case(N, D, K)
    truth = truth_t if builder == 't' else truth_q
    xd = torch.as_tensor(x).cuda()
    pack = _pack(builder, t, q)
    assert tuple(pack.shape) == (K, D + D * (D + 1) // 2 + 4) and torch.isfinite(pack).all()
    what = '%s N=%d D=%d K=%d' % (builder, N, D, K)
    logp, resp, total = M.mixture_score(xd, pack, want_logp=True, want_resp=True, want_sum=True)
    assert logp.shape == (N,) and resp.shape == (N, K) and total.shape == () and total.dtype == torch.float64
    _check(logp, resp, truth, what)
    # each output alone: the same bits
    l1, r1, s1 = M.mixture_score(xd, pack, want_logp=True, want_resp=False, want_sum=False)
    assert r1 is None and s1 is None and torch.equal(l1, logp)
    l2, r2, s2 = M.mixture_score(xd, pack, want_logp=False, want_resp=True, want_sum=False)
    assert l2 is None and s2 is None and torch.equal(r2, resp)
    l3, r3, s3 = M.mixture_score(xd, pack, want_logp=False, want_resp=False, want_sum=True)
    assert l3 is None and r3 is None and torch.equal(s3, total)                  # unchanged by the other outputs
    _, _, s4 = M.mixture_score(xd, pack, want_logp=True, want_resp=True, want_sum=True)
    assert torch.equal(s4, total)                                                # bit-identical across two calls
    want = logp.double().sum().item()
    assert abs(total.item() - want) <= 1e-12 * abs(want), (what, total.item(), want)


@pytest.mark.parametrize('D', [3, 5, 2, 8])
def test_unaligned_x_gives_the_same_bits(D):
    """a view offset by one float: the scalar-load path (vec_ok = 0) against the aligned copy"""
    M = _mix()
    N, K = 257, 17
    x, t, q, _, _ = _case(N, D, K)
    pack = _pack('t', t, q)
    xa = torch.as_tensor(x).cuda()
    buf = torch.empty(N * D + 4, dtype=torch.float32, device='cuda')
    xu = buf[1:1 + N * D].view(N, D)
    xu.copy_(xa)
    assert xa.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    a = M.mixture_score(xa, pack, want_resp=True)
    b = M.mixture_score(xu, pack, want_resp=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _t_params(D, K, seed=3):
    x, t, _ = T.make_case(300, D, K, seed)
    return x, {k: a.copy() for k, a in t.items()}


def test_one_component_with_log_pi_minus_inf_is_ignored():
    from vmp_for_svae_amd.distributions import student_t
    x, t = _t_params(3, 5)
    t['log_w'][2] = -np.inf
    c = _cuda(t)
    logp, resp = student_t.mixture_logprob(torch.as_tensor(x).cuda(), c['mu'], c['sigma'], c['nu'], c['log_w'], return_resp=True)
    assert torch.isfinite(logp).all() and torch.isfinite(resp).all()
    assert (resp[:, 2] == 0).all()
    keep = [0, 1, 3, 4]
    sub = {k: a[keep] for k, a in t.items()}
    truth = T.bars(x, T.pack_t(**sub))
    _check(logp, resp[:, keep], truth, 'log_pi[2] = -inf')


def test_all_components_minus_inf_gives_minus_inf_and_no_nan():
    M = _mix()
    x, t = _t_params(2, 17)
    t['log_w'][:] = -np.inf
    c = _cuda(t)
    pack = M.score_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    logp, resp, total = M.mixture_score(torch.as_tensor(x).cuda(), pack, want_resp=True)
    assert (logp == -math.inf).all() and not torch.isnan(logp).any()
    assert not torch.isnan(resp).any() and (resp == 0).all()
    assert total.item() == -math.inf


def test_a_row_1e4_scale_lengths_away_is_finite():
    M = _mix()
    x, t = _t_params(5, 3)
    scale = np.sqrt(np.linalg.eigvalsh(t['sigma'].astype(np.float64)).max())
    x = x.copy()
    x[7] = t['mu'][0] + 1e4 * scale * np.ones(5, np.float32) / math.sqrt(5)
    x[8] = -x[7]
    c = _cuda(t)
    pack = M.score_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    logp, resp, total = M.mixture_score(torch.as_tensor(x).cuda(), pack, want_resp=True)
    assert torch.isfinite(logp).all() and torch.isfinite(resp).all() and math.isfinite(total.item())
    assert logp[7].item() < -30 and logp[8].item() < -30
    _check(logp, resp, T.bars(x, T.pack_t(**t)), 'far rows')


def test_non_spd_sigma_gives_nan_rows_and_nothing_else():
    M = _mix()
    x, t = _t_params(3, 4)
    good = _cuda(t)
    t['sigma'][1] = np.diag([1.0, -1.0, 1.0]).astype(np.float32)
    c = _cuda(t)
    pack = M.score_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    assert torch.isnan(pack[1, 3:-1]).all() and torch.isfinite(pack[[0, 2, 3]]).all()
    xd = torch.as_tensor(x).cuda()
    logp, resp, total = M.mixture_score(xd, pack, want_resp=True)
    assert torch.isnan(logp).all() and math.isnan(total.item())
    # the same call with the good parameters right after: finite - the NaN stayed in the values
    logp2, _, _ = M.mixture_score(xd, M.score_pack_t(good['log_w'], good['mu'], good['sigma'], good['nu']))
    assert torch.isfinite(logp2).all()


def test_niw_with_non_positive_predictive_dof_gives_nan():
    from vmp_for_svae_amd.models import gmm
    D, K = 3, 4
    x, _, q = T.make_case(100, D, K, 5)
    q = {k: a.copy() for k, a in q.items()}
    q['v'][2] = D - 1.5                                   # nu' = v + 1 - D = -0.5
    c = _cuda(q)
    pack = _mix().score_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])
    assert torch.isnan(pack[2, D:-1]).all() and torch.isfinite(pack[[0, 1, 3]]).all()
    logp, total = gmm.predictive_logprob(torch.as_tensor(x).cuda(), c['alpha'], c['beta'], c['m'], c['C'], c['v'])
    assert torch.isnan(logp).all() and math.isnan(total.item())
    q['v'][2] = D - 1.0                                   # nu' = 0: not a density either
    c = _cuda(q)
    assert torch.isnan(_mix().score_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])[2, D:-1]).all()


# ---- Python surface -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,D,K', [(257, 3, 5), (4099, 8, 16), (65, 5, 33)])
def test_mixture_logprob_equals_logsumexp_of_logprob_smm_mixture(N, D, K):
    from vmp_for_svae_amd.distributions import student_t
    x, t, q, truth, _ = _case(N, D, K)
    c = _cuda(t)
    xd = torch.as_tensor(x).cuda()
    new = student_t.mixture_logprob(xd, c['mu'], c['sigma'], c['nu'], c['log_w'])
    old = torch.logsumexp(student_t.logprob_smm_mixture(xd, c['mu'], c['sigma'], c['nu'], c['log_w']), dim=1)
    assert new.shape == (N,) and new.dtype == torch.float32
    bar = truth[2]
    e = T.rel_err(new, old)
    parity_log.record('rel', e, bar, 'mixture_logprob vs logsumexp(logprob_smm_mixture) N=%d D=%d K=%d' % (N, D, K))
    assert e <= bar, (e, bar)
    _check(new, None, truth, 'mixture_logprob N=%d D=%d K=%d' % (N, D, K))
    lp2, resp = student_t.mixture_logprob(xd, c['mu'], c['sigma'], c['nu'], c['log_w'], return_resp=True)
    assert torch.equal(lp2, new)
    _check(None, resp, truth, 'mixture_logprob resp N=%d D=%d K=%d' % (N, D, K))


def _tiny(seed=0, N=60, D=2, K=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((K, D)) * 4
    x = (c[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)
    r0 = np.exp(rng.standard_normal((N, K)))
    return x, (r0 / r0.sum(1, keepdims=True)).astype(np.float32)


def _cpu64(ts):
    return [t.detach().double().cpu() for t in ts]


def test_gmm_predictive_logprob_on_the_theta_of_a_loop():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import gmm
    M = _mix()
    x, r0 = _tiny()
    N, D = x.shape
    K = r0.shape[1]
    xd = torch.as_tensor(x).cuda()
    loop = M.VMPLoop(xd, torch.as_tensor(r0).cuda(), V._lib.VMP_GMM)
    with pytest.raises(V._lib.VmpError, match='iteration'):
        loop.score(xd)
    for _ in range(3):
        loop.step()
    theta = loop.theta()
    al, be, m, C, v = _cpu64(theta)
    # the default prior cannot reach the NaN branch: nu' = v_k + 1 - D >= D + 1.5 + N_k
    Nk = loop.r.double().sum(0).cpu()
    assert ((v + 1 - D) >= D + 1.5).all() and ((v + 1 - D) > 0).all() and (Nk >= 0).all()
    truth = T.bars(x, T.pack_niw(al, be, m, C, v))
    logp, total, resp = gmm.predictive_logprob(xd, *theta, return_resp=True)
    assert total.is_cuda and total.dtype == torch.float64 and total.dim() == 0
    _check(logp, resp, truth, 'gmm.predictive_logprob on theta()')
    lp2, tot2 = gmm.predictive_logprob(xd, *theta)
    assert torch.equal(lp2, logp) and torch.equal(tot2, total)
    assert loop.score(xd) == total.item() / N
    assert abs(loop.score(xd) - truth[0].mean().item()) <= truth[2] * max(1.0, truth[0].abs().max().item())


def test_smm_heldout_logprob_and_loop_score():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import smm
    M = _mix()
    x, r0 = _tiny(seed=1)
    N, D = x.shape
    K = r0.shape[1]
    xd = torch.as_tensor(x).cuda()
    kappa = torch.full((K,), 5.0, device='cuda')
    loop = M.VMPLoop(xd, torch.as_tensor(r0).cuda(), V._lib.VMP_SMM, kappa=kappa)
    loop.run(3)
    theta = loop.theta()
    al, be, m, C, v = _cpu64(theta)
    truth = T.bars(x, T.pack_t(torch.log(al / al.sum()), m, C / v[:, None, None], kappa.double().cpu()))
    logp, total, resp = smm.heldout_logprob(xd, *theta, kappa, return_resp=True)
    _check(logp, resp, truth, 'smm.heldout_logprob on theta()')
    assert loop.score(xd) == total.item() / N


def test_run_until_stops_on_two_clusters():
    import vmp_for_svae_amd as V
    M = _mix()
    rng = np.random.Generator(np.random.PCG64(7))
    N, K = 512, 4
    centres = np.array([[-6.0, 0.0], [6.0, 0.0]])
    draw = lambda n: (centres[rng.integers(0, 2, n)] + rng.standard_normal((n, 2))).astype(np.float32)
    x, x_val = draw(N), draw(256)
    r0 = np.exp(rng.standard_normal((N, K)))
    r0 = (r0 / r0.sum(1, keepdims=True)).astype(np.float32)
    loop = M.VMPLoop(torch.as_tensor(x).cuda(), torch.as_tensor(r0).cuda(), V._lib.VMP_GMM)
    hist = loop.run_until(torch.as_tensor(x_val).cuda(), tol=1e-4, check_every=5, max_iterations=1000)
    assert 2 <= len(hist) < 200, len(hist)                       # stopped before max_iterations = 200 checks
    assert [it for it, _ in hist] == [5 * (i + 1) for i in range(len(hist))]
    assert loop.iterations == hist[-1][0] < 1000
    assert all(math.isfinite(s) for _, s in hist)
    assert hist[-1][1] >= hist[0][1]
    assert hist[-1][1] - hist[-2][1] < 1e-4
    # a cap that is no multiple of check_every: the last leg is shorter and the count exact
    loop2 = M.VMPLoop(torch.as_tensor(x).cuda(), torch.as_tensor(r0).cuda(), V._lib.VMP_GMM)
    h2 = loop2.run_until(torch.as_tensor(x_val).cuda(), tol=-math.inf, check_every=5, max_iterations=12)
    assert [it for it, _ in h2] == [5, 10, 12] and loop2.iterations == 12
