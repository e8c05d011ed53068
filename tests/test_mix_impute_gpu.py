"""Mixture imputation on the GPU (csrc/vmp_impute.hip): the two pack builders and the streaming impute kernel against the fp64
truth of tests/mix_impute_truth.py, over a shape sweep that crosses the 64-row tile edge, ragged tails and the 16-component tile
edges; each output alone; the deterministic row sum; in-place filling; unaligned x; NaN / Inf in the missing slots; the all-observed,
all-missing, -inf-weight, far-row and NaN-parameter edge cases; and the Python surface (student_t.mixture_impute,
gmm.predictive_impute, smm.heldout_impute, VMPLoop.impute).

Tolerance (never a constant found on the kernel): bar = max(1e-5, 3 x the error of the op-for-op fp32 torch-CPU restatement against
the fp64 truth on the same inputs) - relative to max(1, |value|) for logp and x_out, absolute for resp.  Achieved errors and bars go
to the parity log (tests/parity_log.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import mix_impute_truth as T
import mix_score_truth as S
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
    """inputs, mask, both truth packs' results and their bars: computed once, shared, never modified"""
    seed = 1000 * D + 10 * K + N % 7
    x, t, q = S.make_case(N, D, K, seed=seed)
    miss = T.make_mask(N, D, seed + 1)
    return x, miss, t, q, T.bars(x, miss, T.pack_t(**t)), T.bars(x, miss, T.pack_niw(**q))


def _pack(builder, t, q):
    M = _mix()
    if builder == 't':
        c = _cuda(t)
        return M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    c = _cuda(q)
    return M.impute_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])


def _check(x_out, logp, resp, truth, what):
    for name, got, err, unit in (('logp', logp, S.rel_err, 'rel'), ('resp', resp, S.abs_err, 'abs'), ('x_out', x_out, S.rel_err, 'rel')):
        if got is None:
            continue
        key = {'logp': 'logp', 'resp': 'resp', 'x_out': 'x'}[name]
        e, e32, bar = err(got, truth[name]), truth['e_' + key], truth['bar_' + key]
        parity_log.record(unit, e, bar, '%s %s (fp32 restatement: %.2e)' % (what, name, e32))
        print('%s %s: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, name, e, e32, bar))
        assert e <= bar, (what, name, e, bar, e32)
    if resp is not None:
        assert (resp.double().sum(1) - 1).abs().max().item() < 1e-6, what


def _observed_bits_kept(x_out, x, miss):
    o = torch.as_tensor(miss == 0)
    return torch.equal(x_out.cpu().view(torch.int32)[o], torch.as_tensor(x).view(torch.int32)[o])


@pytest.mark.parametrize('builder', ['t', 'niw'])
@pytest.mark.parametrize('N,D,K', SWEEP)
def test_shape_sweep(N, D, K, builder):
    M = _mix()
    x, miss, t, q, truth_t, truth_q = _case(N, D, K)
    truth = truth_t if builder == 't' else truth_q
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    pack = _pack(builder, t, q)
    assert tuple(pack.shape) == (K, 2 * D + D * (D + 1) // 2 + 5) and torch.isfinite(pack).all()
    what = '%s N=%d D=%d K=%d' % (builder, N, D, K)
    x_out, logp, resp, total = M.mixture_impute(xd, md, pack, want_resp=True, want_sum=True)
    assert x_out.shape == (N, D) and logp.shape == (N,) and resp.shape == (N, K) and total.shape == () and total.dtype == torch.float64
    assert x_out.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.as_tensor(x))
    _check(x_out, logp, resp, truth, what)
    assert _observed_bits_kept(x_out, x, miss), what
    # each output alone: the same bits
    for i in range(4):
        want = [j == i for j in range(4)]
        got = M.mixture_impute(xd, md, pack, want_x=want[0], want_logp=want[1], want_resp=want[2], want_sum=want[3])
        for j, (g, full) in enumerate(zip(got, (x_out, logp, resp, total))):
            assert (g is None) if j != i else torch.equal(g, full), (what, i, j)
    s2 = M.mixture_impute(xd, md, pack, want_resp=True, want_sum=True)[3]
    assert torch.equal(s2, total)                                                # bit-identical across two calls
    want = logp.double().sum().item()
    assert abs(total.item() - want) <= 1e-12 * abs(want), (what, total.item(), want)
    # a bool mask is the same mask
    assert torch.equal(M.mixture_impute(xd, md != 0, pack)[0], x_out)


@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (65, 3, 17), (4099, 2, 16)])
def test_inplace_gives_the_bits_of_the_out_of_place_call(N, D, K):
    M = _mix()
    x, miss, t, q, _, _ = _case(N, D, K)
    pack = _pack('t', t, q)
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    a = M.mixture_impute(xd, md, pack, want_resp=True, want_sum=True)
    xi = xd.clone()
    b = M.mixture_impute(xi, md, pack, want_resp=True, want_sum=True, inplace=True)
    assert b[0] is xi and b[0].data_ptr() == xi.data_ptr()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('D', [3, 5, 2, 8])
def test_unaligned_x_gives_the_same_bits(D):
    """a view offset by one float: the scalar load / store path against the aligned copy"""
    M = _mix()
    N, K = 257, 17
    x, miss, t, q, _, _ = _case(N, D, K)
    pack = _pack('t', t, q)
    xa, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    buf = torch.empty(N * D + 4, dtype=torch.float32, device='cuda')
    xu = buf[1:1 + N * D].view(N, D)
    xu.copy_(xa)
    assert xa.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    a = M.mixture_impute(xa, md, pack, want_resp=True, want_sum=True)
    b = M.mixture_impute(xu, md, pack, want_resp=True, want_sum=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    c = M.mixture_impute(xu, md, pack, inplace=True)                          # unaligned output as well
    assert c[0].data_ptr() == xu.data_ptr() and torch.equal(c[0], a[0])


@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (257, 3, 33)])
def test_nan_and_inf_in_the_missing_slots_change_nothing(N, D, K):
    M = _mix()
    x, miss, t, q, _, _ = _case(N, D, K)
    pack = _pack('niw', t, q)
    md = torch.as_tensor(miss).cuda()
    outs = []
    for fill in (0.0, math.nan, math.inf, -math.inf):
        xf = x.copy()
        xf[miss != 0] = fill
        outs.append(M.mixture_impute(torch.as_tensor(xf).cuda(), md, pack, want_resp=True, want_sum=True))
    for o in outs:
        assert all(torch.isfinite(v).all() for v in o)
    for o in outs[1:]:
        for u, v in zip(outs[0], o):
            assert torch.equal(u, v)


@pytest.mark.parametrize('builder', ['t', 'niw'])
@pytest.mark.parametrize('N,D,K', [(257, 8, 3), (4099, 3, 64)])
def test_all_observed_input_agrees_with_mixture_score(N, D, K, builder):
    M = _mix()
    x, _, t, q, _, _ = _case(N, D, K)
    xd = torch.as_tensor(x).cuda()
    none = torch.zeros(N, D, dtype=torch.uint8, device='cuda')
    x_out, logp, resp, _ = M.mixture_impute(xd, none, _pack(builder, t, q), want_resp=True)
    assert torch.equal(x_out, xd)
    c = _cuda(t if builder == 't' else q)
    spack = M.score_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu']) if builder == 't' else M.score_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])
    slogp, sresp, _ = M.mixture_score(xd, spack, want_resp=True)
    truth = T.bars(x, np.zeros((N, D), np.uint8), T.pack_t(**t) if builder == 't' else T.pack_niw(**q))
    what = 'all observed %s N=%d D=%d K=%d' % (builder, N, D, K)
    _check(None, logp, resp, truth, what)
    e_lp, e_rs = S.rel_err(logp, slogp.double().cpu()), S.abs_err(resp, sresp)
    parity_log.record('rel', e_lp, truth['bar_logp'], what + ' logp vs mixture_score')
    parity_log.record('abs', e_rs, truth['bar_resp'], what + ' resp vs mixture_score')
    assert e_lp <= truth['bar_logp'] and e_rs <= truth['bar_resp'], (e_lp, e_rs, truth['bar_logp'], truth['bar_resp'])


def test_all_missing_rows_give_the_closed_form():
    M = _mix()
    N, D, K = 65, 5, 33
    x, _, t, q, _, _ = _case(N, D, K)
    gone = torch.ones(N, D, dtype=torch.uint8, device='cuda')
    x_out, logp, resp, _ = M.mixture_impute(torch.full((N, D), math.nan, device='cuda'), gone, _pack('t', t, q), want_resp=True)
    lw, mu = torch.as_tensor(t['log_w']).double(), torch.as_tensor(t['mu']).double()
    w = torch.softmax(lw, 0)
    truth = T.bars(x, np.ones((N, D), np.uint8), T.pack_t(**t))
    assert S.rel_err(truth['logp'], torch.logsumexp(lw, 0).expand(N)) <= 1e-12 and S.rel_err(truth['x_out'], (w @ mu).expand(N, D)) <= 1e-12
    _check(x_out, logp, resp, truth, 'all missing N=%d D=%d K=%d' % (N, D, K))
    assert S.abs_err(resp, w.expand(N, K)) <= truth['bar_resp']


def _t_params(D, K, seed=3, N=300):
    x, t, q = S.make_case(N, D, K, seed)
    return x, T.make_mask(N, D, seed + 1), {k: a.copy() for k, a in t.items()}, {k: a.copy() for k, a in q.items()}


def test_one_component_with_log_pi_minus_inf_is_ignored():
    from vmp_for_svae_amd.distributions import student_t
    x, miss, t, _ = _t_params(3, 5)
    t['log_w'][2] = -np.inf
    c = _cuda(t)
    x_out, logp, resp = student_t.mixture_impute(torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda(), c['mu'], c['sigma'], c['nu'],
                                                 c['log_w'], return_resp=True)
    assert torch.isfinite(logp).all() and torch.isfinite(resp).all() and torch.isfinite(x_out).all()
    assert (resp[:, 2] == 0).all()
    keep = [0, 1, 3, 4]
    truth = T.bars(x, miss, T.pack_t(**{k: a[keep] for k, a in t.items()}))
    _check(x_out, logp, resp[:, keep], truth, 'log_pi[2] = -inf')


def test_all_components_minus_inf_gives_minus_inf_zeros_and_no_nan():
    M = _mix()
    x, miss, t, _ = _t_params(2, 17)
    t['log_w'][:] = -np.inf
    c = _cuda(t)
    pack = M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    x_out, logp, resp, total = M.mixture_impute(torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda(), pack, want_resp=True, want_sum=True)
    assert (logp == -math.inf).all() and (resp == 0).all() and total.item() == -math.inf
    assert not torch.isnan(x_out).any() and (x_out.cpu()[torch.as_tensor(miss != 0)] == 0).all()
    assert _observed_bits_kept(x_out, x, miss)


def test_a_row_1e4_scale_lengths_away_is_finite():
    M = _mix()
    D = 6
    x, miss, t, _ = _t_params(D, 3)
    scale = np.sqrt(np.linalg.eigvalsh(t['sigma'].astype(np.float64)).max())
    x, miss = x.copy(), miss.copy()
    x[7] = t['mu'][0] + 1e4 * scale * np.ones(D, np.float32) / math.sqrt(D)
    x[8] = -x[7]
    miss[7] = miss[8] = np.array([1, 0, 1, 0, 1, 0], np.uint8)           # half of the entries missing
    c = _cuda(t)
    pack = M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    x_out, logp, resp, total = M.mixture_impute(torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda(), pack, want_resp=True, want_sum=True)
    assert torch.isfinite(x_out).all() and torch.isfinite(logp).all() and torch.isfinite(resp).all() and math.isfinite(total.item())
    assert logp[7].item() < -30 and logp[8].item() < -30
    _check(x_out, logp, resp, T.bars(x, miss, T.pack_t(**t)), 'far rows')


def test_non_spd_sigma_gives_nan_rows_and_nothing_else():
    M = _mix()
    x, miss, t, _ = _t_params(3, 4)
    good = _cuda(t)
    t['sigma'][1] = np.diag([1.0, -1.0, 1.0]).astype(np.float32)
    c = _cuda(t)
    pack = M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    assert torch.isnan(pack[1]).all() and torch.isfinite(pack[[0, 2, 3]]).all()             # the whole pack row, mu included
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    x_out, logp, _, total = M.mixture_impute(xd, md, pack, want_sum=True)
    assert torch.isnan(logp).all() and math.isnan(total.item())
    assert _observed_bits_kept(x_out, x, miss)
    # the same call with the good parameters right after: finite - the NaN stayed in the values
    x2, logp2, _, _ = M.mixture_impute(xd, md, M.impute_pack_t(good['log_w'], good['mu'], good['sigma'], good['nu']))
    assert torch.isfinite(logp2).all() and torch.isfinite(x2).all()


def test_niw_with_non_positive_predictive_dof_gives_nan():
    from vmp_for_svae_amd.models import gmm
    D, K = 3, 4
    x, miss, _, q = _t_params(D, K, seed=5, N=100)
    good = _cuda(q)
    q['v'][2] = D - 1.5                                   # nu' = v + 1 - D = -0.5
    c = _cuda(q)
    pack = _mix().impute_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])
    assert torch.isnan(pack[2]).all() and torch.isfinite(pack[[0, 1, 3]]).all()
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    _, logp = gmm.predictive_impute(xd, md, c['alpha'], c['beta'], c['m'], c['C'], c['v'])
    assert torch.isnan(logp).all()
    q['v'][2] = D - 1.0                                   # nu' = 0: not a density either
    c = _cuda(q)
    assert torch.isnan(_mix().impute_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])[2]).all()
    x2, logp2 = gmm.predictive_impute(xd, md, good['alpha'], good['beta'], good['m'], good['C'], good['v'])
    assert torch.isfinite(logp2).all() and torch.isfinite(x2).all()


def test_a_pack_of_the_wrong_kind_device_or_type_is_refused_on_the_host():
    """score packs are narrower than impute packs: either kernel would read past the end of the other's pack"""
    import vmp_for_svae_amd as V
    M = _mix()
    E = V._lib.VmpError
    N, D, K = 65, 3, 17
    x, miss, t, q, _, _ = _case(N, D, K)
    c = _cuda(t)
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    ipack = M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    spack = M.score_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    assert ipack.shape[1] != spack.shape[1]
    with pytest.raises(E, match='pack has shape'):
        M.mixture_impute(xd, md, spack)
    with pytest.raises(E, match='pack has shape'):
        M.mixture_score(xd, ipack)
    with pytest.raises(E, match='float32'):
        M.mixture_impute(xd, md, ipack.double())
    with pytest.raises(E, match='cpu'):
        M.mixture_impute(xd, md, ipack.cpu())
    with pytest.raises(E, match='mask is on cpu'):
        M.mixture_impute(xd, md.cpu(), ipack)
    with pytest.raises(E, match='pack must be'):
        M.mixture_impute(xd, md, ipack[0])


# ---- Python surface -----------------------------------------------------------------------------------------------------
def _tiny(seed=0, N=60, D=2, K=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((K, D)) * 4
    x = (c[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)
    r0 = np.exp(rng.standard_normal((N, K)))
    return x, (r0 / r0.sum(1, keepdims=True)).astype(np.float32), T.make_mask(N, D, seed + 100)


def _cpu64(ts):
    return [t.detach().double().cpu() for t in ts]


def test_gmm_predictive_impute_and_loop_impute():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import gmm
    M = _mix()
    x, r0, miss = _tiny()
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    loop = M.VMPLoop(xd, torch.as_tensor(r0).cuda(), V._lib.VMP_GMM)
    with pytest.raises(V._lib.VmpError, match='iteration'):
        loop.impute(xd, md)
    for _ in range(3):
        loop.step()
    theta = loop.theta()
    truth = T.bars(x, miss, T.pack_niw(*_cpu64(theta)))
    x_out, logp, resp = gmm.predictive_impute(xd, md, *theta, return_resp=True)
    _check(x_out, logp, resp, truth, 'gmm.predictive_impute on theta()')
    x2, lp2 = gmm.predictive_impute(xd, md, *theta)
    assert torch.equal(x2, x_out) and torch.equal(lp2, logp)
    x3, lp3 = loop.impute(xd, md)
    assert torch.equal(x3, x_out) and torch.equal(lp3, logp)
    with pytest.raises(V._lib.VmpError, match='shape|must be'):
        loop.impute(xd, md[:, :1])


def test_smm_heldout_impute_student_t_mixture_impute_and_loop_impute():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import smm
    M = _mix()
    x, r0, miss = _tiny(seed=1)
    K = r0.shape[1]
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    kappa = torch.full((K,), 5.0, device='cuda')
    loop = M.VMPLoop(xd, torch.as_tensor(r0).cuda(), V._lib.VMP_SMM, kappa=kappa)
    with pytest.raises(V._lib.VmpError, match='iteration'):
        loop.impute(xd, md)
    loop.run(3)
    theta = loop.theta()
    al, be, m, C, v = _cpu64(theta)
    truth = T.bars(x, miss, T.pack_t(torch.log(al / al.sum()), m, C / v[:, None, None], kappa.double().cpu()))
    x_out, logp, resp = smm.heldout_impute(xd, md, *theta, kappa, return_resp=True)
    _check(x_out, logp, resp, truth, 'smm.heldout_impute on theta()')
    x3, lp3 = loop.impute(xd, md)
    assert torch.equal(x3, x_out) and torch.equal(lp3, logp)
    a_, _, m_, C_, v_ = theta
    y_out, lp4, rs4 = student_t.mixture_impute(xd, md, m_, C_ / v_[:, None, None], kappa, torch.log(a_ / a_.sum()), return_resp=True)
    _check(y_out, lp4, rs4, truth, 'student_t.mixture_impute on theta()')
    assert torch.equal(y_out, x_out) and torch.equal(lp4, logp) and torch.equal(rs4, resp)
