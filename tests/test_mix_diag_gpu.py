"""The diagonal-covariance Gaussian mixture fit on the GPU (csrc/vmp_diagfit.hip, models/_diag.py, gmm.inference_diag /
lower_bound_diag) against the fp64 truth of tests/mix_diag_truth.py: the pass and the loop over a shape sweep (D on both sides of 16 /
32 / 48 and at 64, K on both sides of 16 / 32 and at 64, N not a multiple of 4, below and above a wave's flush interval of 128 rows),
the same with all data offset by +1000, bit identity, iterate against steps, the r_in form, unaligned x, the monotone bound, the
nearest-centre start and the Python surface.

Tolerance (never a constant found on the kernel): per case and per quantity bar = max(1e-5, 3 x the error of the same functions run
in fp32 against fp64, from the same inputs for the same number of iterations) - absolute for r, relative to max(1, |value|) for
everything else.  Achieved errors and bars go to the parity log."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import mix_diag_truth as T
import parity_log

pytestmark = pytest.mark.gpu

SWEEP = [(300, 1, 2), (130, 9, 1), (257, 17, 3), (65, 5, 64), (129, 49, 5), (4099, 16, 16), (1031, 33, 33), (513, 64, 16), (2051, 64, 64)]


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _cuda(a):
    return torch.as_tensor(np.asarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _data(N, D, K, offset=0.0):
    x, r0 = T.make_data(N, D, K, 100 * D + 7 * K + N % 11, offset)
    return x, r0, T.default_prior(x, K)


@functools.lru_cache(maxsize=None)
def _case(N, D, K, iterations, offset=0.0):
    """inputs and the truth with its bars: computed once, shared, never modified"""
    x, r0, prior = _data(N, D, K, offset)
    return x, r0, prior, T.bars(x, r0, prior, iterations)


def _loop(x, r0, prior):
    return _mix().DiagLoop(_cuda(x), _cuda(r0), prior=[_cuda(p) for p in prior])


def _state(loop):
    return dict(r=loop.r, logr=loop.logr, stats=loop.stats, theta=loop.theta(), data=loop._data.item(), bound=loop.lower_bound())


def _check(what, truth, got):
    bad = []
    for name, e in T.errors(got, truth).items():
        bar, e32 = truth['bar_' + name], truth['e_' + name]
        parity_log.record('abs' if name == 'r' else 'rel', e, bar, '%s %s (fp32 restatement: %.2e)' % (what, name, e32))
        print('%s %s: kernel %.3e  fp32 restatement %.3e  bar %.3e' % (what, name, e, e32, bar))
        if not e <= bar:
            bad.append((name, e, bar, e32))
    assert not bad, (what, bad)


def _bits(t):
    return None if t is None else t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _one_and_three(N, D, K, offset=0.0):
    x, r0, prior, truth1 = _case(N, D, K, 1, offset)
    truth3 = _case(N, D, K, 3, offset)[3]
    what = 'N=%d D=%d K=%d%s' % (N, D, K, ' offset %g' % offset if offset else '')
    loop = _loop(x, r0, prior)
    r = loop.step(want_logr=True)
    assert r.shape == (N, K) and (r.double().sum(1) - 1).abs().max().item() < 1e-6
    st = _state(loop)
    assert torch.isfinite(st['stats']).all() and math.isfinite(st['data']) and math.isfinite(st['bound'])
    _check('1 iteration ' + what, truth1, st)
    # the pass through its wrapper is the loop's own pass
    got = _mix().mixture_diag_pass(loop.x, loop.pack, want_logr=True, want_bound=True)
    for u, v in zip(got, (loop.r, loop.logr, loop.stats, loop._data)):
        assert torch.equal(_bits(u), _bits(v))
    loop.run(2)
    assert loop.iterations == 3
    _check('3 iterations ' + what, truth3, _state(loop))


@pytest.mark.parametrize('N,D,K', SWEEP)
def test_pass_and_three_iterations_shape_sweep(N, D, K):
    _one_and_three(N, D, K)


def test_data_offset_by_1000():
    """raw un-shifted fp32 moments lose sxx - sx^2 / Nk here (1e6 against 1); the shifted ones do not"""
    _one_and_three(1031, 33, 33, 1000.0)


@pytest.mark.parametrize('N,D,K', [(1031, 33, 33), (513, 64, 16)])
def test_bit_identity_across_runs_and_every_output_set(N, D, K):
    M = _mix()
    x, r0, prior = _data(N, D, K)
    loop = _loop(x, r0, prior)
    loop.step()
    full = M.mixture_diag_pass(loop.x, loop.pack, want_r=True, want_logr=True, want_stats=True, want_bound=True)
    assert torch.isfinite(full[2]).all() and torch.isfinite(full[3])
    again = M.mixture_diag_pass(loop.x, loop.pack, want_r=True, want_logr=True, want_stats=True, want_bound=True)
    for u, v in zip(full, again):
        assert torch.equal(_bits(u), _bits(v))
    sets = 0
    for want in itertools.product((False, True), repeat=4):
        want_r, want_logr, want_stats, want_bound = want
        if not any(want) or (want_logr and not want_r):
            continue
        part = M.mixture_diag_pass(loop.x, loop.pack, want_r=want_r, want_logr=want_logr, want_stats=want_stats, want_bound=want_bound)
        for asked, u, v in zip(want, part, full):
            assert (u is None) if not asked else torch.equal(_bits(u), _bits(v)), want
        sets += 1
    assert sets == 11


@pytest.mark.parametrize('N,D,K', [(4099, 16, 16), (513, 64, 16), (1031, 33, 33)])
def test_iterate_3_is_three_steps(N, D, K):
    x, r0, prior = _data(N, D, K)
    a, b = _loop(x, r0, prior), _loop(x, r0, prior)
    a.run(3)
    for _ in range(3):
        b.step(want_logr=True)
    assert a.iterations == b.iterations == 3
    assert torch.equal(_bits(a.stats), _bits(b.stats)) and torch.equal(_bits(a._data), _bits(b._data))
    for u, v in zip(a.theta() + a.aux(), b.theta() + b.aux()):
        assert torch.equal(u, v)
    assert a.lower_bound() == b.lower_bound()
    assert torch.equal(a.r, b.r) and torch.equal(a.logr, b.logr)          # produced by one pass on demand


@pytest.mark.parametrize('N,D,K', [(4099, 16, 16), (129, 49, 5), (2051, 64, 64)])
def test_r_in_form_gives_the_moments_of_a_supplied_r(N, D, K):
    x, r0, prior = _data(N, D, K)
    want = T.raw_stats(*T.moments(x, r0, torch.float64))
    e32 = T.rel_err(T.raw_stats(*T.moments(x, r0, torch.float32)), want)
    bar = max(1e-5, 3 * e32)
    xd, rd = torch.as_tensor(x).double(), torch.as_tensor(r0).double()
    direct = torch.cat([rd.sum(0)[:, None], rd.t() @ xd, rd.t() @ (xd * xd)], 1)
    assert T.rel_err(direct, want) < 1e-12
    pack = torch.zeros(K, 2 * D + 1, device='cuda')
    got = _mix().mixture_diag_pass(_cuda(x), pack, r_in=_cuda(r0), want_r=False)
    assert got[0] is None and got[1] is None and got[3] is None
    e = T.rel_err(got[2], direct)
    parity_log.record('rel', e, bar, 'r_in stats N=%d D=%d K=%d (fp32 restatement: %.2e)' % (N, D, K, e32))
    assert e <= bar, (e, bar)


@pytest.mark.parametrize('N,D,K', [(257, 17, 3), (513, 64, 16), (65, 5, 64)])
def test_unaligned_x_gives_the_same_bits(N, D, K):
    """x a view offset by one float: not 16-byte aligned"""
    x, r0, prior = _data(N, D, K)
    a = _loop(x, r0, prior)
    a.run(2)
    buf = torch.empty(N * D + 8, dtype=torch.float32, device='cuda')
    xu = buf[1:1 + N * D].view(N, D)
    xu.copy_(_cuda(x))
    assert a.x.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    b = _mix().DiagLoop(xu, _cuda(r0), prior=[_cuda(p) for p in prior])
    assert b.x.data_ptr() == xu.data_ptr()
    b.run(2)
    assert torch.equal(_bits(a.stats), _bits(b.stats)) and torch.equal(_bits(a._data), _bits(b._data)) and torch.equal(a.r, b.r)


@pytest.mark.parametrize('N,D,K,offset', [(1031, 33, 33, 0.0), (1031, 33, 33, 1000.0), (513, 64, 16, 0.0)])
def test_device_bound_does_not_fall_over_20_iterations(N, D, K, offset):
    x, r0, prior = _data(N, D, K, offset)
    loop = _loop(x, r0, prior)
    bounds = []
    for _ in range(20):
        loop.run(1)
        bounds.append(loop.lower_bound())
    assert all(math.isfinite(b) for b in bounds)
    for u, v in zip(bounds, bounds[1:]):
        assert v >= u - 1e-6 * max(1.0, abs(u)), bounds


def test_from_centers_recovers_planted_clusters():
    N, D, K = 600, 24, 4
    rng = np.random.Generator(np.random.PCG64(11))
    centres = np.zeros((K, D))
    centres[np.arange(K), np.arange(K)] = 12.0 / math.sqrt(2.0)              # pairwise 12 sd apart
    z = rng.integers(0, K, N)
    x = (centres[z] + rng.standard_normal((N, D))).astype(np.float32)
    loop = _mix().DiagLoop.from_centers(_cuda(x), _cuda(centres.astype(np.float32)), smooth=0.1)
    loop.run(5)
    assert torch.equal(loop.r.argmax(1).cpu(), torch.as_tensor(z))
    assert math.isfinite(loop.lower_bound())


def test_python_surface_and_refusals():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import gmm
    M, E = _mix(), V._lib.VmpError
    N, D, K = 300, 12, 3
    x, r0, prior = _data(N, D, K)
    truth = _case(N, D, K, 3)[3]
    xd, rd = _cuda(x), _cuda(r0)
    dp = M.default_diag_prior(xd, K)
    for u, v in zip(dp, prior):
        assert torch.equal(u.cpu(), torch.as_tensor(v))
    step, log_r, theta, aux = gmm.inference_diag(xd, K, 0, r_init=rd)
    for _ in range(3):
        r = step()
    loop = _loop(x, r0, prior)
    with pytest.raises(E, match='iteration'):
        loop.lower_bound()
    for _ in range(3):
        loop.step(want_logr=True)
    assert torch.equal(r, loop.r) and torch.equal(log_r(), loop.logr)
    for u, v in zip(theta() + aux(), loop.theta() + loop.aux()):
        assert torch.equal(u, v)
    _check('gmm.inference_diag N=%d D=%d K=%d' % (N, D, K), truth, dict(r=r, logr=log_r(), theta=theta()))
    lb = gmm.lower_bound_diag(xd, *theta())
    assert lb.shape == () and lb.dtype == torch.float64 and lb.is_cuda and lb.item() == loop.lower_bound()
    _check('gmm.lower_bound_diag', truth, dict(bound=lb.item()))
    # iterations per step, the default Dirichlet start, finalize and terms through their wrappers
    step3 = gmm.inference_diag(xd, K, 0, iterations=3, r_init=rd)[0]
    assert torch.equal(step3(), r)
    assert torch.isfinite(gmm.inference_diag(xd, K, 1)[0]()).all()
    post = M.diag_finalize(loop.stats, dp)
    assert M.diag_bound_terms(dp, [post[n] for n in ('alpha', 'beta', 'm', 'a', 'b')]).shape == (2 + K,)
    hist = loop.run_until_bound(1e-5, check_every=2, max_iterations=40)
    assert 2 <= len(hist) <= 20 and hist[-1][0] == loop.iterations
    for (_, u), (_, v) in zip(hist, hist[1:]):
        assert v >= u - 1e-6 * max(1.0, abs(u)), hist
    assert len(hist) == 20 or hist[-1][1] - hist[-2][1] < 1e-5 * max(1.0, abs(hist[-1][1]))
    for fn in (loop.score, loop.impute, loop.sample):
        with pytest.raises(E, match='not built'):
            fn(xd)
    # a NaN row for a component whose b is not positive
    th = [t.clone() for t in loop.theta()]
    th[4][1, 2] = 0.0
    pack = M.diag_pack(*th)
    assert torch.isnan(pack[1]).all() and torch.isfinite(pack[0]).all() and torch.isfinite(pack[2]).all()
    # the full-covariance loop still stops at 8 dimensions
    with pytest.raises(E, match='D=9'):
        M.VMPLoop(torch.zeros(16, 9, device='cuda'), torch.full((16, 2), 0.5, device='cuda'), V._lib.VMP_GMM)
