"""Coverage of the diagonal-covariance mixture fit on the GPU (csrc/vmp_diagfit.hip, models/_diag.py) beyond tests/test_mix_diag_gpu.py,
against the fp64 truth of tests/mix_diag_truth.py:

  A  every instance: D = 1..64, each with one K <= 16 and one K > 16 (128 of 128 diag_pass_kernel<D, KTMAX>), at N = 600, where each
     wave has a first flush that overwrites, a last one that accumulates, and the last wave a 24-row tile
  B  block geometry: 20, 74, 512 (cap) and 256 (cap) blocks - several waves per reduce group, a wrapped block-partial loop, rows per
     wave rounded under a cap, runs of waves without rows.  Exact integer moments through r_in, an exact row count through the bound,
     and fp64 parity of one real pass with the truth walked in chunks
  C  tiny N: 1, 2, 63, 64
  D  xbar, S, pi and the per-component bound terms against a reference; an empty component on the device; responsibilities that
     underflow to exact zeros in the E-part
  E  the K-sized fp64 kernels (finalize, pack, bound terms) at counts up to 1e8, against mpmath at 50 digits

Tolerance (never a constant found on the kernel): bar = max(1e-5, 3 x the error of the same functions run in fp32 against fp64 from
the same inputs) - absolute for r, relative to max(1, |value|) for everything else.  The exact checks of B use == ; E states its own
bars.  Achieved errors and bars go to the parity log."""
import functools
import math

import numpy as np
import pytest
import torch

import mix_diag_truth as T
import parity_log
import test_mix_diag_gpu as G

pytestmark = pytest.mark.gpu

_mix, _cuda, _loop, _state, _check, _bits = G._mix, G._cuda, G._loop, G._state, G._check, G._bits


def _record(kind, e, bar, what, e32=None):
    parity_log.record(kind, e, bar, what if e32 is None else '%s (fp32 restatement: %.2e)' % (what, e32))
    print('%s: kernel %.3e%s  bar %.3e' % (what, e, '' if e32 is None else '  fp32 restatement %.3e' % e32, bar))
    return e <= bar


def _blocks(N, D, K):
    import vmp_for_svae_amd as V
    return T.workspace_blocks(V._lib.lib().vmp_mixture_diag_workspace_bytes(N, D, K), D, K)


# ---- A. every instance ----

K_SMALL = (1, 2, 3, 5, 7, 8, 15, 16)
K_LARGE = (17, 24, 31, 32, 33, 47, 48, 49, 63, 64)
N_A = 600


def _ks(D):
    return K_SMALL[(D - 1) % len(K_SMALL)], K_LARGE[(D - 1) % len(K_LARGE)]


def test_the_sweep_covers_both_k_sets():
    pairs = [_ks(D) for D in range(1, 65)]
    assert {p[0] for p in pairs} == set(K_SMALL) and {p[1] for p in pairs} == set(K_LARGE)
    assert max(K_SMALL) <= 16 < min(K_LARGE) and {(k + 15) // 16 for k in K_LARGE} == {2, 3, 4}
    g = T.geometry(N_A, 64, 64)
    assert (g['blocks'], g['rpw'], g['empty']) == (1, 192, 0) and N_A - 3 * 192 == 24


@pytest.mark.parametrize('D', range(1, 65))
def test_every_d_instance_in_both_k_forms(D):
    for K in _ks(D):
        x, r0, prior, truth = G._case(N_A, D, K, 1)
        assert _blocks(N_A, D, K) == 1
        loop = _loop(x, r0, prior)
        r = loop.step(want_logr=True)
        assert r.shape == (N_A, K) and (r.double().sum(1) - 1).abs().max().item() < 1e-6
        _check('every instance N=%d D=%d K=%d' % (N_A, D, K), truth, _state(loop))


# ---- B. block geometry ----

GEOMETRY = [(40003, 3, 2), (150001, 2, 17), (1100003, 1, 2), (600001, 16, 64)]


def _assert_geometry(N, D, K):
    g = T.geometry(N, D, K)
    assert _blocks(N, D, K) == g['blocks']
    want = {40003: dict(cap=512, blocks=20, waves=80, rpw=512), 150001: dict(cap=512, blocks=74),
            1100003: dict(cap=512, blocks=512, waves=2048, rpw=576, empty=138),
            600001: dict(cap=256, blocks=256, waves=1024, rpw=640, empty=86)}.get(N, {})
    for name, v in want.items():
        assert g[name] == v, (name, g)
    return g


@pytest.mark.parametrize('N,D,K', GEOMETRY + [(600, 64, 64)])
def test_integer_moments_through_r_in_are_exact(N, D, K):
    """x in {0, 1, 2, 3}, r one-hot: every fp32 operation of the kernel is exact (mix_diag_truth.int_model), so stats are the
    integers - a dropped or doubled row, wave or block cannot hide in a tolerance"""
    _assert_geometry(N, D, K)
    xi, z = T.int_case(N, D, K)
    want = T.int_stats(xi, z, K)
    pack = torch.zeros(K, 2 * D + 1, device='cuda')
    got = _mix().mixture_diag_pass(_cuda(xi.astype(np.float32)), pack, r_in=_cuda(T.one_hot(z, K)), want_r=False)[2].cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    wrong = np.argwhere(got != want.astype(np.float64))
    parity_log.record('abs', np.abs(got - want).max(), 0.0, 'exact r_in stats N=%d D=%d K=%d' % (N, D, K))
    assert len(wrong) == 0, (len(wrong), wrong[:8], got[tuple(wrong[0])], want[tuple(wrong[0])])


@pytest.mark.parametrize('N,D,K', GEOMETRY[:3])
def test_row_count_through_the_bound_is_exact(N, D, K):
    """K = 1, m = 0, lbar = 0, c = 1: every row's log-sum-exp is exactly 1 and its r exactly 1"""
    g = _assert_geometry(N, D, K)
    assert _blocks(N, D, 1) == g['blocks']                                   # K = 1 keeps the block count of the shape
    xi, _ = T.int_case(N, D, 1)
    pack = torch.zeros(1, 2 * D + 1, device='cuda')
    pack[0, 2 * D] = 1.0
    r, logr, stats, bound = _mix().mixture_diag_pass(_cuda(xi.astype(np.float32)), pack, want_logr=True, want_bound=True)
    rows = bound.item() + 0.5 * N * D * math.log(2.0 * math.pi)
    parity_log.record('abs', abs(rows - N), 1e-6, 'row count through the bound N=%d D=%d' % (N, D))
    assert abs(rows - N) <= 1e-6, (rows, N)
    assert r.shape == (N, 1) and (r == 1).all() and (logr == 0).all()
    assert stats[0, 0].item() == N
    want = T.int_stats(xi, np.zeros(N, np.int64), 1)
    assert np.array_equal(stats.cpu().numpy(), want.astype(np.float64))


@functools.lru_cache(maxsize=None)
def _pass_case(N, D, K):
    """x, and theta = the truth's fp64 M-step of a Dirichlet r0 on the first 4096 rows, rounded to fp32"""
    x, r0 = T.make_data(N, D, K, 100 * D + 7 * K + N % 11, r_rows=4096)
    prior = T.default_prior(x, K)
    theta = T.m_step(*T.moments(x[:4096], r0, torch.float64), prior, torch.float64)
    return x, [t.float() for t in theta]


@pytest.mark.parametrize('N,D,K', GEOMETRY)
def test_one_pass_at_block_geometry_against_fp64(N, D, K):
    _assert_geometry(N, D, K)
    M = _mix()
    x, theta = _pass_case(N, D, K)
    xd = _cuda(x)
    pack = M.diag_pack(*[t.cuda() for t in theta])
    r, logr, stats, bound = M.mixture_diag_pass(xd, pack, want_logr=True, want_bound=True)
    fast = M.mixture_diag_pass(xd, pack, want_r=False, want_bound=True)
    assert fast[0] is None and fast[1] is None
    assert torch.equal(_bits(fast[2]), _bits(stats)) and torch.equal(_bits(fast[3]), _bits(bound))
    assert (r.double().sum(1) - 1).abs().max().item() < 1e-6
    truth = T.pass_truth(x, theta, got_r=r.cpu(), got_logr=logr.cpu())
    what = 'one pass N=%d D=%d K=%d ' % (N, D, K)
    errs = dict(r=truth['err_r'], logr=truth['err_logr'], stats=T.rel_err(stats, truth['stats']),
                data=T.rel_err(bound.item(), truth['data']))
    ok = [_record('abs' if n == 'r' else 'rel', e, truth['bar_' + n], what + n, truth['e_' + n]) for n, e in errs.items()]
    assert all(ok), (what, errs, {n: truth['bar_' + n] for n in errs})


# ---- C. tiny N ----

TINY = [(1, 64, 64), (1, 1, 1), (2, 9, 17), (63, 17, 3), (64, 33, 33)]


@pytest.mark.parametrize('N,D,K', TINY)
def test_tiny_n(N, D, K):
    G._one_and_three(N, D, K)
    if N == 1:                                                                # S = 0: the first moments are Nk x_0
        x, r0, prior, truth = G._case(N, D, K, 1)
        assert (truth['S'] == 0).all()
        loop = _loop(x, r0, prior)
        loop.step()
        stats = loop.stats.cpu()
        want = stats[:, :1] * torch.as_tensor(x).double()[0][None, :]
        e = T.rel_err(stats[:, 1:1 + D], want)
        assert _record('rel', e, truth['bar_stats'], 'N=1 D=%d K=%d sx against Nk x_0' % (D, K), truth['e_stats'])


# ---- D. the outputs without a reference, the empty component, exact zeros ----

AUX = [(257, 17, 3, 0.0), (1031, 33, 33, 0.0), (1031, 33, 33, 1000.0)]


@pytest.mark.parametrize('N,D,K,offset', AUX)
def test_aux_and_bound_terms_against_fp64(N, D, K, offset):
    x, r0, prior = G._data(N, D, K, offset)
    what = 'N=%d D=%d K=%d%s' % (N, D, K, ' offset %g' % offset if offset else '')
    loop = _loop(x, r0, prior)
    for iterations in (1, 3):
        loop.run(iterations - loop.iterations)
        truth = G._case(N, D, K, iterations, offset)[3]
        xbar, S, pi = loop.aux()
        got = dict(xbar=xbar, S=S, pi=pi)
        if iterations == 3:
            out = _mix().diag_bound_terms(loop.prior, loop.theta())
            assert out.shape == (2 + K,) and out.dtype == torch.float64
            got.update(kl_pi=out[0].item(), kl_sum=out[1].item(), kl_k=out[2:])
        _check('%d iteration(s) %s' % (iterations, what), truth, got)


def test_an_empty_component_keeps_its_prior_on_the_device():
    N, D, K = 300, 12, 4
    x, r0, prior = G._data(N, D, K)
    r0 = r0.copy()
    r0[:, 2] = 0.0
    r0 /= r0.sum(1, keepdims=True)
    loop = _loop(x, r0, prior)
    loop.step(want_logr=True)
    assert loop.stats[2, 0].item() == 0.0
    for t, p in zip(loop.theta(), prior):
        assert torch.isfinite(t).all()
        assert torch.equal(t[2].cpu(), torch.as_tensor(p)[2])
    xbar, S, pi = loop.aux()
    assert (xbar[2] == 0).all() and (S[2] == 0).all()
    assert all(torch.isfinite(t).all() for t in (xbar, S, pi, loop.r, loop.logr, loop.stats))
    for iterations in (1, 3):
        loop.run(iterations - loop.iterations)
        truth = T.bars(x, r0, prior, iterations)
        st = _state(loop)
        st.update(zip(('xbar', 'S', 'pi'), loop.aux()))
        assert math.isfinite(st['bound'])
        _check('empty component, %d iteration(s)' % iterations, truth, st)


def _planted_loop():
    """4 clusters 40 sd apart, started from the nearest centre, two iterations: (loop, labels, truth with bars)"""
    N, D, K = 600, 24, 4
    x, centres, z = T.planted_clusters(N, D, K, 40.0, 11)
    loop = _mix().DiagLoop.from_centers(_cuda(x), _cuda(centres.astype(np.float32)))
    prior = T.default_prior(x, K)
    for u, v in zip(loop.prior, prior):
        assert torch.equal(u.cpu(), torch.as_tensor(v))
    loop.step(want_logr=True)
    loop.step(want_logr=True)
    return loop, z, T.bars(x, T.one_hot(z, K), prior, 2)


def test_responsibilities_that_underflow_to_exact_zeros():
    """exp(log rho - max) is exactly 0 in fp32 for the three wrong components of every row: r is one-hot, log r stays finite"""
    loop, z, truth = _planted_loop()
    r, logr = loop.r, loop.logr
    assert (r.max(1).values == 1).all() and (r.sum(1) == 1).all() and ((r == 0).sum(1) == loop.K - 1).all()
    assert torch.equal(r.argmax(1).cpu(), torch.as_tensor(z))
    assert torch.isfinite(logr).all() and logr.min().item() < -200
    st = _state(loop)
    assert torch.isfinite(st['stats']).all() and math.isfinite(st['bound'])
    _check('exact zeros N=600 D=24 K=4', truth, dict(r=st['r'], logr=st['logr'], bound=st['bound']))


@pytest.mark.xfail(strict=True, reason='the one-pivot shift (profiles/NOTES_mix_diagfit.md, Accuracy): sx of a component centred at 0 in a '
                                       'column where the pivot sits at 8.0 is recovered from a shifted fp32 sum of -1122; '
                                       'stats 3.9e-5 against a bar of 1e-5 (fp32 restatement 2.3e-6)')
def test_moments_of_one_hot_responsibilities_far_from_the_pivot():
    """The raw moments of the same state.  MI355X: stats 3.919e-05, fp32 restatement 2.251e-06, bar 1.000e-05.  The worst word is
    sx[1, 3] = 0.886: component 1 is centred at 0 in column 3, the pivot (the mean of 64 rows of all four clusters) is 7.96 there, so
    sx = s1 + Nk pivot with s1 = -1122 summed in fp32.  A numpy fp32 model of the kernel's sums gives the same 3.919e-05; the
    restatement centres every component on its own mean and loses nothing.  The bar stays as the rule gives it."""
    loop, z, truth = _planted_loop()
    _check('exact zeros N=600 D=24 K=4', truth, dict(stats=loop.stats))


# ---- E. the K-sized kernels at large counts ----

COUNTS = (0.0, 1e-3, 1.0, 1e3, 1e6, 1e8)
FP32_BAR = 2.0 ** -23          # the kernels work in fp64 and round once (2^-24); as much again for the fp64 work inside
FP32_TINY = 2.0 ** -126


def _synthetic(D, K):
    rng = np.random.Generator(np.random.PCG64(1000 * D + K))
    Nk = np.array([COUNTS[(5 + 7 * k) % len(COUNTS)] for k in range(K)])               # K = 3: 1e8, 0, 1e-3
    xbar = rng.choice([-3.0, 3.0], (K, D)) + 0.25 * rng.standard_normal((K, D))
    S = rng.uniform(0.25, 2.25, (K, D))
    stats = np.concatenate([Nk[:, None], Nk[:, None] * xbar, Nk[:, None] * (S + xbar * xbar)], 1)
    m0 = np.tile((0.5 * rng.standard_normal(D)).astype(np.float32)[None, :], (K, 1))
    prior = (np.full(K, 0.05 / K, np.float32), np.full(K, 0.5, np.float32), m0, np.ones(K, np.float32), np.ones((K, D), np.float32))
    return stats, prior


@pytest.mark.parametrize('D,K', [(64, 64), (5, 3)])
def test_k_sized_kernels_at_large_counts_against_mpmath(D, K):
    M = _mix()
    stats, prior = _synthetic(D, K)
    assert set(stats[:, 0]) == (set(COUNTS) if K >= len(COUNTS) else {1e8, 0.0, 1e-3})
    what = 'large counts D=%d K=%d ' % (D, K)
    dprior = [_cuda(p) for p in prior]
    post = M.diag_finalize(_cuda(stats), dprior)
    theta = [post[n] for n in T.NAMES]
    pack = M.diag_pack(*theta)
    terms = M.diag_bound_terms(dprior, theta)
    assert all(torch.isfinite(t).all() for t in list(post.values()) + [pack, terms])
    bad = []
    ref = T.mp_finalize(stats, prior)
    for name in T.NAMES + ('xbar', 'S', 'pi'):
        e = T.mp_err(post[name], ref[name], FP32_TINY)
        if not _record('rel', e, FP32_BAR, what + name):
            bad.append((name, e, FP32_BAR))
    host = [t.cpu().numpy() for t in theta]                                   # the device's own fp32 posterior: the kernels' input
    e = T.mp_err(pack, T.mp_pack(host), FP32_TINY)
    if not _record('rel', e, FP32_BAR, what + 'pack'):
        bad.append(('pack', e, FP32_BAR))
    mp_pi, mp_ng = T.mp_terms(host, prior)
    kl_pi, kl_ng = T.kl_terms(host, prior)
    for name, got, t64, want in (('kl_pi', terms[:1], [kl_pi], [mp_pi]), ('kl_k', terms[2:], kl_ng.sum(1), mp_ng.sum(1)),
                                 ('kl_sum', terms[1:2], [kl_ng.sum().item()], [mp_ng.sum()])):
        e64 = T.mp_err(t64, want, 1.0)
        bar = max(1e-12, 3 * e64)
        e = T.mp_err(got, want, 1.0)
        parity_log.record('rel', e, bar, '%s%s (fp64 torch: %.2e)' % (what, name, e64))
        print('%s%s: kernel %.3e  fp64 torch %.3e  bar %.3e' % (what, name, e, e64, bar))
        if not e <= bar:
            bad.append((name, e, bar, e64))
    assert not bad, (what, bad)
