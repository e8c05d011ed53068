"""The K-sized parameter maps of the SVAE step (csrc/vmp_prep_parts.h, vmp_prep.hip, vmp_step_parts.h) in every launch that has a short argument
list, against the fp64 truth of tests/svae_kmaps_truth.py: every latent size L = 1..8, K from 1 to a full wave, the hard parameter families, the
`WS = true` bodies inside the encoder's forward launch (the only route to the Student-t packing) and the nblk edges of the 16-group, 4-chain
reductions.  Every bar is max(floor, 3 x the fp32 oracle's own loss on the case) - tests/test_svae_kmaps_truth.py shows on the CPU that no such
bar exceeds 1e-3 and that each rejects the listed wrong kernels by more than ten times; the reductions have a derived per-element bar.  Outputs
are pre-filled with NaN: an element no lane writes fails its comparison.  Measured errors: profiles/NOTES_svae_kmaps.md."""
import functools

import numpy as np
import pytest
import torch

import parity_log
import svae_kmaps_truth as T

pytestmark = pytest.mark.gpu

LS = list(range(1, 9))
# every L with a full wave of components (K = 64) and with K < L^2 (lanes beyond K take part in the matrix work); every K of {1, 3, 16, 33, 64}
PAIRS = [(64, L) for L in LS] + [(3, 1), (1, 2), (16, 2), (3, 3), (33, 3), (1, 4), (16, 4), (16, 5), (3, 6), (33, 6), (1, 7), (16, 7), (3, 8), (33, 8)]
ALL_FAMILY_PAIRS = [(16, 8), (33, 7), (3, 5), (64, 1)]
CASES = list(dict.fromkeys([(K, L, f) for K, L in PAIRS for f in ('generic', 'small_diag')] + [(K, L, f) for K, L in ALL_FAMILY_PAIRS for f in T.FAMILIES]))
RED_PAIRS = [(64, 1), (3, 2), (33, 3), (16, 4), (3, 5), (33, 6), (33, 7), (16, 8)]
NBLKS = [1, 15, 16, 17, 63, 64, 65, 300]
CVI_CASES = list(dict.fromkeys([(K, L, 'generic') for K, L in RED_PAIRS] + [(K, L, f) for K, L in ALL_FAMILY_PAIRS for f in T.FAMILIES]))
ids3 = lambda c: '%d-%d-%s' % c if isinstance(c, tuple) else str(c)
NAN = float('nan')


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda').contiguous()


def poisoned(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def hold(what, got, want, bar):
    """the measured error, relative to the largest entry of the truth, logged and held to the bar (a NaN - an unwritten element - fails)"""
    err = parity_log.record('rel', T.rel(got, want), tol=bar, what=what)
    assert err <= bar, (what, err, bar)


@functools.lru_cache(maxsize=None)
def truth(K, L, fam):
    """computed once per case and shared by the tests below; never written to"""
    rng = T.case_rng(fam, K, L)
    c = T.family(fam, K, L, rng)
    g = T.upstream(K, L, rng)
    phi, theta, smm = T.phi_pair(c, g), T.theta_pair(c), T.smm_pair(c)
    return dict(case=c, g=g, phi=phi[0], theta=theta[0], smm=smm[0], phi_bars=T.bars(*phi)[0], theta_bars=T.bars(*theta)[0], smm_bars=T.bars(*smm)[0])


def _lib():
    import vmp_for_svae_amd as V
    return V._lib, V._lib.lib()


def _logpi_holds(pi_raw, got):
    """log softmax(pi_raw) to 1e-14 absolute; the truth in extended precision (at log pi = -80 an fp64 truth is itself off by 7e-15)"""
    x = np.asarray(pi_raw, np.longdouble)
    want = x - x.max() - np.log(np.exp(x - x.max()).sum())
    err = float(np.abs(got.cpu().numpy().astype(np.longdouble) - want).max())
    parity_log.record('abs', err, tol=1e-14, what='logpi')
    assert err <= 1e-14, err


def _hold_phi_fwd(launch, t, Lk, P, bias):
    for n, a in (('L_k', Lk), ('P', P), ('bias', bias)):
        hold('%s:%s' % (launch, n), a, t['phi'][n], t['phi_bars'][n])


def _hold_theta(launch, t, m, W, kappa, which='theta'):
    for n, a in (('m', m), ('W', W), ('kappa', kappa)):
        if a is None:
            continue
        hold('%s:%s' % (launch, n), a, t[which][n], t[which + '_bars'][n])
        if n == 'W':
            assert torch.count_nonzero(torch.triu(a, 1)) == 0, launch               # packed lower factor: exact zeros above the diagonal


@pytest.mark.parametrize('case', CASES, ids=ids3)
def test_phi_prep_forward_and_backward(case):
    """vmp_svae_phi_prep_fwd (L_k, P, bias) and vmp_svae_phi_prep_bwd against the truth; the upper triangle of g_Lraw exactly 0"""
    K, L, fam = case
    t = truth(*case)
    Lb, lib = _lib()
    mu, Lraw, pi = [dev(a) for a in t['case'].phi]
    Lk, P, bias = poisoned(K, L, L), poisoned(K, L, L), poisoned(K)
    Lb.check(lib.vmp_svae_phi_prep_fwd(Lb.ptr(mu), Lb.ptr(Lraw), Lb.ptr(pi), K, L, Lb.ptr(Lk), Lb.ptr(P), Lb.ptr(bias), Lb.stream()), 'phi_prep_fwd')
    _hold_phi_fwd('phi_prep_fwd', t, Lk, P, bias)
    g = [dev(a) for a in t['g']]
    o = [poisoned(K, L), poisoned(K, L, L), poisoned(K)]
    Lb.check(lib.vmp_svae_phi_prep_bwd(Lb.ptr(mu), Lb.ptr(Lraw), Lb.ptr(pi), *[Lb.ptr(a) for a in g], K, L, *[Lb.ptr(a) for a in o], Lb.stream()),
             'phi_prep_bwd')
    for n, a in zip(('g_mu', 'g_Lraw', 'g_piraw'), o):
        hold('phi_prep_bwd:%s' % n, a, t['phi'][n], t['phi_bars'][n])
    assert torch.count_nonzero(torch.triu(o[1], 1)) == 0


@pytest.mark.parametrize('case', CASES, ids=ids3)
def test_theta_pack_and_the_two_maps_in_one_launch(case):
    """vmp_svae_theta_pack and vmp_svae_prep_fwd2 (both maps + log softmax(pi) in fp64) against the truth"""
    K, L, fam = case
    t = truth(*case)
    Lb, lib = _lib()
    th = [dev(a) for a in t['case'].theta]
    m, W, kap = poisoned(K, L), poisoned(K, L, L), poisoned(K)
    Lb.check(lib.vmp_svae_theta_pack(*[Lb.ptr(a) for a in th], K, L, Lb.ptr(m), Lb.ptr(W), Lb.ptr(kap), Lb.stream()), 'theta_pack')
    _hold_theta('theta_pack', t, m, W, kap)
    mu, Lraw, pi = [dev(a) for a in t['case'].phi]
    Lk, P, bias = poisoned(K, L, L), poisoned(K, L, L), poisoned(K)
    m, W, kap, logpi = poisoned(K, L), poisoned(K, L, L), poisoned(K), poisoned(K, dtype=torch.float64)
    Lb.check(lib.vmp_svae_prep_fwd2(Lb.ptr(mu), Lb.ptr(Lraw), Lb.ptr(pi), *[Lb.ptr(a) for a in th], K, L, Lb.ptr(Lk), Lb.ptr(P), Lb.ptr(bias), Lb.ptr(m),
                                    Lb.ptr(W), Lb.ptr(kap), Lb.ptr(logpi), Lb.stream()), 'prep_fwd2')
    _hold_phi_fwd('prep_fwd2', t, Lk, P, bias)
    _hold_theta('prep_fwd2', t, m, W, kap)
    _logpi_holds(t['case'].phi[2], logpi)


@pytest.mark.parametrize('case', CASES, ids=ids3)
def test_the_maps_inside_the_encoder_forward_launch(case):
    """vmp_mlp_gauss_head_fwd_prep and _prep_smm (the `WS = true` bodies in wave 0 of the encoder launch's extra blocks; R = 5, U = 16, no scalar
    table): both maps against the truth - for the Student-t packing its first, and the only stand-alone route; encoder outputs bit-equal to
    vmp_mlp_gauss_head_fwd."""
    K, L, fam = case
    t = truth(*case)
    Lb, lib = _lib()
    R, Dy, U = 5, 3, 16
    gen = torch.Generator(device='cuda').manual_seed(K * 10 + L)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32, device='cuda')
    enc = [rn(Dy, U) * 0.3, rn(U) * 0.1, rn(U, U) * 0.2, rn(U) * 0.1, rn(U, 2 * L) * 0.2, rn(2 * L) * 0.1, rn(Dy, L) * 0.3, rn(L) * 0.1, rn(L) * 0.1]
    yy = rn(R, Dy)
    e1, e2 = poisoned(R, L), poisoned(R, L)
    Lb.check(lib.vmp_mlp_gauss_head_fwd(Lb.ptr(yy), *[Lb.ptr(a) for a in enc], R, Dy, L, U, -0.5, Lb.ptr(e1), Lb.ptr(e2), Lb.stream()), 'enc')
    mu, Lraw, pi = [dev(a) for a in t['case'].phi]
    th = [dev(a) for a in t['case'].theta]
    o1, o2 = poisoned(R, L), poisoned(R, L)
    Lk, P, bias = poisoned(K, L, L), poisoned(K, L, L), poisoned(K)
    m, W, kap, logpi = poisoned(K, L), poisoned(K, L, L), poisoned(K), poisoned(K, dtype=torch.float64)
    Lb.check(lib.vmp_mlp_gauss_head_fwd_prep(Lb.ptr(yy), *[Lb.ptr(a) for a in enc], R, Dy, L, U, -0.5, Lb.ptr(o1), Lb.ptr(o2), Lb.ptr(mu), Lb.ptr(Lraw),
                                             Lb.ptr(pi), *[Lb.ptr(a) for a in th], K, Lb.ptr(Lk), Lb.ptr(P), Lb.ptr(bias), Lb.ptr(m), Lb.ptr(W), Lb.ptr(kap),
                                             Lb.ptr(logpi), None, 0, None, None, Lb.stream()), 'fwd_prep')
    assert torch.equal(o1, e1) and torch.equal(o2, e2)
    _hold_phi_fwd('fwd_prep', t, Lk, P, bias)
    _hold_theta('fwd_prep', t, m, W, kap)
    _logpi_holds(t['case'].phi[2], logpi)
    al, _, tLraw, dof = [dev(a) for a in t['case'].theta_t]
    o1, o2 = poisoned(R, L), poisoned(R, L)
    Lk, P, bias = poisoned(K, L, L), poisoned(K, L, L), poisoned(K)
    W, kap, logpi = poisoned(K, L, L), poisoned(K), poisoned(K, dtype=torch.float64)
    Lb.check(lib.vmp_mlp_gauss_head_fwd_prep_smm(Lb.ptr(yy), *[Lb.ptr(a) for a in enc], R, Dy, L, U, -0.5, Lb.ptr(o1), Lb.ptr(o2), Lb.ptr(mu), Lb.ptr(Lraw),
                                                 Lb.ptr(pi), Lb.ptr(al), Lb.ptr(tLraw), Lb.ptr(dof), K, Lb.ptr(Lk), Lb.ptr(P), Lb.ptr(bias), Lb.ptr(W),
                                                 Lb.ptr(kap), Lb.ptr(logpi), None, 0, None, None, Lb.stream()), 'fwd_prep_smm')
    assert torch.equal(o1, e1) and torch.equal(o2, e2)
    _hold_phi_fwd('fwd_prep_smm', t, Lk, P, bias)
    _hold_theta('fwd_prep_smm', t, None, W, kap, which='smm')
    _logpi_holds(t['case'].phi[2], logpi)


def _hold_reduce(what, got, want, sabs, nblk):
    """per element |got - want| <= 2^-23 |want| + nblk 2^-52 sum |p| (svae_kmaps_truth.reduce_bar); the logged figure is the largest error / bar"""
    for n in want:
        g = got[n].double().cpu()
        assert bool(torch.isfinite(g).all()), (what, n)
        ratio = float(((g - want[n]).abs() / T.reduce_bar(want[n], sabs[n], nblk).clamp_min(1e-300)).max()) if float(sabs[n].max()) > 0 else 0.0
        assert bool(((g - want[n]).abs() <= T.reduce_bar(want[n], sabs[n], nblk)).all()), (what, n, ratio)
        parity_log.record('err/bar', ratio, tol=1.0, what='%s:%s' % (what, n))


@pytest.mark.parametrize('nblk', NBLKS)
@pytest.mark.parametrize('K,L', RED_PAIRS)
def test_reductions_of_the_partial_rows(K, L, nblk):
    """vmp_svae_bwd_reduce without and with the theta half (g_mk, g_W lower, g_kappa) against the fp64 column sums, at the edges of the 16-group,
    4-chain loop; vmp_svae_bwd_reduce_prep against those sums followed by the truth's recognition backward (generic and small_diag phi)."""
    Lb, lib = _lib()
    rng = np.random.Generator(np.random.PCG64(1000 * nblk + 10 * K + L))
    p = (rng.standard_normal((nblk, K, T.partial_words(L))) * np.exp(rng.standard_normal((nblk, K, 1)))).astype(np.float32)
    pd = dev(p)
    for theta_side in (False, True):
        want, sabs = T.reduce_truth(p, K, L, theta_side)
        o = dict(g_hk=poisoned(K, L), g_P=poisoned(K, L, L), g_bias=poisoned(K))
        if theta_side:
            o.update(g_mk=poisoned(K, L), g_W=poisoned(K, L, L), g_kappa=poisoned(K))
        ptr = lambda n: Lb.ptr(o.get(n))
        Lb.check(lib.vmp_svae_bwd_reduce(Lb.ptr(pd), nblk, K, L, ptr('g_hk'), ptr('g_P'), ptr('g_bias'), ptr('g_mk'), ptr('g_W'), ptr('g_kappa'),
                                         Lb.stream()), 'bwd_reduce')
        _hold_reduce('bwd_reduce%s' % ('+theta' if theta_side else ''), o, want, sabs, nblk)
        assert torch.equal(o['g_P'], o['g_P'].transpose(1, 2))
        if theta_side:
            assert torch.count_nonzero(torch.triu(o['g_W'], 1)) == 0
    want, _ = T.reduce_truth(p, K, L, False)
    g = (want['g_hk'].numpy(), want['g_P'].numpy(), want['g_bias'].numpy())
    for fam in ('generic', 'small_diag'):
        c = T.family(fam, K, L, T.case_rng(fam, K, L))
        t64 = T.phi_truth(*c.phi, g=g)
        t32 = T.phi_truth(*c.phi, g=[a.astype(np.float32) for a in g], dtype=T.F32)
        names = ('g_mu', 'g_Lraw', 'g_piraw')
        bars, _ = T.bars(t64, t32, names)
        mu, Lraw, pi = [dev(a) for a in c.phi]
        logpi = dev(t64['logpi'].numpy(), torch.float64)
        o = [poisoned(K, L), poisoned(K, L, L), poisoned(K)]
        Lb.check(lib.vmp_svae_bwd_reduce_prep(Lb.ptr(pd), nblk, Lb.ptr(mu), Lb.ptr(Lraw), Lb.ptr(pi), Lb.ptr(logpi), K, L, *[Lb.ptr(a) for a in o],
                                              Lb.stream()), 'bwd_reduce_prep')
        for n, a in zip(names, o):
            hold('bwd_reduce_prep:%s' % n, a, t64[n], bars[n])
        assert torch.count_nonzero(torch.triu(o[1], 1)) == 0


@pytest.mark.parametrize('case', CVI_CASES, ids=ids3)
def test_cvi_update_and_stats_cvi(case):
    """vmp_svae_cvi_update (on vmp_mix_stats' moments) and vmp_svae_stats_cvi: theta*, theta against svae_ref.m_step + update_gmm_params in
    fp64, theta updated in place with its version counter bumped; step size by value and through the device word"""
    from vmp_for_svae_amd.models import _mix, _svae_ops
    K, L, fam = case
    c = T.family(fam, K, L, T.case_rng(fam, K, L))
    x_s, r = T.cvi_inputs(K, L, np.random.Generator(np.random.PCG64(K * 100 + L)))
    c64, c32 = T.cvi_pair(c, x_s, r)
    (bar_star, bar_theta), _ = T.cvi_bars(c64, c32)
    prior = [dev(a.numpy()) for a in T.E.oracle_prior(K, L)]
    xd, rd = dev(x_s), dev(r)
    for rho_dev in (None, torch.full((), T.CVI_RHO, device='cuda')):
        rho = T.CVI_RHO if rho_dev is None else 0.0
        for launch in ('cvi_update', 'stats_cvi'):
            th = [dev(a) for a in c.theta]
            vers = [a._version for a in th]
            if launch == 'cvi_update':
                star = _svae_ops.cvi_update(prior, th, _mix.raw_stats(xd, rd), rho, rho_dev=rho_dev)
            else:
                _, star = _svae_ops.stats_cvi(xd, rd, prior, th, rho, rho_dev=rho_dev)
            for i, n in enumerate(('alpha', 'A', 'b', 'beta', 'v_hat')):
                hold('%s:theta_star/%s' % (launch, n), star[i], c64[0][i], bar_star[i])
                hold('%s:theta/%s' % (launch, n), th[i], c64[1][i], bar_theta[i])
            assert all(a._version > v0 for a, v0 in zip(th, vers))
