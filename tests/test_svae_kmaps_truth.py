"""tests/svae_kmaps_truth.py checked on the CPU: every family is well posed at every latent size, no bar is wide enough to hide a failure
(cap 1e-3), and each bar rejects each of the listed wrong kernels (MUTATIONS) by more than ten times - so the GPU half
(tests/test_svae_kmaps_gpu.py) can be judged before it runs.  The per-family figures are in profiles/NOTES_svae_kmaps.md."""
import functools

import numpy as np
import pytest
import torch

import svae_kmaps_truth as T

LS = list(range(1, 9))
KS = (3, 64)
# mutations that change nothing at a latent size: a 1 x 1 matrix is its own transpose, has no off-diagonal and no upper triangle
NOOPS = {(m, 1) for m in ('L_transposed', 'gP_lower_only', 'W_offdiag_zeroed', 'W_upper_nonzero', 'gW_symmetrised')}


def _lower_upstream(g):
    return g[0], np.tril(g[1]), g[2]


@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('name', T.FAMILIES)
def test_families_are_well_posed_and_no_bar_can_hide_a_failure(name, L):
    for K in KS:
        rng = T.case_rng(name, K, L)
        c = T.family(name, K, L, rng)
        g = T.upstream(K, L, rng)
        # every C_k SPD in the fp32 values: the fp64 Cholesky factorisation ends with all pivots > 0
        fac, info = torch.linalg.cholesky_ex(T.theta_C(c.theta))
        assert int(info.abs().max()) == 0 and float(torch.diagonal(fac, dim1=-2, dim2=-1).min()) > 0.0
        nu = torch.tensor(c.theta[4]) - (L + 2)
        assert float(nu.min()) > 0.0 and float(torch.tensor(c.theta[3]).min()) > 0.0 and float((torch.tensor(c.theta[0]) + 1).min()) > 0.0
        pairs = [T.phi_pair(c, g), T.theta_pair(c), T.smm_pair(c, _lower_upstream(g))]
        for t64, t32 in pairs:
            assert all(bool(torch.isfinite(v).all()) for v in t64.values()), (name, K, L)
            bars, _ = T.bars(t64, t32)
            assert max(bars.values()) <= T.BAR_CAP, (name, K, L, bars)
        x_s, r = T.cvi_inputs(K, L, rng)
        c64, c32 = T.cvi_pair(c, x_s, r)
        cb, _ = T.cvi_bars(c64, c32)
        assert all(bool(torch.isfinite(v).all()) for row in c64 for v in row)
        assert max(max(row) for row in cb) <= T.BAR_CAP, (name, K, L, cb)
        # the factor the truth states the bias on IS the Cholesky factor of the oracle's P (where P can be factorised to fp64 at all)
        Lk, P = pairs[0][0]['L_k'], pairs[0][0]['P']
        assert T.rel(Lk @ Lk.transpose(-1, -2), P) < 1e-12                                 # needs no factorisation: holds at small_diag too
        if name != 'small_diag':
            assert T.rel(torch.linalg.cholesky(P), Lk) < 1e-9
        assert float(torch.triu(pairs[1][0]['W'], 1).abs().max()) == 0.0 and float(torch.triu(pairs[2][0]['W'], 1).abs().max()) == 0.0
        WtW = pairs[1][0]['W'].transpose(-1, -2) @ pairs[1][0]['W']
        nuC = T.theta_C(c.theta) / nu.view(-1, 1, 1)                                       # E[Sigma] = C / nu
        assert T.rel(WtW @ nuC, torch.eye(L, dtype=torch.float64).expand(K, L, L)) < 1e-7


def test_families_have_the_hard_feature_they_name():
    K, L = 64, 6
    mk = lambda n: T.family(n, K, L, T.case_rng(n, K, L))
    i = np.arange(L)
    sp = np.log1p(np.exp(mk('small_diag').phi[1][:, i, i]))
    assert 9e-4 < sp.min() < 2e-3 and 3e-2 < sp.max() < 5e-2
    P = T.phi_truth(*mk('small_diag').phi)['P']
    assert float(torch.linalg.cond(P).max()) > 1e3
    ld = mk('large_diag').phi[1][:, i, i]
    assert ld.min() >= 20.0 and ld.max() <= 45.0 and np.all(np.log1p(np.exp(-ld)) < 2.1e-9)
    assert float(T.phi_truth(*mk('wide_pi').phi)['logpi'].min()) < -79.9
    a = mk('alpha_pole')
    for al in (a.theta[0], a.theta_t[0]):
        assert abs((al + 1).min() - 1e-3) < 1e-7 and abs((al + 1).max() - 1e6) < 1.0
    nu = mk('low_nu').theta[4] - (L + 2)
    assert 0.05 <= nu.min() and nu.max() < 1.0 + 1e-6
    cb = mk('cancelling_b')
    bb = np.einsum('ki,kj->kij', cb.theta[2], cb.theta[2]) / cb.theta[3][:, None, None]
    ratio = np.linalg.norm(bb, 2, axis=(1, 2)) / np.linalg.norm(T.theta_C(cb.theta).numpy(), 2, axis=(1, 2))
    assert 5e2 < ratio.min() and ratio.max() < 2e3
    dof = mk('dof_ends').theta_t[3]
    assert abs(dof.min() - 2.01) < 1e-6 and abs(dof.max() - 300.0) < 1e-3


@pytest.mark.parametrize('L', [1, 2, 3])
@pytest.mark.parametrize('name', T.FAMILIES)
def test_truth_gradients_are_the_probe_loss_gradients(name, L):
    """central differences (step 1e-6, fp64) of the probe loss sum(out * g_out) in every raw entry against the autograd gradients, K = 2, in
    every family, to 1e-6 of the largest gradient entry"""
    K = 2
    rng = T.case_rng(name, K, L)
    c = T.family(name, K, L, rng)
    g = T.upstream(K, L, rng)
    gs = _lower_upstream(g)

    def phi_loss(args):
        t = T.phi_truth(*args)
        return float((torch.tensor(args[0]) * torch.tensor(g[0])).sum() + (t['P'] * torch.tensor(g[1])).sum() + (t['bias'] * torch.tensor(g[2])).sum())

    def smm_loss(args):
        t = T.smm_theta_truth(c.theta_t[0], args[0], args[1], c.theta_t[3])
        return float((torch.tensor(args[0]) * torch.tensor(gs[0])).sum() + (t['W'] * torch.tensor(gs[1])).sum() + (t['kappa'] * torch.tensor(gs[2])).sum())
    tp = T.phi_truth(*c.phi, g=g)
    ts = T.smm_theta_truth(*c.theta_t, g=gs)
    for loss, args, grads in ((phi_loss, c.phi, [tp['g_mu'], tp['g_Lraw'], tp['g_piraw']]),
                              (smm_loss, c.theta_t[1:3], [ts['g_mu'], ts['g_Lraw']])):
        scale = max(1.0, max(float(gr.abs().max()) for gr in grads))
        for a, gr in zip(range(len(args)), grads):
            for idx in np.ndindex(args[a].shape):
                hi, lo = [x.copy() for x in args], [x.copy() for x in args]
                hi[a][idx] += 1e-6
                lo[a][idx] -= 1e-6
                fd = (loss(hi) - loss(lo)) / 2e-6
                assert abs(fd - float(gr[idx])) <= 1e-6 * scale, (a, idx, fd, float(gr[idx]))


def _moved(mut, real, bars):
    """the largest movement of any output in units of its bar; an output the mutation makes non-finite counts as moved without bound (the GPU
    test's `err <= bar` fails on a NaN)"""
    return max(float('inf') if not bool(torch.isfinite(mut[n]).all()) else T.rel(mut[n], real[n]) / bars[n] for n in bars)


def _reduce_case(K, L, nblk, rng):
    return (rng.standard_normal((nblk, K, T.partial_words(L))) * np.exp(rng.standard_normal((nblk, K, 1)))).astype(np.float32)


PHI_MUTS = ('L_transposed', 'softplus_grad_dropped', 'gP_lower_only', 'logpi_unnormalised')
THETA_MUTS = ('dirichlet_plus1_dropped', 'nu_off_by_one', 'W_offdiag_zeroed', 'W_upper_nonzero', 'kappa_logdiag_sign')
SMM_MUTS = ('dirichlet_plus1_dropped', 'W_offdiag_zeroed', 'W_upper_nonzero', 'kappa_logdiag_sign', 'smm_gkappa_term_dropped')
REDUCE_MUTS = ('reduce_row_left_out', 'gW_symmetrised')


@functools.lru_cache(maxsize=None)
def _case_truths(name, K, L):
    rng = T.case_rng(name, K, L)
    c = T.family(name, K, L, rng)
    g = T.upstream(K, L, rng)
    gs = _lower_upstream(g)
    phi, theta, smm = T.phi_pair(c, g), T.theta_pair(c), T.smm_pair(c, gs)
    return c, g, gs, (phi[0], T.bars(*phi)[0]), (theta[0], T.bars(*theta)[0]), (smm[0], T.bars(*smm)[0])


def mutation_margins(mut, name, K, L):
    """{truth it applies to: movement in bars} of one mutation on one case - the very case, truth and bars of the GPU test"""
    c, g, gs, phi, theta, smm = _case_truths(name, K, L)
    out = {}
    if mut in REDUCE_MUTS:
        rng = np.random.Generator(np.random.PCG64(31 * K + L))
        for nblk in (17, 65):
            p = _reduce_case(K, L, nblk, rng)
            want, sabs = T.reduce_truth(p, K, L, True)
            got, _ = T.reduce_truth(p, K, L, True, mut=mut)
            out['reduce%d' % nblk] = max(float(((got[n] - want[n]).abs() / T.reduce_bar(want[n], sabs[n], nblk).clamp_min(1e-300)).max()) for n in want)
    if mut in PHI_MUTS:
        out['phi'] = _moved(T.phi_truth(*c.phi, g=g, mut=mut), *phi)
    if mut in THETA_MUTS:
        out['theta'] = _moved(T.theta_truth(*c.theta, mut=mut), *theta)
    if mut in SMM_MUTS:
        out['smm'] = _moved(T.smm_theta_truth(*c.theta_t, g=gs, mut=mut), *smm)
    return out


# (mutation, family, truth) the bars cannot see at any L or K, and why.  Each is visible in another family at the same L and K (`generic` sees all).
BLIND = {
    ('L_transposed', 'init', 'phi'): 'init_recognition_params gives a diagonal L_k: L^T L = L L^T',
    ('W_offdiag_zeroed', 'init', 'theta'): 'C = c I at the init point: E[Sigma] and W are diagonal but for the rounding of b b^T / beta',
    ('W_upper_nonzero', 'init', 'theta'): 'as W_offdiag_zeroed: the copied off-diagonal is rounding noise',
    ('gP_lower_only', 'small_diag', 'phi'): 'g_Lraw is dominated by the bias terms in 1 / L_ii (1e3 and more) and the bar is relative to its largest '
                                            'entry; the (G + G^T) L term carries a factor L_ij of 1e-2 and less',
    ('softplus_grad_dropped', 'large_diag', 'phi'): "softplus'(x) = 1 to 2e-9 for x >= 20",
}


@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('name', T.FAMILIES)
@pytest.mark.parametrize('mut', T.MUTATIONS)
def test_the_bars_would_catch_a_wrong_kernel(mut, name, L):
    """Each listed error, applied to the truth of a case, moves at least one output by more than 10 x that output's bar - the bar the GPU test
    holds the kernel to on the same case - in every truth it applies to, in every family, at both K.  Where it is a no-op (NOOPS: L = 1) it moves
    nothing (less than a thousandth of a bar); where a family cannot see it (BLIND) it stays under the 10 bars, so the table cannot overstate."""
    for K in KS:
        margins = mutation_margins(mut, name, K, L)
        assert margins
        for which, m in margins.items():
            if (mut, L) in NOOPS:
                assert m < 1e-3, (mut, name, K, L, which, m)              # rounding of the rearranged products alone
            elif (mut, name, which) in BLIND:
                assert m <= 10.0, (mut, name, K, L, which, m)
            else:
                assert m > 10.0, (mut, name, K, L, which, m)


def test_the_oracle_derived_bars_reject_the_mutations_of_their_own_truth():
    """the bars that do NOT sit at their floor - cancelling_b theta/W and kappa, dof_ends smm/kappa, small_diag g_Lraw - against the mutations of
    their own truth (small_diag: all but the listed blind spot)"""
    for name, which, muts in (('cancelling_b', 'theta', THETA_MUTS), ('dof_ends', 'smm', SMM_MUTS), ('small_diag', 'phi', PHI_MUTS)):
        i = dict(phi=3, theta=4, smm=5)[which]
        all_bars = [_case_truths(name, K, L)[i][1] for K in KS for L in LS]
        assert any(b > 2 * T.floor_of(n) for bars in all_bars for n, b in bars.items()), name   # a bar of this family does come from the oracle
        for mut in muts:
            if (mut, name, which) in BLIND:
                continue
            for K in KS:
                for L in LS[1:]:
                    assert mutation_margins(mut, name, K, L)[which] > 10.0, (mut, name, K, L)


def test_reduce_truth_unpacks_the_documented_layout():
    """word w of component k holds 1000 k + w in one row: g_P carries the packed lower word in both triangles, g_W in the lower one only"""
    K, L, TRI = 3, 4, 10
    TH = L + TRI + 1
    p = np.zeros((2, K, 2 * TH), np.float32)
    p[0] = 1000.0 * np.arange(K)[:, None] + np.arange(2 * TH)[None, :]
    for theta_side in (False, True):
        got, sabs = T.reduce_truth(p, K, L, theta_side)
        assert set(got) == ({'g_hk', 'g_P', 'g_bias'} | ({'g_mk', 'g_W', 'g_kappa'} if theta_side else set()))
        for k in range(K):
            for i in range(L):
                assert got['g_hk'][k, i] == 1000 * k + i
                for j in range(i + 1):
                    w = 1000 * k + L + i * (i + 1) // 2 + j
                    assert got['g_P'][k, i, j] == w and got['g_P'][k, j, i] == w
                    if theta_side:
                        assert got['g_W'][k, i, j] == w + TH and (i == j or got['g_W'][k, j, i] == 0.0)
            assert got['g_bias'][k] == 1000 * k + L + TRI
            if theta_side:
                assert got['g_kappa'][k] == 1000 * k + 2 * TH - 1 and got['g_mk'][k, 1] == 1000 * k + TH + 1
        assert all(torch.equal(sabs[n], got[n].abs()) for n in got)
