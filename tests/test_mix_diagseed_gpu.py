"""The seeded start of the diagonal mixture on wide rows (csrc/vmp_diagseed.hip; include/vmp_hip.h "Diagonal-covariance mixture:
seeded start on wide rows") against the fp64 truth of tests/mix_seed_truth.py on the fixtures of tests/mix_diagseed_truth.py: the
chosen rows and the centres bit for bit, the final weights within the bar of the fp32 restatement, the assignment on every row the
truth can decide, the rows of the D <= 8 kernels, alignment, determinism, and fits started from the seed."""
import functools

import numpy as np
import pytest
import torch

import mix_diag_truth as DT
import mix_diagseed_truth as S
import mix_seed_truth as T

pytestmark = pytest.mark.gpu

CASES = S.SWEEP + [S.CAPPED]


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _dev(a, off=0):
    """the array on the GPU; off > 0: a view that starts `off` elements into its buffer (breaks 16-byte alignment)"""
    t = torch.as_tensor(np.ascontiguousarray(a))
    if not off:
        return t.cuda()
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device='cuda')
    view = buf[off:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _truth(N, D, K):
    t = S.truth(N, D, K)
    t['e32'] = T.restatement_error(t['x'], None, None, K, S.DRAW_SEED, t['c'])
    return t


def _check_centers(N, D, K, off):
    t = _truth(N, D, K)
    c = t['c']
    assert c['margin'].min() >= S.MARGIN, ('fixture', c['margin'].min())                 # a condition on the fixture, every round
    cen, idx, w = _mix().diag_seed_centers(_dev(t['x'], off), K, S.DRAW_SEED, want_index=True, want_mind2=True)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), c['index'])
    assert np.array_equal(cen.cpu().numpy().view(np.uint32), c['centers'].view(np.uint32))   # the bits of x at those rows
    err = float(np.max(np.abs(w.cpu().numpy().astype(np.float64) - c['w']) / np.maximum(1.0, np.abs(c['w']))))
    bar = max(1e-5, 3 * t['e32'])
    print('N=%d D=%d K=%d off=%d: mind2 err %.3e  restatement %.3e  bar %.3e' % (N, D, K, off, err, t['e32'], bar))
    assert err <= bar
    return cen, idx, w


@pytest.mark.parametrize('N,D,K', CASES)
def test_centres_match_the_truth(N, D, K):
    _check_centers(N, D, K, 0)


def _check_assign(N, D, K, off):
    t = _truth(N, D, K)
    decided = t['a']['margin'] > S.Z_MARGIN
    assert int((~decided).sum()) <= S.allowed_undecided(N), ('fixture', int((~decided).sum()))
    xg, cg = _dev(t['x'], off), _dev(t['c']['centers'])
    out = []
    for smooth in (0.0, 0.1):
        r, z = _mix().diag_seed_assign(xg, cg, smooth=smooth, want_z=True)
        torch.cuda.synchronize()
        out += [r, z]
        a = T.assign(t['x'], None, t['c']['centers'], smooth)
        assert np.array_equal(z.cpu().numpy()[decided], a['z'][decided])
        assert np.array_equal(r.cpu().numpy()[decided].view(np.uint32), a['r'][decided].view(np.uint32))
        # on the other rows r is still the rule applied to the kernel's own z
        s = np.float32(smooth)
        want = np.full((N, K), s / np.float32(K), np.float32)
        want[np.arange(N), z.cpu().numpy()] = (np.float32(1) - s) + s / np.float32(K)
        assert np.array_equal(r.cpu().numpy().view(np.uint32), want.view(np.uint32))
    return out


@pytest.mark.parametrize('N,D,K', CASES)
def test_assignment_matches_the_truth(N, D, K):
    _check_assign(N, D, K, 0)


@pytest.mark.parametrize('N,D,K', S.SAME_AS_SEED_KERNELS)
def test_the_rows_of_the_narrow_seed_kernels(N, D, K):
    """D <= 8, no mask: the same stream and the same fp32 dist2 as vmp_mixture_seed_centers - the same rows, centres and weights"""
    xg = _dev(_truth(N, D, K)['x'])
    wide = _mix().diag_seed_centers(xg, K, S.DRAW_SEED, want_index=True, want_mind2=True)
    narrow = _mix().seed_centers(xg, K, S.DRAW_SEED, want_index=True, want_mind2=True)
    assert torch.equal(wide[1], narrow[1])
    assert torch.equal(_bits(wide[0]), _bits(narrow[0])) and torch.equal(_bits(wide[2]), _bits(narrow[2]))


@pytest.mark.parametrize('N,D,K', S.UNALIGNED)
def test_a_view_offset_by_one_float_gives_the_same_bits(N, D, K):
    aligned = _check_centers(N, D, K, 0)
    shifted = _check_centers(N, D, K, 1)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(aligned, shifted))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_check_assign(N, D, K, 0), _check_assign(N, D, K, 1)))


def test_two_runs_and_every_output_set_give_the_same_bits():
    N, D, K = 2049, 64, 64
    xg = _dev(_truth(N, D, K)['x'])
    mix = _mix()
    full = mix.diag_seed_centers(xg, K, S.DRAW_SEED, want_index=True, want_mind2=True)
    again = mix.diag_seed_centers(xg, K, S.DRAW_SEED, want_index=True, want_mind2=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full, again))
    for wi, wm in ((False, False), (True, False), (False, True)):
        cen, idx, w = mix.diag_seed_centers(xg, K, S.DRAW_SEED, want_index=wi, want_mind2=wm)
        assert torch.equal(_bits(cen), _bits(full[0]))
        assert (idx is None) == (not wi) and (w is None) == (not wm)
        assert idx is None or torch.equal(idx, full[1])
        assert w is None or torch.equal(_bits(w), _bits(full[2]))
    other = mix.diag_seed_centers(xg, K, S.DRAW_SEED + 1, want_index=True)[1]
    assert not torch.equal(other, full[1])                                      # the seed enters
    r1, z1 = mix.diag_seed_assign(xg, full[0], smooth=0.1, want_z=True)
    r2, z2 = mix.diag_seed_assign(xg, full[0], smooth=0.1, want_z=True)
    r3, z3 = mix.diag_seed_assign(xg, full[0], smooth=0.1)
    assert torch.equal(r1, r2) and torch.equal(z1, z2) and torch.equal(r1, r3) and z3 is None
    # the C entry point with z_out alone (the Python wrapper always asks for r)
    import vmp_for_svae_amd as V
    L = V._lib
    z4 = torch.empty(N, dtype=torch.int32, device='cuda')
    L.check(L.lib().vmp_mixture_diag_seed_assign(L.ptr(xg), N, D, K, L.ptr(full[0]), 0.1, None, L.ptr(z4), L.stream()), 'assign')
    assert torch.equal(z4, z1)


@pytest.mark.parametrize('N,D,K', [(3, 64, 5), (63, 17, 64)])
def test_fewer_rows_than_centres_repeat_centres_as_the_truth_does(N, D, K):
    t = _truth(N, D, K)
    cen, idx, _ = _mix().diag_seed_centers(_dev(t['x']), K, S.DRAW_SEED, want_index=True)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, t['c']['index']) and len(set(idx.tolist())) <= N
    assert np.array_equal(cen.cpu().numpy().view(np.uint32), t['x'][idx].view(np.uint32))


# fp64 truth (mix_diag_truth.iterate, default prior, data seed 0, draw seed 1; computed on the CPU, tests/mix_diagseed_truth.py E2E):
# bound after ten iterations from the truth's k-means++ r_init -73233.3776, from the Dirichlet r_init of gmm.inference_diag
# -74600.0389: gap 1366.6613 nats.
TRUTH_GAP = 1366.6613


def test_a_seeded_fit_reaches_a_higher_bound_than_the_random_start():
    """Four unit-variance clusters eight standard deviations apart in D = 24 (N = 2048, K = 4): lower_bound() of
    DiagLoop.from_seed(...) after ten iterations must exceed that of the loop started from the random Dirichlet r_init with the same
    (default) prior by at least half the gap of the fp64 truth: -73233.3776 against -74600.0389, gap 1366.6613 nats, margin 683.33."""
    from vmp_for_svae_amd.models import gmm
    mix, E = _mix(), S.E2E
    x = S.four_clusters_wide()
    prior = DT.default_prior(x, E['K'])
    c = T.centers(x, None, None, E['K'], E['seed'])
    a = T.assign(x, None, c['centers'])
    r_rand = S.dirichlet_r_init(E['N'], E['K'], E['seed'])
    gap = DT.iterate(x, a['r'], prior, E['iterations'])['bound'] - DT.iterate(x, r_rand, prior, E['iterations'])['bound']
    assert gap > 0 and abs(gap - TRUTH_GAP) < 1e-3 * TRUTH_GAP, ('fixture', gap)          # the fixture condition, and the docstring's figure
    xg = _dev(x)
    seeded = mix.DiagLoop.from_seed(xg, E['K'], E['seed'])
    seeded.run(E['iterations'])
    r0 = gmm._dirichlet_init(E['N'], E['K'], E['seed'], xg.device)
    assert np.array_equal(r0.cpu().numpy(), r_rand)
    random = mix.DiagLoop(xg, r0)
    random.run(E['iterations'])
    b_seed, b_rand = seeded.lower_bound(), random.lower_bound()
    print('bound: seeded %.4f  random %.4f  gap %.4f  (truth gap %.4f)' % (b_seed, b_rand, b_seed - b_rand, gap))
    assert b_seed - b_rand >= 0.5 * gap


def test_from_seed_is_centres_then_assign_then_the_r_in_pass():
    N, D, K = 4099, 9, 33
    mix = _mix()
    xg = _dev(_truth(N, D, K)['x'])
    for smooth in (0.0, 0.1):
        a = mix.DiagLoop.from_seed(xg, K, S.DRAW_SEED, smooth=smooth).stats
        b = mix.DiagLoop(xg, mix.diag_seed_assign(xg, mix.diag_seed_centers(xg, K, S.DRAW_SEED)[0], smooth)[0]).stats
        assert torch.equal(a, b) and a.dtype == torch.float64


def test_inference_diag_starts_from_the_seed_and_an_explicit_r_init_still_wins():
    from vmp_for_svae_amd.models import gmm
    E = S.E2E
    xg = _dev(S.four_clusters_wide())
    step, log_r, theta, aux = gmm.inference_diag(xg, E['K'], E['seed'], init='kmeans++')
    r = step()
    loop = _mix().DiagLoop.from_seed(xg, E['K'], E['seed'])
    assert torch.equal(r, loop.step())                                          # the start of from_seed
    assert torch.isfinite(r).all() and torch.allclose(r.sum(1), torch.ones_like(r[:, 0]), atol=1e-5)
    assert all(torch.isfinite(t).all() for t in theta()) and all(torch.isfinite(t).all() for t in aux())
    r0 = gmm._dirichlet_init(E['N'], E['K'], 3, xg.device)
    a = gmm.inference_diag(xg, E['K'], 0, r_init=r0, init='kmeans++')[0]()
    b = gmm.inference_diag(xg, E['K'], 0, r_init=r0)[0]()
    assert torch.equal(a, b)
