"""Mixture initialisation on the device (csrc/vmp_seed.hip; include/vmp_hip.h "Mixture initialisation") against the fp64 truth of
tests/mix_seed_truth.py: the chosen rows and the centres bit for bit, the final weights within the bar of the fp32 restatement, the
assignment on every row the truth can decide, determinism, and fits started from the seeded responsibilities."""
import functools

import numpy as np
import pytest
import torch

import mix_missfit_truth as M
import mix_seed_truth as T

pytestmark = pytest.mark.gpu

CASES = [(N, D, K, masked) for (N, D, K) in T.SWEEP for masked in (False, True)]


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


@functools.lru_cache(maxsize=None)
def _truth(N, D, K, masked):
    """the case, its fill as the DEVICE computes it (the column means of mean_filled), and the truth from that fill: computed once"""
    x, miss, fill = T.case(N, D, K, masked)
    if masked:
        dev_fill = _mix()._observed_mean(_dev(x), _dev(miss) != 0).cpu().numpy()
        assert np.allclose(dev_fill, fill, rtol=1e-6, atol=1e-7)
        fill = dev_fill
    c = T.centers(x, miss, fill, K, T.DRAW_SEED)
    a = T.assign(x, miss, c['centers'])
    return dict(x=x, miss=miss, fill=fill, c=c, a=a, e32=T.restatement_error(x, miss, fill, K, T.DRAW_SEED, c))


def _check_centers(N, D, K, masked, off):
    t = _truth(N, D, K, masked)
    c = t['c']
    assert c['margin'].min() >= T.MARGIN, ('fixture', c['margin'].min())                 # a condition on the fixture, every round
    xg = _dev(t['x'], off)
    mg = _dev(t['miss'], 1 if off else 0) if masked else None
    cen, idx, w = _mix().seed_centers(xg, K, T.DRAW_SEED, miss=mg, want_index=True, want_mind2=True)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), c['index'])
    assert np.array_equal(cen.cpu().numpy().view(np.uint32), c['centers'].view(np.uint32))   # the bits of x~ at those rows
    err = float(np.max(np.abs(w.cpu().numpy().astype(np.float64) - c['w']) / np.maximum(1.0, np.abs(c['w']))))
    bar = max(1e-5, 3 * t['e32'])
    print('N=%d D=%d K=%d masked=%d off=%d: mind2 err %.3e  restatement %.3e  bar %.3e' % (N, D, K, masked, off, err, t['e32'], bar))
    assert err <= bar


@pytest.mark.parametrize('N,D,K,masked', CASES)
def test_centres_match_the_truth(N, D, K, masked):
    _check_centers(N, D, K, masked, 0)


@pytest.mark.parametrize('N,D,K', T.UNALIGNED)
@pytest.mark.parametrize('masked', [False, True])
def test_centres_from_a_view_that_breaks_the_alignment(N, D, K, masked):
    _check_centers(N, D, K, masked, 1)


def _check_assign(N, D, K, masked, off):
    t = _truth(N, D, K, masked)
    a = t['a']
    decided = a['margin'] > T.Z_MARGIN
    left_out = int((~decided).sum())
    assert left_out <= 0.005 * N or (N < 800 and left_out <= 4), ('fixture', left_out)
    xg = _dev(t['x'], off)
    mg = _dev(t['miss'], 1 if off else 0) if masked else None
    cg = _dev(t['c']['centers'])
    for smooth in (0.0, 0.1):
        r, z = _mix().seed_assign(xg, cg, miss=mg, smooth=smooth, want_z=True)
        torch.cuda.synchronize()
        z, r = z.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(z[decided], a['z'][decided])
        assert np.array_equal(z < 0, a['z'] < 0)
        s = np.float32(smooth)
        lo = s / np.float32(K)
        want = np.full((N, K), lo, np.float32)
        want[np.arange(N), np.maximum(z, 0)] = (np.float32(1) - s) + lo
        want[z < 0] = np.float32(1) / np.float32(K)
        assert np.array_equal(r.view(np.uint32), want.view(np.uint32))
        if smooth == 0.1:
            assert np.array_equal(want[decided], T.assign(t['x'], t['miss'], t['c']['centers'], smooth)['r'][decided])


@pytest.mark.parametrize('N,D,K,masked', CASES)
def test_assignment_matches_the_truth(N, D, K, masked):
    _check_assign(N, D, K, masked, 0)


@pytest.mark.parametrize('N,D,K', T.UNALIGNED)
def test_assignment_from_a_view_that_breaks_the_alignment(N, D, K):
    _check_assign(N, D, K, True, 1)


def test_two_runs_and_every_output_set_give_the_same_bits():
    N, D, K = 4099, 8, 64
    t = _truth(N, D, K, True)
    xg, mg = _dev(t['x']), _dev(t['miss'])
    mix = _mix()
    full = mix.seed_centers(xg, K, T.DRAW_SEED, miss=mg, want_index=True, want_mind2=True)
    again = mix.seed_centers(xg, K, T.DRAW_SEED, miss=mg, want_index=True, want_mind2=True)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(full, again))
    for wi, wm in ((False, False), (True, False), (False, True)):
        cen, idx, w = mix.seed_centers(xg, K, T.DRAW_SEED, miss=mg, want_index=wi, want_mind2=wm)
        assert torch.equal(cen.view(torch.int32), full[0].view(torch.int32))
        assert (idx is None) == (not wi) and (w is None) == (not wm)
        assert idx is None or torch.equal(idx, full[1])
        assert w is None or torch.equal(w.view(torch.int32), full[2].view(torch.int32))
    other = mix.seed_centers(xg, K, T.DRAW_SEED + 1, miss=mg, want_index=True)[1]
    assert not torch.equal(other, full[1])                                      # the seed enters
    r1, z1 = mix.seed_assign(xg, full[0], miss=mg, smooth=0.1, want_z=True)
    r2, z2 = mix.seed_assign(xg, full[0], miss=mg, smooth=0.1, want_z=True)
    r3, z3 = mix.seed_assign(xg, full[0], miss=mg, smooth=0.1)
    assert torch.equal(r1, r2) and torch.equal(z1, z2) and torch.equal(r1, r3) and z3 is None


# fp64 oracle, data seed 0 (tests/mix_seed_truth.py four_clusters), held-out mean log predictive density after 10 iterations:
#   complete rows   oracle.mixtures.gmm_inference_step from the truth's k-means++ r_init -5.6414, from the Dirichlet r_init of
#                   gmm.inference -6.3418: gap 0.7005 nats per row (data seeds 1, 2, 3: 0.6658, 0.5803, 0.7827);
#   25 % missing    mix_missfit_truth.iterate: -5.6410 against -7.1991: gap 1.5581 (data seeds 1, 2, 3: 1.3310, 1.7122, 1.7828).
E2E_SEED = 0
ORACLE_GAP_FULL = 0.7005
ORACLE_GAP_MISS = 1.5581


def test_a_seeded_fit_beats_the_random_start_after_ten_iterations():
    """Four clusters eight standard deviations apart, N = 2048, D = 3, K = 4, 512 held-out rows: VMPLoop.from_seed(...).run(10) must
    score higher on the held-out rows than the loop of gmm.inference's random r_init after run(10), by at least half the gap the fp64
    oracle shows for this data seed: -5.6414 against -6.3418, gap 0.7005 nats per row (at least 0.1 was asked of the seed)."""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import gmm
    mix = _mix()
    x, xv, _ = T.four_clusters(E2E_SEED)
    xg, xvg = _dev(x), _dev(xv)
    seeded = mix.VMPLoop.from_seed(xg, 4, V._lib.VMP_GMM, E2E_SEED)
    seeded.run(10)
    random = mix.VMPLoop(xg, gmm._dirichlet_init(2048, 4, E2E_SEED, xg.device), V._lib.VMP_GMM)
    random.run(10)
    s_seed, s_rand = seeded.score(xvg), random.score(xvg)
    print('held-out score: seeded %.4f  random %.4f  gap %.4f  (oracle gap %.4f)' % (s_seed, s_rand, s_seed - s_rand, ORACLE_GAP_FULL))
    assert ORACLE_GAP_FULL >= 0.1
    assert s_seed - s_rand >= 0.5 * ORACLE_GAP_FULL
    # the start itself is the truth's: r_init of from_seed = the truth's assignment on every row it can decide
    c = T.centers(x, None, None, 4, E2E_SEED)
    a = T.assign(x, None, c['centers'])
    r0 = mix.seeded_r_init(xg, 4, E2E_SEED).cpu().numpy()
    ok = a['margin'] > T.Z_MARGIN
    assert c['margin'].min() >= T.MARGIN and np.array_equal(r0[ok], a['r'][ok])


def test_a_seeded_fit_on_partly_observed_rows_beats_the_random_start():
    """The same data with 25 % of the entries missing, through gmm.inference_missing(init='kmeans++') against init='random', ten
    steps each, scored on the complete held-out rows.  fp64 oracle (mix_missfit_truth.iterate from the truth's two r_init):
    -5.6410 against -7.1991, gap 1.5581 nats per row; the margin is half of it."""
    from vmp_for_svae_amd.models import gmm
    x, xv, miss = T.four_clusters(E2E_SEED, frac=0.25)
    x = x.copy()
    x[miss != 0] = np.nan
    xg, mg, xvg = _dev(x), _dev(miss), _dev(xv)
    scores = []
    for init in ('kmeans++', 'random'):
        step, _, theta, _, filled = gmm.inference_missing(xg, mg, 4, E2E_SEED, init=init)
        for _ in range(10):
            step()
        assert torch.isfinite(filled()).all()
        _, total = gmm.predictive_logprob(xvg, *theta())
        scores.append(total.item() / xv.shape[0])
    print('held-out score: seeded %.4f  random %.4f  gap %.4f  (oracle gap %.4f)' % (scores[0], scores[1], scores[0] - scores[1], ORACLE_GAP_MISS))
    assert ORACLE_GAP_MISS >= 0.1
    assert scores[0] - scores[1] >= 0.5 * ORACLE_GAP_MISS


def test_the_student_t_mixture_starts_from_the_seed():
    from vmp_for_svae_amd.models import smm
    x, _, _ = T.four_clusters(E2E_SEED)
    step, log_r, theta, aux = smm.inference(_dev(x), 4, 5.0, E2E_SEED, init='kmeans++')
    for _ in range(3):
        r = step()
    torch.cuda.synchronize()
    lr = log_r()
    assert torch.isfinite(r).all() and not torch.isnan(lr).any() and (lr <= 0).all()     # log r = -inf where r underflows to 0
    assert torch.allclose(r.sum(1), torch.ones_like(r[:, 0]), atol=1e-5)
    assert all(torch.isfinite(t).all() for t in theta()) and all(torch.isfinite(t).all() for t in aux())


def test_an_explicit_r_init_still_wins():
    from vmp_for_svae_amd.models import gmm
    x, _, _ = T.four_clusters(E2E_SEED, N=300, M=1)
    xg = _dev(x)
    r0 = gmm._dirichlet_init(300, 4, 3, xg.device)
    a = gmm.inference(xg, 4, 0, r_init=r0, init='kmeans++')[0]()
    b = gmm.inference(xg, 4, 0, r_init=r0)[0]()
    assert torch.equal(a, b)
