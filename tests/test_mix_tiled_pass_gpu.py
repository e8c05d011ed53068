"""The tiled form of the mixture pass (csrc/vmp_mix.hip: pass_kernel<D, KT, FLAV, ESTEP, STATS, MASK> and pass_epilogue) against
fp64 truths, over the tables of tests/mix_tiled_shapes.py - tests/test_mix_tiled_cover.py proves on the host that they reach every
(D, KT) pair, both block reductions at every KT and block size, blocks with idle waves, equal and split plans and three tiles per wave.

  1. one fused step (VMPLoop.step + finalize) of both flavours against oracle.mixtures at the bars of tests/mix_pass_truth.py;
  2. the E-only instance (_mix.estep on the loop's pack) at the same r / u bars - the loop's posterior is the M-step of r0, so the
     oracle's E-step from that posterior is the r (and u) of the same truth - and the stats-only instance (_mix.raw_stats with an
     explicit pivot: without one, batches of <= 512 rows take small_stats_kernel instead) against a direct fp64 evaluation of
     sum_n w [1 | x | x x^T] at 1e-6 relative (test_uneven_wave_shares_cover_every_row_once's figure), also for K <= 16;
  3. several tiles per wave at K > 16 (400 037 rows: split plan, 248 / 144 or 240 / 152 rows per wave) against the chunked oracle;
  4. the masked E-pass (gmm.e_step_missing_data) against oracle.mixtures.gmm_e_step(..., missing_mask=) at 1e-5 absolute, on both
     sides of K = 16: nothing missing (also against the unmasked E-pass), ~30 % missing, rows that observe nothing, and missing
     entries flagged with the byte 255.  A NaN in x under the mask is NOT a case: the kernel forms (x - m) * keep, and NaN * 0 is
     NaN by design - callers hold finite placeholders there (as the reference's x * mask does);
  5. x one float off 16-byte alignment (vec_ok = 0: scalar row loads in pass_kernel and pass_xdl_kernel): only the load instructions
     differ, the arithmetic and its order do not, so the results carry the bits of the aligned run; and one D whose pack has an odd
     number of words (word-by-word parameter loads) on such a view against the oracle.

Achieved errors go to the parity log (tests/parity_log.py)."""
import functools

import numpy as np
import pytest
import torch

import mix_pass_truth as P
import mix_tiled_shapes as S
import parity_log
import test_mix_gpu as T

pytestmark = pytest.mark.gpu

_id = lambda s: 'N%d-D%d-K%d' % s


def _flav(flavour):
    from vmp_for_svae_amd import _lib as L
    return L.VMP_SMM if flavour == 'smm' else L.VMP_GMM


# ---- 1. the fused instance -------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour', S.FLAVOURS)
@pytest.mark.parametrize('shape', S.STEP_SHAPES, ids=_id)
def test_one_fused_step_vs_oracle(shape, flavour):
    P.one_step(*shape, flavour)


# ---- 2. the E-only and the stats-only instances ---------------------------------------------------------------
@pytest.mark.parametrize('flavour', S.FLAVOURS)
@pytest.mark.parametrize('shape', S.STEP_SHAPES, ids=_id)
def test_estep_only_vs_oracle(shape, flavour):
    from vmp_for_svae_amd.models import _mix
    N, D, K = shape
    smm = flavour == 'smm'
    tr = P.truth(N, D, K, smm)
    lp = P.loop(tr[0], tr[1], smm, K)
    lp.finalize()                                                 # the posterior and pack of r0's moments (the stats-only pass made them)
    r, u, _, _ = _mix.estep(lp.x, lp.post['pack'], _flav(flavour))
    P.check_ru(r, u, tr, 'E-only %s N=%d D=%d K=%d ' % (flavour, N, D, K), smm)


def _moments(x, r, u):
    """direct fp64 [N_k | W_k | sum w x | sum w x x^T], w = r u"""
    xd, rd = torch.as_tensor(x).double(), torch.as_tensor(r).double()
    w = rd if u is None else rd * torch.as_tensor(u).double()
    return rd.sum(0), w.sum(0), w.t() @ xd, torch.einsum('nk,nd,ne->kde', w, xd, xd)


def _check_moments(st, x, r, u, what, tol=1e-6):
    N, D = x.shape
    K = r.shape[1]
    st = st.double().cpu()
    assert st.shape == (K, 2 + D + D * D) and torch.isfinite(st).all(), what
    nk, wk, sx, sxx = _moments(x, r, u)
    for n_, got, want in (('N_k', st[:, 0], nk), ('W_k', st[:, 1], wk), ('sum w x', st[:, 2:2 + D], sx),
                          ('sum w x x^T', st[:, 2 + D:].reshape(K, D, D), sxx)):
        err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
        parity_log.record('rel', err, tol, what + n_)
        assert err <= tol, (what, n_, err)


def _weights(N, K, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (0.25 + 1.5 * rng.random((N, K))).astype(np.float32)


@pytest.mark.parametrize('flavour', S.FLAVOURS)
@pytest.mark.parametrize('shape', S.STATS_SHAPES, ids=_id)
def test_stats_only_pass_vs_direct_fp64_moments(shape, flavour):
    from vmp_for_svae_amd.models import _mix
    N, D, K = shape
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    u = _weights(N, K, N + D + K) if flavour == 'smm' else None
    xd = T.dev(x)
    st = _mix.raw_stats(xd, T.dev(r0), None if u is None else T.dev(u), pivot=_mix.pivot_of(xd))
    _check_moments(st, x, r0, u, 'M-only %s N=%d D=%d K=%d ' % (flavour, N, D, K))


# ---- 3. several tiles per wave ------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour', S.FLAVOURS)
@pytest.mark.parametrize('shape', S.SEVERAL, ids=_id)
def test_one_fused_step_vs_oracle_several_tiles_per_wave(shape, flavour):
    P.one_step(*shape, flavour, cached=False)                     # used once: not kept


# ---- 4. the masked E-pass -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _posterior(N, D, K):
    """x and the fp32 posterior (alpha, beta, m, P = C^-1, v) of the oracle's M-step of r0: the device and the fp64 oracle start from
    the same rounded numbers"""
    from oracle import dists, mixtures
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    xo = torch.as_tensor(x).double()
    al, be, m, C, v = mixtures.gmm_m_step(xo, torch.as_tensor(r0).double(), *mixtures.vmp_prior(K, D, torch.float64))[:5]
    return x, tuple(t.float() for t in (al, be, m, dists.inv(C), v))


def _mask(kind, N, D, seed):
    """(bool mask for the oracle, what the device is given)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    miss = np.zeros((N, D), dtype=bool)
    if kind != 'none':
        miss = rng.random((N, D)) < 0.3
    if kind == 'empty_rows':
        miss[[0, N // 2, N - 1]] = True                           # first row, one inside, the last (ragged tile) row
    if kind == 'random' and D > 1:
        miss[miss.all(1), 0] = False                              # this kind keeps something of every row
    given = torch.as_tensor(miss).cuda()
    if kind == 'byte255':
        given = given.to(torch.uint8) * 255
    return torch.as_tensor(miss), given


@pytest.mark.parametrize('kind', S.MASK_KINDS)
@pytest.mark.parametrize('shape', S.MASKED, ids=_id)
def test_masked_estep_vs_oracle(shape, kind):
    from oracle import mixtures
    from vmp_for_svae_amd.models import gmm
    N, D, K = shape
    x, th = _posterior(N, D, K)
    miss, given = _mask(kind, N, D, N + D + K)
    what = 'masked(%s) N=%d D=%d K=%d ' % (kind, N, D, K)
    if kind == 'empty_rows':
        assert miss.all(1).sum() >= 3
    if kind == 'byte255':
        assert given.dtype == torch.uint8 and set(given.unique().tolist()) <= {0, 255} and (given == 255).any()
    want = mixtures.gmm_e_step(torch.as_tensor(x).double(), *[t.double() for t in th], missing_mask=miss)[0]
    dth = [t.cuda() for t in th]
    r, _ = gmm.e_step_missing_data(T.dev(x), *dth, given)
    assert r.shape == (N, K) and torch.isfinite(r).all(), what
    assert float((r.double().sum(1) - 1.0).abs().max()) <= 1e-6, what
    assert T.abserr(r, want.numpy(), what + 'r_nk', 1e-5) <= 1e-5, what
    gone = miss.all(1)
    if gone.any():                                                # a row that observes nothing: the prior weights of the pack, as the oracle's
        assert T.abserr(r[gone.cuda()], want[gone].numpy(), what + 'r_nk of rows without an observed entry', 1e-5) <= 1e-5, what
    if kind == 'none':
        r_plain, _ = gmm.e_step(T.dev(x), *dth)
        assert T.abserr(r, r_plain.double().cpu().numpy(), what + 'r_nk vs the unmasked E-pass', 1e-5) <= 1e-5, what


# ---- 5. unaligned rows, word-by-word parameter loads --------------------------------------------------------------
def _one_float_in(x):
    xa = T.dev(x)
    buf = torch.empty(xa.numel() + 4, dtype=torch.float32, device='cuda')
    xu = buf[1:1 + xa.numel()].view(xa.shape)
    xu.copy_(xa)
    assert xa.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    return xa, xu


@pytest.mark.parametrize('flavour', S.FLAVOURS)
@pytest.mark.parametrize('shape', S.UNALIGNED, ids=_id)
def test_unaligned_x_gives_the_same_bits(shape, flavour):
    from vmp_for_svae_amd.models import _mix
    N, D, K = shape
    smm = flavour == 'smm'
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    u0 = T.dev(_weights(N, K, 7)) if smm else None
    out = []
    for xv in _one_float_in(x):
        lp = P.loop(xv, r0, smm, K)
        assert lp.x.data_ptr() == xv.data_ptr()                   # the loop keeps the caller's view
        r = lp.step().clone()
        u = lp.u.clone() if smm else None
        lp.finalize()
        re, ue, _, _ = _mix.estep(xv, lp.post['pack'], _flav(flavour))
        st = _mix.raw_stats(xv, T.dev(r0), u0, pivot=lp.pivot)
        out.append([r, u, re, ue, st, lp.pivot] + [t.clone() for t in lp.theta()])
    names = ('r', 'u', 'E-only r', 'E-only u', 'raw_stats', 'pivot', 'alpha', 'beta', 'm', 'C', 'v')
    for n_, a, b in zip(names, *out):
        assert (a is None and b is None) or torch.equal(a, b), (flavour, shape, n_)
    assert torch.isfinite(out[0][0]).all() and float((out[0][0].double().sum(1) - 1.0).abs().max()) <= 1e-6


@pytest.mark.parametrize('flavour', S.FLAVOURS)
def test_odd_pack_words_on_an_unaligned_view_vs_oracle(flavour):
    from vmp_for_svae_amd import _lib as L
    N, D, K = S.ODD_PACK
    smm = flavour == 'smm'
    assert L.lib().vmp_mix_pack_words(D) % 2 == 1
    tr = P.truth(N, D, K, smm)
    _, xu = _one_float_in(tr[0])
    P.check_step(P.loop(xu, tr[1], smm, K), tr, 'odd pack, unaligned x: %s N=%d D=%d K=%d ' % (flavour, N, D, K), smm)
