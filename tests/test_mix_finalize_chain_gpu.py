"""The K-sized finalize launch between two streaming passes (csrc/vmp_mix.hip: finalize_block) at the shapes where its reduction and
its posterior chain take different paths.  Every case runs ONE fused pass and ONE finalize from a seeded (x, r0), through the C ABI
(VMPLoop, as tests/test_mix_gpu.py does), and holds what the finalize launch wrote - the posterior, x_k, S_k, pi and, through the E-pass
that reads it, the E-step pack - to oracle.mixtures in fp64 on the responsibilities the fused pass itself produced.

Bars: those of tests/test_mix_gpu.py for the same quantities (test_vmp_steps_vs_oracle, test_gmm_golden, test_smm_golden): alpha, beta,
m, C, v, x_k, pi 1e-5 relative; S_k 1e-5 max(1, max x^2) absolute; r 1e-5 absolute - for the Student-t mixture the error of the oracle
in the reference's own fp32 on the same inputs where THAT is larger, measured and recorded; u 2e-5 relative; the raw moments of the
reduction-only form 1e-6 relative (test_full_size_properties).

Partial rows: the reduction sums the per-block partial rows in 16 LOGICAL groups (group lg: blocks lg, lg + 16, ... ascending, then the
groups ascending) whatever the launch's thread count; 1, 15, 16, 17 rows are less than one group round, exactly one, one past, and 255
is the headline count.  The block count of every case is asserted against vmp_mix_pass_plan, so a plan change cannot move a case.

Not here: a prior-constant table handed to the launch.  There is none: what it would take off the launch's chain was stamped at under
300 cycles (profiles/NOTES_mix_finalize_chain.md), so every entry point evaluates the prior's constants per call, on one code path."""
import ctypes

import numpy as np
import pytest
import torch

import parity_log
import test_mix_gpu as T

pytestmark = pytest.mark.gpu

KAPPA = 5.0
ROWS = {1: 475, 15: 7643, 16: 8155, 17: 8667, 255: 130523}          # partial rows -> N (512 rows per block, ragged last tile)


def _plan_blocks(N, D, K, smm):
    from vmp_for_svae_amd import _lib as L
    out = (ctypes.c_int64 * 8)()
    L.check(L.lib().vmp_mix_pass_plan(N, D, K, L.VMP_SMM if smm else L.VMP_GMM, 1, 1, 0, out), 'vmp_mix_pass_plan')
    return int(out[3])


def _loop(x, r0, smm, pivot=True):
    """VMPLoop on (x, r0); pivot=False: the same loop without the shift of the data (the seeding M-pass is run again without it)"""
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    K = r0.shape[1]
    lp = _mix.VMPLoop(T.dev(x), T.dev(r0), L.VMP_SMM if smm else L.VMP_GMM, kappa=torch.full((K,), KAPPA, device='cuda') if smm else None)
    if not pivot:
        lp.pivot = None
        L.check(L.lib().vmp_mix_stats_ws(L.ptr(lp.x), L.ptr(lp.r), L.ptr(lp.u), None, lp.N, lp.D, K, L.ptr(lp.ws), lp.nb, L.stream()),
                'vmp_mix_stats_ws')
    return lp


def _oracle_step(x, r, u, smm, dtype=torch.float64):
    """oracle.mixtures on (x, r[, u]) in `dtype`: (r_new, u_new or None, theta x 5, (x_k, S_k, pi))"""
    from oracle import mixtures
    xo, ro = torch.as_tensor(x).to(dtype), r.to(dtype)
    if not smm:
        rn, _, th, aux = mixtures.gmm_inference_step_chunked(xo, ro)
        return rn, None, th, aux
    rn, un, th, aux = mixtures.smm_inference_step_chunked(xo, ro, u.to(dtype), KAPPA)
    return rn, un, th[:5], aux


def _check_posterior(lp, th, aux, x, what):
    for n_, t, o in zip(('alpha', 'beta', 'm', 'C', 'v'), lp.theta(), th):
        assert T.relerr(t, o.numpy(), what + n_, 1e-5) <= 1e-5, what + n_
    xk, Sk, pi = lp.aux()
    assert T.relerr(xk, aux[0].numpy(), what + 'x_k', 1e-5) <= 1e-5, what
    tol_S = 1e-5 * max(1.0, float((np.asarray(x, dtype=np.float64) ** 2).max()))
    assert T.abserr(Sk, aux[1].numpy(), what + 'S_k', tol_S) <= tol_S, what
    assert T.relerr(pi, aux[2].numpy(), what + 'pi', 1e-5) <= 1e-5, what


def _one_pass_one_finalize(N, D, K, smm, pivot=True, blocks=None):
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    if blocks is not None:
        assert _plan_blocks(N, D, K, smm) == blocks, (N, D, K, smm, _plan_blocks(N, D, K, smm))
    what = '%s N=%d D=%d K=%d pivot=%d ' % ('smm' if smm else 'gmm', N, D, K, int(pivot))
    lp = _loop(x, r0, smm, pivot)
    lp.step()                                                       # the fused pass: r1 (u1) and the partial rows of their moments
    r1, u1 = lp.r.double().cpu(), (lp.u.double().cpu() if smm else None)
    lp.finalize()                                                   # the launch under test, on those partial rows
    rn, un, th, aux = _oracle_step(x, r1, u1, smm)
    _check_posterior(lp, th, aux, x, what)
    # the pack, through the E-pass that reads it
    lp.estep()
    bar = 1e-5
    if smm:
        ref32 = float((_oracle_step(x, r1, u1, smm, torch.float32)[0].double() - rn).abs().max())
        parity_log.record('abs', ref32, None, what + 'r_nk: fp32 oracle (reference dtype) vs fp64 truth')
        bar = max(1e-5, ref32)
    assert torch.isfinite(lp.r).all(), what
    assert T.abserr(lp.r, rn.numpy(), what + 'r_nk', bar) <= bar, what
    if smm:
        assert T.relerr(lp.u, un.numpy(), what + 'u_nk', 2e-5) <= 2e-5, what
    return lp


@pytest.mark.parametrize('smm', [False, True], ids=['gmm', 'smm'])
@pytest.mark.parametrize('blocks', sorted(ROWS))
def test_partial_row_counts(blocks, smm):
    """less than one round of the 16 logical groups, exactly one, one past, and the headline count; D = 8, K = 16"""
    _one_pass_one_finalize(ROWS[blocks], 8, 16, smm, blocks=blocks)


@pytest.mark.parametrize('pivot', [True, False], ids=['pivot', 'nopivot'])
@pytest.mark.parametrize('smm', [False, True], ids=['gmm', 'smm'])
@pytest.mark.parametrize('K', [1, 10, 16])
@pytest.mark.parametrize('D', [1, 5, 8])
def test_every_dimension_and_component_count(D, K, smm, pivot):
    """D x K: one lane per matrix element up to the full 8 x 8 tile of the factorising wave, one block up to 16; 17 partial rows"""
    _one_pass_one_finalize(ROWS[17], D, K, smm, pivot=pivot, blocks=17)


@pytest.mark.parametrize('smm', [False, True], ids=['gmm', 'smm'])
def test_moments_handed_in_and_reduction_only(smm):
    """the reduction-only launch (no posterior output: do_post off) against fp64 sums over the rows, then src == 1 (vmp_mix_finalize: the
    posterior from moments the caller hands in - here those just reduced; this entry point always writes the posterior) against the
    oracle.  (The hand-in path works on the un-shifted moments, the launch on the partial rows on the shifted ones: the two agree to
    the bars, not to the bit.)"""
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    N, D, K = ROWS[17], 8, 16
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    lp = _loop(x, r0, smm)
    lp.step()
    lp.finalize()
    before = {k: v.clone() for k, v in lp.post.items()}
    st = torch.empty((K, L.lib().vmp_mix_stats_words(D)), dtype=torch.float64, device='cuda')
    L.check(L.lib().vmp_mix_finalize_ws(*lp._fin_ptrs(post=False), L.ptr(st), L.stream()), 'vmp_mix_finalize_ws')
    for k, v in before.items():
        assert torch.equal(lp.post[k], v), k                         # the reduction-only launch writes no posterior
    xd, rd = torch.as_tensor(x).double(), lp.r.double().cpu()
    w = rd * lp.u.double().cpu() if smm else rd
    st = st.cpu()
    assert T.relerr(st[:, 0], rd.sum(0).numpy(), 'N_k', 1e-6) <= 1e-6 and T.relerr(st[:, 1], w.sum(0).numpy(), 'W_k', 1e-6) <= 1e-6
    assert T.relerr(st[:, 2:2 + D], (w.t() @ xd).numpy(), 'sum w x', 1e-6) <= 1e-6
    assert T.relerr(st[:, 2 + D:].reshape(K, D, D), torch.einsum('nk,nd,ne->kde', w, xd, xd).numpy(), 'sum w x x^T', 1e-6) <= 1e-6
    out = _mix.finalize(st.cuda(), lp.prior, lp.flavour, kappa=lp.kappa)
    r1, u1 = lp.r.double().cpu(), (lp.u.double().cpu() if smm else None)
    _, _, th, aux = _oracle_step(x, r1, u1, smm)
    lp.post.update(out)
    _check_posterior(lp, th, aux, x, 'moments handed in ')


def test_component_without_rows():
    """N_k = 0: the reference's un-normalised branch (gmm.py:34-36, 44-46).  The partial rows are those of the loop's own seeding
    M-pass over r0, whose third column is empty."""
    from oracle import mixtures
    N, D, K = ROWS[17], 8, 16
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    r0[:, 2] = 0.0
    r0 /= r0.sum(1, keepdims=True)
    lp = _loop(x, r0, False)
    lp.finalize()
    xo = torch.as_tensor(x).double()
    want = mixtures.gmm_inference_step_chunked(xo, torch.as_tensor(r0).double())
    assert float(want[2][0][2]) == float(mixtures.vmp_prior(K, D, torch.float64)[0][2])           # alpha_2 = alpha_0: no rows
    for t in lp.post.values():
        assert torch.isfinite(t).all()
    _check_posterior(lp, want[2], want[3], x, 'empty component ')
    lp.estep()
    assert T.abserr(lp.r, want[0].numpy(), 'empty component r_nk', 1e-5) <= 1e-5
