"""The XDL mixture pass builds its E-step MFMA operands once per block, into an LDS image that every lane then reads
(csrc/vmp_mix.hip, pass_xdl_body).  One VMP iteration of both flavours - the E-only pass with pivot = NULL and the fused E + M pass
with the dataset's pivot - against oracle.mixtures in fp64, at the bars of tests/test_mix_gpu.py::test_vmp_steps_vs_oracle, on the
shapes at which the image build takes another path: one-wave blocks (fewer threads than the 16 D items), D < 4 (one-MFMA coordinates
alone), D = 5 (the first two-MFMA coordinate), K < 16 (switched-off lanes), a partial last tile, and N = 70 000 (2-term moments)."""
import functools

import numpy as np
import pytest
import torch

import parity_log
import test_mix_gpu as T

pytestmark = pytest.mark.gpu

NS = (1, 63, 65, 4097, 70000)
KAPPA = 5.0


@functools.lru_cache(maxsize=None)
def _truth(N, D, K, smm):
    """inputs, the fp64 oracle's r after one iteration, the posterior that r gives, and (SMM) the error of the oracle in the reference's
    own fp32 on that r: computed once per shape and shared, never modified"""
    from oracle import mixtures
    x, r0 = T._synth(N, D, K, seed=N + D + K)
    xo, ro = torch.as_tensor(x).double(), torch.as_tensor(r0).double()
    if not smm:
        r1 = mixtures.gmm_inference_step_chunked(xo, ro)[0]
        th = mixtures.gmm_inference_step_chunked(xo, r1)[2]
        return x, r0, r1.numpy(), [t.numpy() for t in th], 0.0
    uo = torch.ones(N, K, dtype=torch.float64)
    r1, u1 = mixtures.smm_inference_step_chunked(xo, ro, uo, KAPPA)[:2]
    th = mixtures.smm_inference_step_chunked(xo, r1, u1, KAPPA)[2]
    r32 = mixtures.smm_inference_step_chunked(torch.as_tensor(x), torch.as_tensor(r0), torch.ones(N, K), KAPPA)[0]
    return x, r0, r1.numpy(), [t.numpy() for t in th[:5]], float((r32.double() - r1).abs().max())


def _check_r(r, want, bar, what):
    assert torch.isfinite(r).all(), what
    assert float((r.double().sum(1) - 1.0).abs().max()) <= 1e-6, what
    assert T.abserr(r, want, what, bar) <= bar, what


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('K', [1, 7, 16])
@pytest.mark.parametrize('D', [1, 3, 4, 5, 8])
def test_one_iteration_vs_oracle(D, K, flavour):
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    smm = flavour == 'smm'
    fl = L.VMP_SMM if smm else L.VMP_GMM
    for N in NS:
        x, r0, r1, th1, ref32 = _truth(N, D, K, smm)
        what = '%s N=%d D=%d K=%d ' % (flavour, N, D, K)
        if smm:
            parity_log.record('abs', ref32, None, what + 'r_nk: fp32 oracle (reference dtype) vs fp64 truth')
        bar_r = max(1e-5, ref32)                                  # test_vmp_steps_vs_oracle: 1e-5, or the reference's own fp32 error
        loop = _mix.VMPLoop(T.dev(x), T.dev(r0), fl, kappa=torch.full((K,), KAPPA, device='cuda') if smm else None)
        loop.finalize()
        # E-only pass, pivot = NULL
        r_e = _mix.estep(loop.x, loop.post['pack'], fl)[0]
        _check_r(r_e, r1, bar_r, what + 'E-only r_nk')
        # fused E + M pass, the dataset's pivot; its moments through the next finalize
        assert loop.pivot is not None
        loop.estep()
        _check_r(loop.r, r1, bar_r, what + 'fused r_nk')
        loop.finalize()
        for n_, t, o in zip(('alpha', 'beta', 'm', 'C', 'v'), loop.theta()[:5], th1):
            assert T.relerr(t, o, what + n_, 1e-5) <= 1e-5, what + n_
