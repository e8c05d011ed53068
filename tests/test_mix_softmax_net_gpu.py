"""The reduce-scatter softmax network of the XDL mixture pass (csrc/vmp_mix.hip: row16_rs4_max / row16_rs4_sum / row16_bcast_bank,
one reciprocal per lane) against the all-reduce helpers it replaces on whole tiles - bit for bit, inside ONE build.

The E-pass vmp_mix_estep without stats gives every row an r (and, Student-t, a u) that depends on that row and the pack alone.  The
same rows run once as whole 64-row tiles of K = 16 (straight-line path: the new network) and once through the general form (ragged
tile: row16_max2 / row16_sum2, four reciprocals), and must agree with torch.equal:

  * the N-call, N a multiple of 64 and every wave's share a multiple of 64 (asserted on vmp_mix_pass_plan): whole tiles only;
  * the call on the first N - 24 rows: its last tile holds 40 rows = a full 32-row body and a masked one of the general form;
  * calls on windows of 63 rows of the same x (x[s : s + 63], s = 0, 63, ...): one wave, one ragged tile each, so that EVERY row of
    the N-call has a general-form twin, at shifting positions of the tile (and shifting row alignment: both row-load forms).

Inputs: the pack of one finalize on seeded data around 16 centres.  Row n sits at centre n mod 16, so that in every 16-lane DPP row
every bank meets the winning component in turn; a quarter of the rows - one register of every DPP row, rotating - is pushed far
out, where the components' log rho spread over more than 60 (asserted on r), so that a row normalised with a neighbouring row's
maximum or sum cannot pass.  Every row's r sums to 1 within 4 ulp of 1 (2^-23): r_k = e_k * rcp(S) with S the rounded sum of the e_k
carries the rounding of S, of the 1-ulp v_rcp_f32 and of the product - below 3 ulp of 2^-24 each, summed over a row."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 16
KAPPA = 5.0
WINDOW = 63


def _centres(D):
    rng = np.random.Generator(np.random.PCG64(100 + D))
    c = rng.standard_normal((K, D)) * 3
    c[:, 0] = 10.0 * np.arange(K)                      # ten standard deviations apart along the first axis whatever D is
    return c


@functools.lru_cache(maxsize=None)
def _pack(D, smm):
    """E-step pack of one finalize (hard assignments of 128 rows per centre); computed once per (D, flavour), never modified"""
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    rng = np.random.Generator(np.random.PCG64(7 + D))
    c = _centres(D)
    z = np.arange(128 * K) % K
    x = (c[z] + rng.standard_normal((z.size, D))).astype(np.float32)
    r0 = np.zeros((z.size, K), np.float32)
    r0[np.arange(z.size), z] = 1
    lp = _mix.VMPLoop(torch.as_tensor(x).cuda(), torch.as_tensor(r0).cuda(), L.VMP_SMM if smm else L.VMP_GMM,
                      kappa=torch.full((K,), KAPPA, device='cuda') if smm else None)
    lp.finalize()
    torch.cuda.synchronize()
    return lp.post['pack'].clone()


def _far(n):
    """row n = sub-tile s, register v, DPP row kk (row = 16 s + 4 v + kk): one register of every DPP row, rotating with s"""
    s, v, kk = n // 16, (n % 16) // 4, n % 4
    return (s + v + kk) % 4 == 0


@functools.lru_cache(maxsize=None)
def _rows(N, D):
    rng = np.random.Generator(np.random.PCG64(N + D))
    c = _centres(D)
    n = np.arange(N)
    x = c[n % K] + 0.3 * rng.standard_normal((N, D))
    far = _far(n)
    x[far] += 25.0 * np.sign(rng.standard_normal((int(far.sum()), D)))
    return torch.as_tensor(x.astype(np.float32)).cuda(), torch.as_tensor(far)


def _estep(x, pack, smm):
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    r, u, _, _ = _mix.estep(x, pack, L.VMP_SMM if smm else L.VMP_GMM)
    return r, u


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('D', [1, 4, 5, 8])
@pytest.mark.parametrize('N', [64, 128, 8 * 64 * 2])
def test_whole_tiles_equal_the_general_form_bit_for_bit(N, D, flavour):
    from vmp_for_svae_amd import _lib as L
    smm = flavour == 'smm'
    plan = (ctypes.c_int64 * 8)()
    assert L.lib().vmp_mix_pass_plan(N, D, K, L.VMP_SMM if smm else L.VMP_GMM, 1, 0, 0, plan) == 0
    assert plan[0] == 2 and plan[4] % 64 == 0 and plan[5] % 64 == 0, list(plan)      # XDL form, every wave's share = whole tiles
    pack = _pack(D, smm)
    x, far = _rows(N, D)
    r, u = _estep(x, pack, smm)
    what = '%s N=%d D=%d' % (flavour, N, D)

    # the inputs are what the docstring says
    assert torch.isfinite(r).all(), what
    win = r.argmax(1).cpu()
    assert torch.equal(win[~far], (torch.arange(N) % K)[~far]), what
    rf = r[far.to(r.device)].double()
    assert far.sum() == N // 4 and (rf.min(1).values < np.exp(-60.0) * rf.max(1).values).all(), what
    err = (r.double().sum(1) - 1.0).abs().max().item()
    print('%s: max |sum_k r - 1| = %.3e (bar %.3e)' % (what, err, 4 * 2.0 ** -23))
    assert err <= 4 * 2.0 ** -23, what

    # the ragged last tile of the shorter call (40 rows) and its whole tiles ahead of it
    rt, ut = _estep(x[:N - 24], pack, smm)
    assert torch.equal(rt, r[:N - 24]), what + ' N - 24 rows: r'
    assert not smm or torch.equal(ut, u[:N - 24]), what + ' N - 24 rows: u'
    # every row's general-form twin
    for s in range(0, N, WINDOW):
        e = min(s + WINDOW, N)
        rw, uw = _estep(x[s:e], pack, smm)
        assert torch.equal(rw, r[s:e]), what + ' rows %d..%d: r' % (s, e - 1)
        assert not smm or torch.equal(uw, u[s:e]), what + ' rows %d..%d: u' % (s, e - 1)
