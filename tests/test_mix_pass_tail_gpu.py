"""The end of a wave's row range in the XDL mixture pass (csrc/vmp_mix.hip, pass_xdl_body, K == 16): the rows behind the last whole
64-row tile run as ONE MORE straight-line tile [hi - 64, hi) - or, when 32 rows or fewer are left, as its second half alone - that
overlaps rows the wave has already been through.  The overlapped rows' r / u are stored a second time (same bits); their moment
weight is zero.  A wave of fewer than 64 rows (the last wave of the grid at most) and every wave of K < 16 keep the general form.

The plan gives a wave more than 64 rows only above 131 072 rows (256 x 8 waves, shares a multiple of 8), and a share is never
64 + 1 or 64 + 63 rows: the shapes below put the LAST wave of the grid, which N cuts short, on 64 + rem rows for rem in
{1, 31, 32, 33, 63}, and on exactly 128 rows (no tail).  The plan is read through vmp_mix_pass_plan and every wave's case is
derived from it: the test asserts which case the last wave (and the others) hit.  N = 209 is three whole tiles and a 17-row wave
(the fallback), N = 1 041 with K = 10 the untouched general form.

Per shape, from a fixed pack (one finalize of the loop's r_init):
  1. r (and u) of the fused pass == those of the E-only pass of the same pack (no moments, same tail path), == a second fused pass
     (and its moments, bit for bit), and - the check that does not go through the overlap code - the last wave's rows == the E-only
     pass over those rows ALONE, a data set of its own in which every row sits in another tile position or in the general form;
  2. the moments (N_k, W_k, sum w x, sum w x x^T, reduced from the per-block partials) against fp64 sums over the pass's own r / u,
     at the 1e-5 relative bar tests/mix_pass_truth.py puts on what the moments give.  The rows just ahead of the last wave's tail -
     the overlapped ones - are 4 x as far out as the rest: counted twice they move a component's second moment by ~10 %;
  3. sum_k N_k == N within 1e-6 N (the bar of that module on a row sum of r).
The posterior against the fp64 oracle, at that module's bars, is checked once per flavour on the smallest of these shapes; the
existing large shapes of tests/test_mix_pass_pipeline_gpu.py (104 and 240 / 152 rows per wave) reach both tail cases as well."""
import ctypes

import pytest
import torch

import parity_log
from mix_pass_truth import KAPPA, one_step as _one_step

pytestmark = pytest.mark.gpu

TR = 64
XDL = 2
# (N, K, rows of the last non-empty wave)
SHAPES = [(1900 * 72 + 65, 16, 65), (1900 * 96 + 95, 16, 95), (1899 * 96 + 96, 16, 96), (1900 * 104 + 97, 16, 97),
          (250 * 1024 + 127, 16, 127), (250 * 1024 + 128, 16, 128), (3 * 64 + 17, 16, 17), (1024 + 17, 10, None)]
BAR = 1e-5


def _wave_ranges(N, D, K, fl, estep, stats):
    """[lo, hi) of every wave of the grid, from the plan, as pass_xdl_body derives them"""
    from vmp_for_svae_amd import _lib as L
    out = (ctypes.c_int64 * 8)()
    assert L.lib().vmp_mix_pass_plan(N, D, K, fl, estep, stats, 0, out) == 0
    form, _, nw, blocks, rpw, rpw_b = list(out)[:6]
    assert form == XDL
    rng = []
    for b in range(blocks):
        for w in range(nw):
            if rpw_b == rpw:
                lo, n = (b * nw + w) * rpw, rpw
            else:
                hw = nw // 2
                base = b * hw * (rpw + rpw_b)
                lo, n = (base + w * rpw, rpw) if w < hw else (base + hw * rpw + (w - hw) * rpw_b, rpw_b)
            rng.append((lo, min(N, lo + n)))
    return rng


def _case(lo, hi, K):
    n = hi - lo
    if n <= 0:
        return 'empty'
    if K < 16 or n < TR:
        return 'general'
    rem = n % TR
    return 'whole' if rem == 0 else ('half' if rem <= 32 else 'tile')


def _data(N, D, K, hot):
    """x around K centres, rows [hot) 4 x as far out; r_init"""
    g = torch.Generator(device='cuda').manual_seed(N + D + K)
    c = torch.randn(K, D, device='cuda', generator=g) * 5
    x = c[torch.randint(0, K, (N,), device='cuda', generator=g)] + torch.randn(N, D, device='cuda', generator=g)
    x[hot[0]:hot[1]] *= 4
    r0 = torch.softmax(3 * torch.randn(N, K, device='cuda', generator=g), 1)
    return x.contiguous(), r0


def _e_only(x, pack, pivot, fl, K):
    from vmp_for_svae_amd import _lib as L
    N, D = x.shape
    r = torch.full((N, K), -1.0, device='cuda')
    u = torch.full((N, K), -1.0, device='cuda') if fl == L.VMP_SMM else None
    L.check(L.lib().vmp_mix_estep(L.ptr(x), N, D, K, fl, L.ptr(pack), None, L.ptr(r), L.ptr(u), None, L.ptr(pivot), None, None, 0,
                                  L.stream()), 'vmp_mix_estep')
    return r, u


def _rel(got, want, what):
    e = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    parity_log.record('rel', e, BAR, what)
    return e


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('D', [8, 3])
@pytest.mark.parametrize('N,K,last', SHAPES)
def test_tail_of_a_wave(N, K, last, D, flavour):
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    smm = flavour == 'smm'
    fl = L.VMP_SMM if smm else L.VMP_GMM
    rng = _wave_ranges(N, D, K, fl, 1, 1)
    assert rng == _wave_ranges(N, D, K, fl, 1, 0)                     # the E-only pass walks the same ranges
    cases = [_case(lo, hi, K) for lo, hi in rng]
    llo, lhi = [r_ for r_, c_ in zip(rng, cases) if c_ != 'empty'][-1]
    assert lhi == N
    if K < 16:
        assert set(cases) <= {'general', 'empty'}
        hot = (0, 0)
    else:
        assert lhi - llo == last
        want = 'general' if last < TR else ('whole' if last % TR == 0 else ('half' if last % TR <= 32 else 'tile'))
        assert _case(llo, lhi, K) == want
        assert all(hi - lo >= TR for lo, hi in rng if lo < N and hi < N)          # only the wave that N cuts short can be short
        done = (last // TR) * TR
        hot = (llo + done - (TR - last % TR), llo + done) if last >= TR and last % TR else (0, 0)    # the rows the tail overlaps
    what = 'tail %s N=%d D=%d K=%d ' % (flavour, N, D, K)
    x, r0 = _data(N, D, K, hot)
    loop = _mix.VMPLoop(x, r0, fl, kappa=torch.full((K,), KAPPA, device='cuda') if smm else None)
    loop.finalize()                                                   # the fixed pack
    pack = loop.post['pack'].clone()
    loop.estep()
    r, u, st = loop.r.clone(), (loop.u.clone() if smm else None), loop.stats.clone()
    loop.post['pack'].copy_(pack)                                     # (stats reduces through finalize and restores the posterior)
    assert torch.equal(loop.post['pack'], pack)

    # 1. the same bits from the E-only pass, from a second run, and from the last wave's rows as a data set of their own
    assert torch.isfinite(r).all() and float((r.double().sum(1) - 1.0).abs().max()) <= 1e-6, what
    re_, ue_ = _e_only(x, pack, loop.pivot, fl, K)
    assert torch.equal(r, re_), what + 'r: fused pass vs E-only pass'
    assert not smm or torch.equal(u, ue_), what + 'u: fused pass vs E-only pass'
    loop.estep()
    assert torch.equal(r, loop.r) and (not smm or torch.equal(u, loop.u)), what + 'second run'
    assert torch.equal(st, loop.stats), what + 'moments of a second run'
    rs_, us_ = _e_only(x[llo:lhi], pack, loop.pivot, fl, K)
    assert torch.equal(r[llo:lhi], rs_), what + 'r: rows of the last wave vs the same rows alone'
    assert not smm or torch.equal(u[llo:lhi], us_), what + 'u: rows of the last wave vs the same rows alone'

    # 2. moments against fp64 sums over the pass's own r / u (the overlapped rows weigh ~10 % of a component's second moment)
    rd, xd = r.double(), x.double()
    wd = rd * u.double() if smm else rd
    assert _rel(st[:, 0], rd.sum(0), what + 'N_k') <= BAR
    assert _rel(st[:, 1], wd.sum(0), what + 'W_k') <= BAR
    assert _rel(st[:, 2:2 + D], wd.t() @ xd, what + 'sum w x') <= BAR
    xx = (xd[:, :, None] * xd[:, None, :]).reshape(N, D * D)
    assert _rel(st[:, 2 + D:], wd.t() @ xx, what + 'sum w x x^T') <= BAR
    # 3. every row counted once
    assert abs(float(st[:, 0].sum()) - N) <= 1e-6 * N, what + 'sum_k N_k'


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
def test_one_fused_step_vs_oracle_on_an_overlap_tail(flavour):
    """every wave 72 rows (one whole tile, then the half-tile overlap), the last one 65: the posterior against the fp64 oracle"""
    N = SHAPES[0][0]
    assert {_case(lo, hi, 16) for lo, hi in _wave_ranges(N, 8, 16, 1 if flavour == 'smm' else 0, 1, 1)} - {'empty'} == {'half'}
    _one_step(N, 8, 16, flavour, cached=False)
