"""The XDL mixture pass (csrc/vmp_mix.hip, pass_xdl_body) flushes its fp32 moment accumulators into fp64 every VMP_XDL_MOM_FLUSH-th
tile (FLUSH below) and after the wave's last tile.  What a row's r / u / logr are must not depend on the wave's row state (its range,
the tile's first row and row count, the flush test), and the moments must hold their bars with the longer fp32 accumulation.

1. r, u and logr do not depend on where in a wave's range, or in a tile, a row sits: one fused pass from a fixed pack, then the same
   rows again ALONE (two slices that start at rows 37 and N / 2 + 5, so that every row lands in another tile position, another wave
   and, for the short slices, another kernel form), bit for bit; and the E-only pass of the same pack, bit for bit.  K = 16, D = 8 at
   N = 128 (two one-tile waves), 1 024 and 65 573 (whole tiles and the overlap tail); K = 10, D = 3 at N = 4 099 (the general form).
   With and without logr (the logr stores sit in a branch of their own).
2. The moments across a flush boundary, against fp64 sums over the pass's own r / u, at the bars of tests/test_mix_pass_tail_gpu.py
   (1e-5 relative, sum_k N_k within 1e-6 N), and the same bits from a second run.  The plan gives a wave more than one tile only from
   131 072 rows on: N = 400 037 (waves of 240 / 152 rows with the SMM's split, 248 / 144 with the GMM's: 4 and 3 tiles), and the smallest N at which the older waves of BOTH
   flavours have more than FLUSH whole tiles, so that a flush falls inside the whole-tile loop and another after the last tile.
   pass_plan gives a SIMD pair pr = ceil(N / 1024) rows rounded up to a multiple of 8, of which the older wave takes
   ra = ((pr * split / 100 + 4) / 8) * 8 with split = 64 (GMM), 62 (SMM).  ra > 64 FLUSH first holds at ra = 64 FLUSH + 8; the
   smallest pr (a multiple of 8) that gives it for the SMM's smaller split is found below by walking pr, and N = 1024 (pr - 8) + 1
   is the first row count that rounds up to it.  The test asserts the tile counts it relies on from vmp_mix_pass_plan."""
import ctypes

import pytest
import torch

import parity_log
from mix_pass_truth import KAPPA

pytestmark = pytest.mark.gpu

TR = 64
XDL = 2
FLUSH = 16
BAR = 1e-5


def _older_rows(pr, split):
    return (pr * split // 100 + 4) // 8 * 8


def _first_n_past_flush():
    pr = 8
    while min(_older_rows(pr, 64), _older_rows(pr, 62)) <= TR * FLUSH:
        pr += 8
    return 1024 * (pr - 8) + 1


N_FLUSH = _first_n_past_flush()


def _plan(N, D, K, fl):
    from vmp_for_svae_amd import _lib as L
    out = (ctypes.c_int64 * 8)()
    assert L.lib().vmp_mix_pass_plan(N, D, K, fl, 1, 1, 0, out) == 0
    form, _, nw, blocks, rpw, rpw_b = list(out)[:6]
    assert form == XDL
    return nw, blocks, rpw, rpw_b


def _data(N, D, K):
    g = torch.Generator(device='cuda').manual_seed(N + D + K)
    c = torch.randn(K, D, device='cuda', generator=g) * 5
    x = c[torch.randint(0, K, (N,), device='cuda', generator=g)] + torch.randn(N, D, device='cuda', generator=g)
    r0 = torch.softmax(3 * torch.randn(N, K, device='cuda', generator=g), 1)
    return x.contiguous(), r0


def _loop(N, D, K, flavour):
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    smm = flavour == 'smm'
    fl = L.VMP_SMM if smm else L.VMP_GMM
    x, r0 = _data(N, D, K)
    loop = _mix.VMPLoop(x, r0, fl, kappa=torch.full((K,), KAPPA, device='cuda') if smm else None)
    loop.finalize()                                                   # the fixed pack
    return loop, x, fl, smm


def _e_only(x, pack, pivot, fl, K, want_logr):
    from vmp_for_svae_amd import _lib as L
    N, D = x.shape
    r = torch.full((N, K), -1.0, device='cuda')
    u = torch.full((N, K), -1.0, device='cuda') if fl == L.VMP_SMM else None
    logr = torch.full((N, K), -1.0, device='cuda') if want_logr else None
    L.check(L.lib().vmp_mix_estep(L.ptr(x), N, D, K, fl, L.ptr(pack), None, L.ptr(r), L.ptr(u), L.ptr(logr), L.ptr(pivot), None, None, 0,
                                  L.stream()), 'vmp_mix_estep')
    return r, u, logr


@pytest.mark.parametrize('want_logr', [False, True])
@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('N,D,K', [(128, 8, 16), (1024, 8, 16), (65573, 8, 16), (4099, 3, 10)])
def test_rows_do_not_depend_on_their_tile_position(N, D, K, flavour, want_logr):
    loop, x, fl, smm = _loop(N, D, K, flavour)
    what = 'uniform %s N=%d D=%d K=%d logr=%d ' % (flavour, N, D, K, want_logr)
    pack = loop.post['pack'].clone()
    loop.estep(want_logr)
    r, u, logr = loop.r.clone(), (loop.u.clone() if smm else None), (loop.logr.clone() if want_logr else None)
    assert torch.equal(loop.post['pack'], pack)
    assert torch.isfinite(r).all() and float((r.double().sum(1) - 1.0).abs().max()) <= 1e-6, what
    for s, e in ((0, N), (37, N), (N // 2 + 5, N - 3)):
        rs, us, ls = _e_only(x[s:e], pack, loop.pivot, fl, K, want_logr)
        assert torch.equal(r[s:e], rs), what + 'r: rows [%d, %d) alone' % (s, e)
        assert not smm or torch.equal(u[s:e], us), what + 'u: rows [%d, %d) alone' % (s, e)
        assert not want_logr or torch.equal(logr[s:e], ls), what + 'logr: rows [%d, %d) alone' % (s, e)
    loop.estep(want_logr)
    assert torch.equal(r, loop.r) and (not smm or torch.equal(u, loop.u)) and (not want_logr or torch.equal(logr, loop.logr)), what + 'second run'


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('N', [400037, N_FLUSH])
def test_moments_across_a_flush_boundary(N, flavour):
    D, K = 8, 16
    loop, x, fl, smm = _loop(N, D, K, flavour)
    nw, blocks, rpw, rpw_b = _plan(N, D, K, fl)
    assert nw == 8 and rpw > rpw_b >= TR
    tiles_old, tiles_young = -(-rpw // TR), -(-rpw_b // TR)
    if N == 400037:
        assert (rpw, rpw_b) == ((240, 152) if smm else (248, 144))
    else:
        # the older waves flush inside the whole-tile loop and after their last tile; one row fewer in N and they would not
        assert rpw // TR >= FLUSH and tiles_old > FLUSH
        assert min(_plan(N - 1, D, K, f_)[2] for f_ in (0, 1)) <= TR * FLUSH
    what = 'uniform %s N=%d (%d / %d tiles per wave) ' % (flavour, N, tiles_old, tiles_young)
    loop.estep()
    r, u, st = loop.r.clone(), (loop.u.clone() if smm else None), loop.stats.clone()
    loop.estep()
    assert torch.equal(r, loop.r) and (not smm or torch.equal(u, loop.u)), what + 'second run'
    assert torch.equal(st, loop.stats), what + 'moments of a second run'

    def rel(got, want, name):
        e = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
        parity_log.record('rel', e, BAR, what + name)
        return e
    rd, xd = r.double(), x.double()
    wd = rd * u.double() if smm else rd
    assert rel(st[:, 0], rd.sum(0), 'N_k') <= BAR
    assert rel(st[:, 1], wd.sum(0), 'W_k') <= BAR
    assert rel(st[:, 2:2 + D], wd.t() @ xd, 'sum w x') <= BAR
    xx = (xd[:, :, None] * xd[:, None, :]).reshape(N, D * D)
    assert rel(st[:, 2 + D:], wd.t() @ xx, 'sum w x x^T') <= BAR
    assert abs(float(st[:, 0].sum()) - N) <= 1e-6 * N, what + 'sum_k N_k'
