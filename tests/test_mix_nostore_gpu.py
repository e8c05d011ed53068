"""The fused mixture pass without its r / u stores (csrc/vmp_mix.hip, pass_xdl_body<.., KEEP = false>; vmp_mixture_estep_fused_nostore,
vmp_mixture_iterate_nostore) and the loop that runs it (models/_mix.py: VMPLoop.stream_phase / run, the lazy `r` / `u` properties).

Three iterations from the same x and r0, once with the storing entry point called directly (vmp_mix_finalize_ws + vmp_mix_estep_fused
on the loop's buffers) and once through finalize_phase() + stream_phase().  Everything is compared bit for bit - the no-store instance
runs the statements of the storing one, less the stores:
  1. the workspace (per-block fp64 partials) after every iteration.  Both workspaces start from the same bytes, so the words no pass
     writes agree as well;
  2. the posterior arrays after every iteration;
  3. `r` (and `u`) read after the third iteration: one E-only pass from the current pack and the loop's pivot;
  4. a second read launches nothing and returns the same tensor object;
  5. the r / u buffers are filled with NaN before every no-store iteration and must still be all NaN after it, before any read.
run(3) - two no-store iterations, then a storing one, so that r is current when it returns and no E-only pass is ever launched for
it - must leave the same workspace, posterior and r.
Shapes, for both flavours and D in {1, 3, 8}: K = 16, N = 1 088 (the instance of whole tiles alone: 17 waves of one tile); K = 16,
N = 65 573 (N mod 64 = 37: a last wave of 37 rows, 2-term moment operands); K = 10, N = 4 099 (general instance, 3-term operands);
K = 16, N = 131 073 (waves of 72 rows and a last one of 33: the general instance with 2-term operands); K = 16, N = 147 456 (2 048
waves of 72 rows: the instance of whole tiles with every wave's last 8 rows as an overlapping tile).  K = 17 runs the tiled pass,
which has no such instance: the new entry points refuse on the host and the loop keeps the storing call."""
import pytest
import torch

from mix_pass_truth import KAPPA

pytestmark = pytest.mark.gpu

POST = ('alpha', 'beta', 'm', 'C', 'v', 'xbar', 'S', 'pi')
ENTRIES = ('vmp_mix_estep', 'vmp_mix_estep_fused', 'vmp_mixture_estep_fused_nostore', 'vmp_mixture_iterate_nostore', 'vmp_mix_iterate')


def _data(N, D, K):
    g = torch.Generator(device='cuda').manual_seed(7 * N + D + K)
    c = torch.randn(K, D, device='cuda', generator=g) * 5
    x = c[torch.randint(0, K, (N,), device='cuda', generator=g)] + torch.randn(N, D, device='cuda', generator=g)
    r0 = torch.softmax(3 * torch.randn(N, K, device='cuda', generator=g), 1)
    return x.contiguous(), r0


def _loops(N, D, K, flavour, n, cls=None):
    """n loops of the same x, r0 whose workspaces hold the same bytes (the words no pass writes included)"""
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    smm = flavour == 'smm'
    fl = L.VMP_SMM if smm else L.VMP_GMM
    x, r0 = _data(N, D, K)
    loops = [(cls or _mix.VMPLoop)(x, r0, fl, kappa=torch.full((K,), KAPPA, device='cuda') if smm else None) for _ in range(n)]
    for lp in loops[1:]:
        lp.ws.copy_(loops[0].ws)
    return loops, fl, smm


def _count(monkeypatch):
    """calls of the streaming entry points, by name: the library handle's attributes are wrapped, every caller goes through them"""
    from vmp_for_svae_amd import _lib as L
    calls = dict.fromkeys(ENTRIES, 0)

    def wrap(name, fn):
        def counted(*a):
            calls[name] += 1
            return fn(*a)
        return counted
    for name in ENTRIES:
        monkeypatch.setattr(L.lib(), name, wrap(name, getattr(L.lib(), name)), raising=False)
    return calls


def _storing_step(lp):
    """one iteration through the entry points as they were: vmp_mix_finalize_ws, then vmp_mix_estep_fused into the loop's buffers"""
    from vmp_for_svae_amd import _lib as L
    lp.finalize()
    L.check(L.lib().vmp_mix_estep_fused(L.ptr(lp.x), lp.N, lp.D, lp.K, lp.flavour, L.ptr(lp.post['pack']), L.ptr(lp._r), L.ptr(lp._u), None,
                                        L.ptr(lp.pivot), L.ptr(lp.ws), lp.nb, L.stream()), 'vmp_mix_estep_fused')


def _same_state(a, b, what):
    assert torch.equal(a.ws, b.ws), what + 'workspace partials'
    for k in POST:
        assert torch.equal(a.post[k], b.post[k]), what + k


def _all_nan(t):
    return bool(torch.isnan(t).all())


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('D', [1, 3, 8])
@pytest.mark.parametrize('N,K', [(64 * 8 * 2 + 64, 16), (65573, 16), (4099, 10), (131073, 16), (147456, 16)])
def test_nostore_iterations_leave_the_bits_of_the_storing_ones(N, K, D, flavour, monkeypatch):
    (keep, lazy, one_call), fl, smm = _loops(N, D, K, flavour, 3)
    what = 'nostore %s N=%d D=%d K=%d: ' % (flavour, N, D, K)
    assert lazy._nostore and not lazy._stale
    calls = _count(monkeypatch)
    for it in range(3):
        _storing_step(keep)
        lazy._r.fill_(float('nan'))
        if smm:
            lazy._u.fill_(float('nan'))
        lazy.finalize_phase()
        lazy.stream_phase()
        assert _all_nan(lazy._r) and (not smm or _all_nan(lazy._u)), what + 'iteration %d wrote to r / u' % it
        _same_state(keep, lazy, what + 'iteration %d, ' % it)
    assert calls['vmp_mixture_estep_fused_nostore'] == 3 and calls['vmp_mix_estep_fused'] == 3 and calls['vmp_mix_estep'] == 0
    r = lazy.r
    assert calls['vmp_mix_estep'] == 1 and not lazy._stale
    assert torch.equal(r, keep._r), what + 'r'
    u = lazy.u
    assert not smm or torch.equal(u, keep._u), what + 'u'
    assert (u is None) == (not smm)
    assert lazy.r is r and lazy.u is u and r is lazy._r, what + 'a second read returns another tensor'
    assert calls['vmp_mix_estep'] == 1 and calls['vmp_mix_estep_fused'] == 3, what + 'a second read launched a pass'
    # the same three iterations through run(): two without the stores, the last one with them - r is current, nothing launched for it
    one_call._r.fill_(float('nan'))
    rr = one_call.run(3)
    assert calls['vmp_mixture_iterate_nostore'] == 1 and calls['vmp_mix_iterate'] == 1 and one_call.iterations == 3
    assert not one_call._stale
    _same_state(keep, one_call, what + 'run(3), ')
    assert rr is one_call.r and torch.equal(rr, keep._r) and (not smm or torch.equal(one_call.u, keep._u)), what + 'run(3), r / u'
    assert calls['vmp_mix_estep'] == 1, what + 'run(3) launched an E-only pass'
    # a storing pass after a no-store one: the buffers are current again, nothing is launched by the read
    lazy.finalize_phase()
    lazy.estep()
    n = calls['vmp_mix_estep']
    _storing_step(keep)
    assert torch.equal(lazy.r, keep._r) and calls['vmp_mix_estep'] == n, what + 'r after a storing pass'


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
def test_tiled_pass_keeps_the_storing_call(flavour, monkeypatch):
    from vmp_for_svae_amd import _lib as L
    N, D, K = 4099, 8, 17
    (keep, lazy, one_call), fl, smm = _loops(N, D, K, flavour, 3)
    what = 'nostore fallback %s K=%d: ' % (flavour, K)
    assert not lazy._nostore
    lib = L.lib()
    P = L.ptr
    post = [P(lazy.post[k]) for k in POST + ('pack',)]
    before = lazy.ws.clone()
    assert lib.vmp_mixture_estep_fused_nostore(P(lazy.x), N, D, K, fl, P(lazy.post['pack']), P(lazy.pivot), P(lazy.ws), lazy.nb, L.stream()) == -4
    assert b'K = 17' in lib.vmp_last_error()
    assert lib.vmp_mixture_iterate_nostore(P(lazy.x), N, D, K, fl, *[P(t) for t in lazy.prior], P(lazy.kappa), P(lazy.pivot), *post, P(lazy.ws),
                                           lazy.nb, 2, L.stream()) == -4
    assert torch.equal(lazy.ws, before), what + 'a refused call launched something'
    calls = _count(monkeypatch)
    for it in range(3):
        _storing_step(keep)
        lazy.finalize_phase()
        lazy.stream_phase()
        _same_state(keep, lazy, what + 'iteration %d, ' % it)
        assert torch.equal(lazy._r, keep._r) and (not smm or torch.equal(lazy._u, keep._u)), what + 'the pass stores r / u as before'
    assert calls['vmp_mix_estep_fused'] == 6 and calls['vmp_mixture_estep_fused_nostore'] == 0
    one_call.run(3)
    assert calls['vmp_mix_iterate'] == 1 and calls['vmp_mixture_iterate_nostore'] == 0 and calls['vmp_mix_estep'] == 0
    _same_state(keep, one_call, what + 'run(3), ')
    assert torch.equal(one_call.r, keep._r)


@pytest.mark.parametrize('kind', ['accurate', 'logr'])
def test_paths_that_need_r_every_step_keep_the_storing_call(kind, monkeypatch):
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import _mix
    N, D, K = 4099, 8, 16
    x, r0 = _data(N, D, K)
    loop = _mix.VMPLoop(x, r0, L.VMP_GMM, accurate=(kind == 'accurate'))
    calls = _count(monkeypatch)
    loop.finalize_phase()
    loop.stream_phase(want_logr=(kind == 'logr'))
    assert calls['vmp_mixture_estep_fused_nostore'] == 0 and not loop._stale
    assert calls['vmp_mix_estep_fused'] == (1 if kind == 'logr' else 0)
    if kind == 'logr':                                              # log r and r of the same pass: |r log r| 2^-24 <= 2.2e-8 apart
        assert float((loop.logr.exp() - loop.r).abs().max()) <= 1e-6
    r = loop.step()                                                 # step() hands r back: the storing pass, nothing lazy
    assert r is loop.r and not loop._stale and calls['vmp_mixture_estep_fused_nostore'] == 0 and calls['vmp_mix_estep'] == 0


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
def test_data_parallel_loop_of_one_rank(flavour, monkeypatch):
    """DistributedVMPLoop.run (three launches of finalize around a sum over ranks that is a no-op for one process) goes through the
    no-store pass as well, but for its last iteration: the state and r of the same loop driven through the storing pass"""
    from vmp_for_svae_amd.models.parallel_mix import DistributedVMPLoop
    (keep, lazy), fl, smm = _loops(65573, 8, 16, flavour, 2, cls=DistributedVMPLoop)
    calls = _count(monkeypatch)
    for _ in range(2):
        keep.finalize_phase()
        keep.estep()
    lazy.run(2)                                                     # one no-store iteration, then a storing one
    assert calls['vmp_mixture_estep_fused_nostore'] == 1 and calls['vmp_mix_estep_fused'] == 3 and lazy.iterations == 2
    assert not lazy._stale and calls['vmp_mix_estep'] == 0
    _same_state(keep, lazy, 'nostore data-parallel %s: ' % flavour)
    assert torch.equal(lazy.r, keep._r) and (not smm or torch.equal(lazy.u, keep._u))
