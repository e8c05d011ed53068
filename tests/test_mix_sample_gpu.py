"""Mixture sampling on the GPU (csrc/vmp_sample.hip): vmp_mixture_sample against the fp64 truth of tests/mix_sample_truth.py over a
shape sweep that crosses the 64-row tile edge, ragged tails, the 16-component tile edges and a grid whose waves walk a full group of
64 rows plus a ragged one while others stay empty; observed bits; garbage in missing slots; unaligned x; run-to-run and
output-set invariance; chunk invariance; the unconditional form; component frequencies; the -inf-weight and NaN-parameter rows; and
the Python surface (VMPLoop.sample / impute_draws, gmm, smm, student_t).

z must equal the truth's on every DECIDABLE row - a row none of whose decision margins (mix_sample_truth.draw) is below TAU - and x_out
on those rows is within BAR relative to 1 + |truth|.  TAU and BAR come from the fp32 restatement's own disagreement with the truth
over this sweep (profiles/NOTES_mix_sample.md; tests/test_mix_sample_truth.py asserts that they still hold and that the truth alone
leaves at most 1 % of any case undecidable)."""
import functools

import numpy as np
import pytest
import torch

import mix_impute_truth as T
import mix_sample_truth as ST

pytestmark = pytest.mark.gpu


def _mix():
    from vmp_for_svae_amd.models import _mix
    return _mix


def _cuda(d):
    return {k: torch.as_tensor(a).cuda() for k, a in d.items()}


@functools.lru_cache(maxsize=None)
def _case(N, D, K):
    return ST.case_inputs(N, D, K)


@functools.lru_cache(maxsize=None)
def _truth(N, D, K, builder, draws):
    """the fp64 draws of a sweep case: computed once, shared, never modified"""
    x, miss, t, q, seed = _case(N, D, K)
    return ST.draw(x, miss, T.pack_t(**t) if builder == 't' else T.pack_niw(**q), seed, 0, draws)


def _pack(builder, t, q):
    M = _mix()
    if builder == 't':
        c = _cuda(t)
        return M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    c = _cuda(q)
    return M.impute_pack_niw(c['alpha'], c['beta'], c['m'], c['C'], c['v'])


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(xd, z, x, miss, truth, what):
    keep = ~ST.undecidable(truth, ST.TAU)
    und = 1.0 - keep.mean()
    zt = truth['z']
    zg = z.cpu().numpy()
    e = ST.rel_err(xd.cpu().numpy(), truth['x'], keep)
    print('%s: undecidable %.4f  z mismatches on decidable rows %d  x_out err %.3e (bar %.3e)' % (what, und, (zg != zt)[:, keep].sum(), e, ST.BAR))
    assert und <= 0.01, (what, und)
    assert (zg == zt)[:, keep].all(), (what, np.argwhere((zg != zt) & keep[None, :])[:5])
    assert e <= ST.BAR, (what, e, ST.BAR)
    o = torch.as_tensor(miss == 0)
    for s in range(xd.shape[0]):
        assert torch.equal(_bits(xd[s])[o], torch.as_tensor(x).view(torch.int32)[o]), (what, s)


@pytest.mark.parametrize('draws', [1, 3])
@pytest.mark.parametrize('builder', ['t', 'niw'])
@pytest.mark.parametrize('N,D,K', ST.SWEEP)
def test_shape_sweep(N, D, K, builder, draws):
    M = _mix()
    x, miss, t, q, seed = _case(N, D, K)
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    pack = _pack(builder, t, q)
    out, z = M.mixture_sample(xd, md, pack, seed, draws=draws, want_z=True)
    assert out.shape == (draws, N, D) and z.shape == (draws, N) and z.dtype == torch.int32
    assert torch.equal(xd.cpu(), torch.as_tensor(x))
    _check(out, z, x, miss, _truth(N, D, K, builder, draws), '%s N=%d D=%d K=%d draws=%d' % (builder, N, D, K, draws))
    # two runs, with and without z_out: the same bits
    out2, z2 = M.mixture_sample(xd, md, pack, seed, draws=draws, want_z=True)
    out3, z3 = M.mixture_sample(xd, md != 0, pack, seed, draws=draws)
    assert _same(out, out2) and torch.equal(z, z2) and _same(out, out3) and z3 is None


@pytest.mark.parametrize('builder', ['t', 'niw'])
def test_full_group_plus_ragged_group_and_empty_waves(builder):
    """N = 532 481 on the capped grid of 8192 waves: 68 rows per wave (64 + a ragged 4), the last 361 waves without rows"""
    M = _mix()
    N, D, K = ST.LONG_N
    x, miss, t, q, seed = _case(N, D, K)
    out, z = M.mixture_sample(torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda(), _pack(builder, t, q), seed, want_z=True)
    _check(out, z, x, miss, _truth(N, D, K, builder, 1), '%s N=%d' % (builder, N))


def _small(N=257, D=8, K=3):
    x, miss, t, q, seed = _case(N, D, K)
    return torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda(), _pack('t', t, q), seed


def test_missing_slots_never_enter_and_alignment_does_not_matter():
    M = _mix()
    xd, md, pack, seed = _small()
    out, z = M.mixture_sample(xd, md, pack, seed, draws=3, want_z=True)
    for junk in (float('nan'), float('inf'), -float('inf'), 1e30):
        xj = torch.where(md != 0, torch.full_like(xd, junk), xd)
        oj, zj = M.mixture_sample(xj, md, pack, seed, draws=3, want_z=True)
        assert _same(out, oj) and torch.equal(z, zj), junk
    buf = torch.empty(xd.numel() + 1, device='cuda')
    view = buf[1:].view_as(xd)
    view.copy_(xd)
    assert view.data_ptr() % 16 != 0
    ou, zu = M.mixture_sample(view, md, pack, seed, draws=3, want_z=True)
    assert _same(out, ou) and torch.equal(z, zu)


def test_chunks_and_seeds():
    """rows [a, b) drawn with row0 = a are rows a .. b of the whole call; another seed is another draw"""
    M = _mix()
    xd, md, pack, seed = _small()
    out, z = M.mixture_sample(xd, md, pack, seed, draws=3, want_z=True)
    for a, b in ((0, 64), (64, 129), (129, 257), (5, 6)):
        oc, zc = M.mixture_sample(xd[a:b].contiguous(), md[a:b].contiguous(), pack, seed, draws=3, row0=a, want_z=True)
        assert _same(out[:, a:b], oc) and torch.equal(z[:, a:b], zc), (a, b)
    o2, _ = M.mixture_sample(xd, md, pack, seed + 1, draws=3)
    m = (md != 0).expand(3, -1, -1)
    assert (o2[m] != out[m]).float().mean().item() > 0.99
    full, zf = M.mixture_draw(300, pack, seed, want_z=True)
    part, zp = M.mixture_draw(100, pack, seed, row0=200, want_z=True)
    assert _same(full[200:], part) and torch.equal(zf[200:], zp)


def test_no_x_is_the_all_missing_mask():
    M = _mix()
    for (N, D, K) in ((300, 8, 3), (70, 3, 17)):
        _, _, t, q, seed = _case(*[c for c in ST.SWEEP if c[1:] == (D, K)][0])
        pack = _pack('niw', t, q)
        xa, za = M.mixture_draw(N, pack, seed, want_z=True)
        junk = torch.full((N, D), float('nan'), device='cuda')
        xb, zb = M.mixture_sample(junk, torch.ones(N, D, dtype=torch.uint8, device='cuda'), pack, seed, want_z=True)
        assert xa.shape == (N, D) and za.shape == (N,) and _same(xa, xb[0]) and torch.equal(za, zb[0])
        assert torch.isfinite(xa).all() and (za >= 0).all() and (za < K).all()


def test_a_complete_row_returns_itself_and_z_follows_resp():
    M = _mix()
    xd, md, pack, seed = _small()
    draws = 4096
    row = xd[1:2].contiguous()                                   # row 1 of every case: nothing missing
    none = torch.zeros(1, xd.shape[1], dtype=torch.uint8, device='cuda')
    out, z = M.mixture_sample(row, none, pack, seed, draws=draws, want_z=True)
    assert _same(out, row.expand(draws, 1, -1))
    resp = M.mixture_impute(row, none, pack, want_resp=True)[2][0].double().cpu().numpy()
    freq = np.bincount(z[:, 0].cpu().numpy(), minlength=3) / draws
    se = np.sqrt(resp * (1 - resp) / draws)
    assert (np.abs(freq - resp) <= 5 * se + 1e-12).all(), (freq, resp, se)
    # ... and on a row where all three components carry weight: equal weights, a point midway between the locations
    K, D = 3, 2
    mu = torch.tensor([[1., 0.], [-0.5, 0.8660254], [-0.5, -0.8660254]], device='cuda')
    pk = M.impute_pack_t(torch.log(torch.full((K,), 1 / 3., device='cuda')), mu, torch.eye(D, device='cuda').expand(K, D, D).contiguous(),
                         torch.tensor([3., 5., 9.], device='cuda'))
    pt = torch.tensor([[0.2, 0.1]], device='cuda')
    none = torch.zeros(1, D, dtype=torch.uint8, device='cuda')
    _, z = M.mixture_sample(pt, none, pk, 7, draws=draws, want_z=True)
    resp = M.mixture_impute(pt, none, pk, want_resp=True)[2][0].double().cpu().numpy()
    assert resp.min() > 0.1
    freq = np.bincount(z[:, 0].cpu().numpy(), minlength=3) / draws
    assert (np.abs(freq - resp) <= 5 * np.sqrt(resp * (1 - resp) / draws)).all(), (freq, resp)


def test_rows_without_mass_and_nan_parameters():
    M = _mix()
    x, miss, t, q, seed = _case(257, 8, 3)
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    c = _cuda(t)
    pack = M.impute_pack_t(torch.full_like(c['log_w'], -float('inf')), c['mu'], c['sigma'], c['nu'])
    out, z = M.mixture_sample(xd, md, pack, seed, draws=2, want_z=True)
    assert (z == -1).all() and not torch.isnan(out).any()
    assert _same(out, torch.where(md != 0, torch.zeros_like(xd), xd).expand(2, -1, -1))
    nu = c['nu'].clone()
    nu[1] = -1.0                                                    # a NaN pack row
    pack = M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], nu)
    out, z = M.mixture_sample(xd, md, pack, seed, draws=2, want_z=True)
    m = (md != 0).expand(2, -1, -1)
    assert torch.isnan(out[m]).all() and _same(out[~m], xd.expand(2, -1, -1)[~m]) and (z == -1).all()


def test_python_surface_agrees_with_the_pass():
    """VMPLoop.sample / impute_draws (a complete-data GMM loop, an SMM loop, a masked GMM loop after two iterations) and the gmm / smm /
    student_t wrappers: the bits of mixture_sample / mixture_draw on the pack they build"""
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import gmm, smm
    M = _mix()
    N, D, K = 257, 8, 3
    x, miss, t, q, seed = _case(N, D, K)
    xd, md = torch.as_tensor(x).cuda(), torch.as_tensor(miss).cuda()
    g = torch.Generator(device='cpu').manual_seed(5)
    r0 = torch.softmax(3 * torch.randn(N, K, generator=g), 1).cuda()
    kap = torch.full((K,), 5.0, device='cuda')
    for flav, kw in ((L.VMP_GMM, {}), (L.VMP_SMM, dict(kappa=kap)), (L.VMP_GMM, dict(miss=md))):
        loop = M.VMPLoop(xd, r0, flav, **kw)
        with pytest.raises(L.VmpError, match='at least one iteration'):
            loop.sample(4, seed)
        with pytest.raises(L.VmpError, match='at least one iteration'):
            loop.impute_draws(xd, md, 2, seed)
        loop.run(2)
        pack = loop.impute_pack()
        xs, zs = loop.sample(100, seed, want_z=True)
        ws, wz = M.mixture_draw(100, pack, seed, want_z=True)
        assert _same(xs, ws) and torch.equal(zs, wz) and _same(loop.sample(100, seed), ws)
        xi, zi = loop.impute_draws(xd, md, 3, seed, want_z=True)
        wi, wzi = M.mixture_sample(xd, md, pack, seed, draws=3, want_z=True)
        assert _same(xi, wi) and torch.equal(zi, wzi) and _same(loop.impute_draws(xd, md, 3, seed), wi)
        th = loop.theta()
        if flav == L.VMP_SMM:
            assert _same(smm.heldout_sample(100, seed, *th, kap), ws)
            assert _same(smm.heldout_impute_draws(xd, md, 3, seed, *th, kap), wi)
        else:
            assert _same(gmm.predictive_sample(100, seed, *th), ws)
            a, b = gmm.predictive_impute_draws(xd, md, 3, seed, *th, want_z=True)
            assert _same(a, wi) and torch.equal(b, wzi)
    c = _cuda(t)
    pack = M.impute_pack_t(c['log_w'], c['mu'], c['sigma'], c['nu'])
    ys, yz = student_t.mixture_sample(64, seed, c['mu'], c['sigma'], c['nu'], c['log_w'], want_z=True)
    ws, wz = M.mixture_draw(64, pack, seed, want_z=True)
    assert _same(ys, ws) and torch.equal(yz, wz)
