"""The N-sized forms of the SVAE E-step against the fp64 truth of tests/svae_estep_truth.py at GENERIC parameters: the in-kernel-noise
forward forms (fwd1 at every L, tile with and without the compiled-in S, pst, pst2) with their epilogue (sub-sample, r, moments,
CVI), the one-block-per-tile backward bwd1 at every L, and one shape per noise-tensor form with a generic Gaussian theta.  Every
case asserts the form it is there for through vmp_svae_launch_plan first, so a plan change cannot silently empty a case.

The truth is fed the device's own materialised stream (PhiloxNoise.materialise, tied to oracle.philox.cell_noise within 2e-5 by
tests/test_philox.py), so the generator's hardware log / sin / cos do not eat the 1e-5 budget of x.  Bars: the project's clauses
(svae_estep_truth.bars / grad_bar / moment_bar), none measured on the kernel."""
import ctypes

import numpy as np
import pytest
import torch

import parity_log
import svae_estep_truth as T

pytestmark = pytest.mark.gpu
RHO = 0.2


def _lib():
    from vmp_for_svae_amd import _lib as L
    return L


def _plan(direction, N, K, Ld, S, f0, f1, f2, f3):
    L = _lib()
    out = (ctypes.c_int64 * 8)()
    L.check(L.lib().vmp_svae_launch_plan(direction, N, K, Ld, S, f0, f1, f2, f3, out), 'vmp_svae_launch_plan')
    return list(out)


def _fwd_form(shape, rng, mom=0, fwd1_ok=1):
    return T.FWD_FORMS[_plan(0, *shape, int(rng), 1, int(mom), int(fwd1_ok))[0]]


def _bwd_form(shape, student=0, nblk=0):
    return T.BWD_FORMS[_plan(1, *shape, int(student), 1, int(nblk), 0)[0]]


def _f(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device='cuda', requires_grad=grad)


def _err(got, want, rel=True):
    got, want = got.detach().double().cpu(), want.double()
    e = float((got - want).abs().max())
    return e / max(float(want.abs().max()), 1e-300) if rel else e


def _check(tag, what, err, bar, ref=None):
    parity_log.record('rel' if what != 'r' else 'abs', err, bar, '%s %s' % (tag, what))
    print('FORMS|%s|%s|err=%.3e|bar=%.3e|oracle32=%s' % (tag, what, err, bar, 'n/a' if ref is None else '%.3e' % ref))
    assert err <= bar, (tag, what, err, bar, ref)


def _device_params(params, grad=True):
    phi32, th32 = params.as_torch(torch.float32)
    phi = [p.cuda().requires_grad_(grad) for p in phi32]
    th = [t.cuda() for t in th32]
    if params.student and grad:
        th[1].requires_grad_(True)
        th[2].requires_grad_(True)
    return phi, th


def _truths(params, e1, e2, noise64, wx):
    t64 = T.estep_truth(params, e1, e2, noise64, wx=wx)
    t32 = T.estep_truth(params, e1, e2, noise64, wx=wx, dtype=torch.float32)
    bar, ref = T.bars(t64, t32)
    return t64, t32, bar, ref


def _compare_forward(tag, x, lz, Tp, t64, bar, ref):
    _check(tag, 'x', _err(x, t64['x']), bar['x'], ref['x'])
    _check(tag, 'r', _err(torch.exp(lz.detach().double()), t64['r'], rel=False), bar['r'], ref['r'])
    _check(tag, "T'", _err(Tp, t64['Tp']), bar['Tp'], ref['Tp'])


def _compare_grads(tag, got, t64, t32, S):
    assert len(got) == len(t64['grads'])
    for g, w, w32, n_ in zip(got, t64['grads'], t32['grads'], T.GRAD_NAMES):
        bar, o32 = T.grad_bar(S, w, w32)
        _check(tag, 'grad ' + n_, _err(g, w), bar, o32)


RNG_SWEEP = [(f, s, False) for f, s in T.RNG_CASES] + [(f, s, True) for f, s in T.RNG_CASES_T]


def test_the_sweep_covers_what_it_claims():
    """every in-kernel-noise form, fwd1 and bwd1 at every L, both tile instances (S = 10 compiled in, S at run time), pst beyond and
    below 256 tiles, the moments in pst and pst2, and every noise-tensor / backward form - asked of the library, not restated"""
    L = _lib()
    seen_f, seen_b, fwd1_L = set(), set(), set()
    for form, shape, student in RNG_SWEEP:
        mom = L.lib().vmp_svae_fwd_mom_blocks(*shape) > 0
        assert _fwd_form(shape, True, mom) == form, (form, shape)
        assert L.lib().vmp_svae_rng_in_kernel(*shape[1:]) == 1
        seen_f.add((form, shape[3] == 10, mom))
        if form == 'fwd1' and not student:
            assert _bwd_form(shape) == 'bwd1' and _plan(1, *shape, 0, 1, 0, 0)[1] == L.lib().vmp_svae_bwd_blocks_for(*shape, 0)
            fwd1_L.add(shape[2])
    assert fwd1_L == set(range(1, 9))
    assert {f for f, _, _ in seen_f} == {'fwd1', 'tile', 'pst', 'pst2'}
    assert ('tile', True, False) in seen_f and ('tile', False, False) in seen_f and ('pst', False, True) in seen_f and ('pst2', True, True) in seen_f
    for shape in T.MOM_SHAPES:
        assert L.lib().vmp_svae_fwd_mom_blocks(*shape) > 0 and (('pst', shape) in T.RNG_CASES or ('pst2', shape) in T.RNG_CASES)
    assert _fwd_form(T.AT_CASE[1], True, fwd1_ok=0) == T.AT_CASE[0] and _fwd_form(T.AT_CASE[1], True) == 'fwd1'
    for ff, bf, shape, which in T.TENSOR_CASES:
        nblk = 0 if which == 'for' else L.lib().vmp_svae_bwd_blocks(shape[0], shape[1])
        assert _fwd_form(shape, False) == ff and _bwd_form(shape, nblk=nblk) == bf, (shape, _fwd_form(shape, False), _bwd_form(shape, nblk=nblk))
        seen_b.add(bf)
        seen_f.add((ff, None, None))
    assert seen_b == {'bwd1', 'ring', 'generic_one', 'generic_stream'}
    assert {f for f, _, _ in seen_f} == set(T.FWD_FORMS) - {'none'}


@pytest.mark.parametrize('form,shape,student', RNG_SWEEP, ids=['%s-%s-%s' % (f, 'x'.join(map(str, s)), 't' if st else 'g') for f, s, st in RNG_SWEEP])
def test_in_kernel_noise_forms_vs_fp64_truth(form, shape, student):
    """svae.e_step(noise='philox') - forward with epilogue, autograd backward (bwd1 on the fwd1 shapes with a Gaussian theta: the
    N-sized gradients directly, the K-sized sums through vmp_svae_bwd_reduce and the phi-prep backward) - against the truth."""
    from vmp_for_svae_amd.models import svae, _svae_ops
    L = _lib()
    N, K, Ld, S = shape
    nb = L.lib().vmp_svae_fwd_mom_blocks(N, K, Ld, S)
    assert _fwd_form(shape, True, nb > 0) == form
    if form == 'fwd1' and not student:
        assert _bwd_form(shape) == 'bwd1'
    tag = '%s%s %s' % (form, ' student-t' if student else '', shape)
    params, e1, e2, wx, seed = T.sweep_case(shape, student)
    noise64 = _svae_ops.PhiloxNoise(seed, S).materialise(N, K, Ld, 'cuda').double().cpu().numpy()
    t64, t32, bar, ref = _truths(params, e1, e2, noise64, wx)
    phi, th = _device_params(params)
    pe1, pe2 = _f(e1, True), _f(e2, True)
    x, lz, pt, _ = svae.e_step((pe1, pe2), phi, S, seed=seed, noise='philox', theta=th)
    loss = (x * _f(wx)).sum() + (torch.exp(lz) * (pt.T_prime + lz)).sum()
    got = torch.autograd.grad(loss, [pe1, pe2] + phi + ([th[1], th[2]] if student else []))
    _compare_forward(tag, x, lz, pt.T_prime, t64, bar, ref)
    _compare_grads(tag, got, t64, t32, S)
    # ---- the epilogue of the same launch
    assert pt.x_samples is not None and pt.r_nk is not None and (pt.mom is not None) == (nb > 0)
    _check(tag, 'r', _err(pt.r_nk, t64['r'], rel=False), bar['r'], ref['r'])
    z, near = T.picks(t64['r'], seed, margin=1e-5)
    keep = ~near if N > 2000 else torch.ones(N, dtype=torch.bool)
    assert float((~keep).double().mean()) <= 0.005
    n = torch.arange(N)
    want_xs = x.detach().cpu()[n, z, 0, :]
    assert torch.equal(pt.x_samples.cpu()[keep], want_xs[keep]), (tag, int((pt.x_samples.cpu() != want_xs).any(1)[keep].sum()))
    if shape not in T.MOM_SHAPES or student:
        return
    assert nb > 0
    z32 = T.picks(t32['r'], seed)
    assert torch.equal(z, z32)
    stats, _ = _svae_ops.mom_cvi(pt.mom)
    x_s64 = t64['x'][n, z, 0, :]
    mom64, _ = T.raw_moments(x_s64, t64['r'])
    mbar, mloss = T.moment_bar(t64, t32, z)
    ratio = float(((stats.cpu() - mom64).abs() / mbar.clamp_min(1e-300)).max())
    _check(tag, 'moments / bar', ratio, 1.0, float((mloss / mbar.clamp_min(1e-300)).max()))
    prior = svae.init_mm(K, Ld, seed=0, param_device='cuda')[0]
    th_dev = [t.clone() for t in th]
    _, star = _svae_ops.mom_cvi(pt.mom, prior, th_dev, RHO)
    th32 = params.as_torch(torch.float32)[1]
    star64, new64 = T.cvi_truth([p.double().cpu() for p in prior], [t.double() for t in th32], x_s64, t64['r'], RHO)
    star32, new32 = T.cvi_truth([p.cpu() for p in prior], th32, t32['x'][n, z, 0, :], t32['r'], RHO)
    for n_, g_s, g_n, s64, s32, n64, n32 in zip(('alpha', 'A', 'b', 'beta', 'v_hat'), star, th_dev, star64, star32, new64, new32):
        for what, g, w64, w32 in (('theta* ', g_s, s64, s32), ('theta after CVI ', g_n, n64, n32)):
            o32 = _err(w32, w64)
            _check(tag, what + n_, _err(g, w64), max(1e-5, 3 * o32), o32)


def test_row_offset_form_vs_fp64_truth():
    """vmp_svae_estep_fwd_rng_at with row0 = 1000: the streaming kernel on the noise of cells (row0 + n) K + k"""
    from vmp_for_svae_amd.models import svae, _svae_ops
    form, shape, row0 = T.AT_CASE
    N, K, Ld, S = shape
    assert _fwd_form(shape, True, fwd1_ok=0) == form
    params, e1, e2, wx, seed = T.sweep_case(shape)
    noise64 = _svae_ops.PhiloxNoise(seed, S, row0=row0).materialise(N, K, Ld, 'cuda').double().cpu().numpy()
    whole = _svae_ops.PhiloxNoise(seed, S).materialise(row0 + N, K, Ld, 'cuda')[row0:].double().cpu().numpy()
    assert np.array_equal(noise64, whole)
    from oracle import philox
    cells = (row0 + np.arange(N))[:, None] * K + np.arange(K)[None, :]
    assert np.abs(noise64 - philox.cell_noise(seed, cells.reshape(-1), Ld, S).reshape(N, K, Ld, S)).max() < 2e-5
    t64 = T.estep_truth(params, e1, e2, noise64)
    t32 = T.estep_truth(params, e1, e2, noise64, dtype=torch.float32)
    bar, ref = T.bars(t64, t32)
    phi, th = _device_params(params, grad=False)
    with torch.no_grad():
        x, lz, pt, _ = svae.e_step((_f(e1), _f(e2)), phi, S, noise=_svae_ops.PhiloxNoise(seed, S, row0=row0), theta=th)
    _compare_forward('%s _at row0=%d %s' % (form, row0, shape), x, lz, pt.T_prime, t64, bar, ref)


@pytest.mark.parametrize('ff,bf,shape,which', T.TENSOR_CASES, ids=['%s-%s-%s' % (a, b, 'x'.join(map(str, s))) for a, b, s, _ in T.TENSOR_CASES])
def test_noise_tensor_forms_with_generic_theta_vs_fp64_truth(ff, bf, shape, which):
    """One shape per noise-tensor forward form and per backward form with a generic Gaussian theta (the theta term of T' - m_k, W_k,
    kappa_k - is isotropic in test_estep_vs_oracle_shapes).  'for': the autograd path (nblk = vmp_svae_bwd_blocks_for); 'blocks':
    vmp_svae_estep_bwd's geometry (nblk = vmp_svae_bwd_blocks), launched here, its sums through vmp_svae_bwd_reduce and the phi-prep
    backward as the autograd path takes them."""
    from vmp_for_svae_amd.models import svae
    L = _lib()
    N, K, Ld, S = shape
    nblk = L.lib().vmp_svae_bwd_blocks_for(N, K, Ld, S, 0) if which == 'for' else L.lib().vmp_svae_bwd_blocks(N, K)
    assert _fwd_form(shape, False) == ff and _bwd_form(shape, nblk=0 if which == 'for' else nblk) == bf
    tag = '%s/%s tensor %s' % (ff, bf, shape)
    params, e1, e2, wx, seed = T.sweep_case(shape)
    noise = np.random.Generator(np.random.PCG64(seed + 1)).standard_normal((N, K, Ld, S)).astype(np.float32)
    t64, t32, bar, ref = _truths(params, e1, e2, noise.astype(np.float64), wx)
    phi, th = _device_params(params)
    pe1, pe2 = _f(e1, True), _f(e2, True)
    prep = svae.recognition_prep(phi, th)
    x, lz, pt, _ = svae.e_step((pe1, pe2), phi, S, noise=_f(noise), theta=th, prep=prep)
    _compare_forward(tag, x, lz, pt.T_prime, t64, bar, ref)
    if which == 'for':
        loss = (x * _f(wx)).sum() + (torch.exp(lz) * (pt.T_prime + lz)).sum()
        got = torch.autograd.grad(loss, [pe1, pe2] + phi)
    else:
        f32 = dict(dtype=torch.float32, device='cuda')
        with torch.no_grad():
            r = torch.exp(lz)
            Gx, Glz, GT = _f(wx).contiguous(), (r * (pt.T_prime + lz + 1.0)).contiguous(), r.contiguous()
            hk, P, bias, mk, Wk = [t.detach().contiguous() for t in prep[:5]]
            PW = L.lib().vmp_svae_bwd_partial_words(Ld)
            g1, g2, part = torch.empty(N, Ld, **f32), torch.empty(N, Ld, **f32), torch.empty(nblk, K, PW, **f32)
            xd, lzd = x.detach().contiguous(), lz.detach().contiguous()
            L.check(L.lib().vmp_svae_estep_bwd_n(L.ptr(pe1.detach()), L.ptr(pe2.detach()), L.ptr(hk), L.ptr(P), L.ptr(bias), L.ptr(mk), L.ptr(Wk), None,
                                                 L.ptr(xd), L.ptr(lzd), L.ptr(Gx), L.ptr(Glz), L.ptr(GT), N, K, Ld, S, L.ptr(g1), L.ptr(g2),
                                                 L.ptr(part), part.numel() * 4, nblk, L.stream()), 'vmp_svae_estep_bwd_n')
            g_hk, g_P, g_bias = torch.empty(K, Ld, **f32), torch.empty(K, Ld, Ld, **f32), torch.empty(K, **f32)
            L.check(L.lib().vmp_svae_bwd_reduce(L.ptr(part), nblk, K, Ld, L.ptr(g_hk), L.ptr(g_P), L.ptr(g_bias), None, None, None,
                                                L.stream()), 'vmp_svae_bwd_reduce')
        got = [g1, g2] + list(torch.autograd.grad(list(prep[:3]), phi, [g_hk, g_P, g_bias]))
    _compare_grads(tag, got, t64, t32, S)
