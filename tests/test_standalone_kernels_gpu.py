"""Shape sweeps of the stand-alone density and metric kernels (csrc/vmp_density.hip, csrc/vmp_loglike.hip) against the fp64 oracle:
every D instantiation of VMP_SWITCH_DIM, K in {1, 5, 32, 33, 64} (64 / 12 / 2 / 1 / 1 rows per wave), both Bernoulli forms, the
float4 and the scalar reconstruction paths, every lanes-per-cell mapping of the loglike / eval kernels, and one case above every
launcher's grid cap (guarded, NaN-prefilled outputs; called twice: bit-identical).

References: oracle/dists.py, oracle/metrics.py, oracle/nets.py, oracle/mixtures.gmm_expct_mahalanobis in fp64, gradients from their fp64
autograd under a random upstream gradient.  Where the oracle has no per-cell output (A_nk, the cell metrics, the Bernoulli rows) or
tiles an operand (the grid-cap sizes), the reference is the closed form written here, and the same test checks it against the oracle
to 1e-12 after the oracle's contractions / at a small shape.

Bars (max |got - want| / max |want|): forward values 1e-5, the two per-sample densities 2e-5, every gradient 5e-5 - or 3x the error
of the same reference evaluated in fp32 on the same inputs where that is larger (measured from the reference, never from the kernel;
both figures go to the parity log).  Every output must be finite wherever the reference is."""
import math

import numpy as np
import pytest
import torch

import parity_log

pytestmark = pytest.mark.gpu
FWD, PER_SAMP, GRAD = 1e-5, 2e-5, 5e-5
LOG2PI = math.log(2.0 * math.pi)
GUARD, SENT = 64, 12345.0


# ------------------------------------------------------------------------------------------------------------------ helpers
def rng_for(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def dev(a, dtype=torch.float32, grad=False):
    t = torch.as_tensor(np.asarray(a)).to('cuda', dtype).contiguous()
    return t.requires_grad_(True) if grad else t


def cpu(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def npy(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def relerr(got, want):
    """max |got - want| / max |want| over the entries where the reference is finite; there `got` must be finite, and elsewhere it
    must be the reference's own infinity"""
    got, want = npy(got), npy(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all(), 'non-finite output where the reference is finite'
    assert np.array_equal(got[~fin], want[~fin]), 'output differs from the reference infinity'
    if not fin.any():
        return 0.0
    return float(np.abs(got[fin] - want[fin]).max() / max(np.abs(want[fin]).max(), 1e-300))


def check(what, got, want, base, ref32=None, tag=None):
    """assert the bar: base, or 3x the fp32 reference's own error (the floor) where that is larger; both go to the parity log"""
    floor = relerr(ref32, want) if ref32 is not None else 0.0
    tol = max(base, 3.0 * floor)
    e = relerr(got, want)
    if ref32 is not None:
        parity_log.record('rel', floor, None, what + ' [reference in fp32]')
    parity_log.record('rel', e, tol, what)
    print('%-44s %-28s err %.3e  fp32-reference %.3e  bar %.1e' % (what, tag, e, floor, tol))
    assert e <= tol, (what, tag, e, tol)
    return e


def agree(a, b, what, tol=1e-12):
    """closed form vs oracle, both fp64"""
    a, b = npy(a), npy(b)
    e = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert e <= tol, ('closed form vs oracle: ' + what, e)


def L_():
    import vmp_for_svae_amd as V
    return V._lib


class Guarded(object):
    """an output buffer pre-filled with NaN and followed by 64 guard floats"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.full = torch.empty(self.n + GUARD, dtype=torch.float32, device='cuda')
        self.t = self.full[:self.n].view(*shape)
        self.reset()

    def reset(self):
        self.full[:self.n] = float('nan')
        self.full[self.n:] = SENT

    def verify(self):
        assert not torch.isnan(self.t).any().item(), 'an output element was never written'
        assert (self.full[self.n:] == SENT).all().item(), 'write past the end of the output'


def run_twice(name, args, outs):
    """the raw C entry, twice into the same NaN-prefilled guarded buffers: complete, in bounds, bit-identical"""
    L = L_()
    first = None
    for it in range(2):
        for o in outs:
            o.reset()
        L.check(getattr(L.lib(), name)(*args), name)
        torch.cuda.synchronize()
        for o in outs:
            o.verify()
        if first is None:
            first = [o.t.clone() for o in outs]
    for a, o in zip(first, outs):
        assert torch.equal(a.view(torch.int32), o.t.view(torch.int32)), name + ': two calls differ'


# ------------------------------------------------------------------------------------------------------- Gaussian / Student-t
KS = (1, 5, 32, 33, 64)
DK = [(8, k) for k in KS] + [(1, k) for k in KS] + [(2, 5), (3, 32), (4, 33), (5, 64), (6, 1), (7, 33), (3, 64), (4, 1), (7, 5), (6, 64)]
DK_IDS = ['D%d-K%d' % dk for dk in DK]
N_SWEEP, S_SWEEP = 37, 3            # 37 rows: a partial last wave tile at every K above


def eta2_of(A):
    eye = torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
    return -0.5 * (A @ A.transpose(-1, -2) + 0.5 * eye)


def sigma_of(B):
    eye = torch.eye(B.shape[-1], dtype=B.dtype, device=B.device)
    return B @ B.transpose(-1, -2) + 0.5 * eye


def three_ways(arrays, g, fn_oracle, fn_kernel, n_leaves):
    """(value, leaf gradients) of the oracle in fp64, the oracle in fp32 and the kernel; `arrays` are fp32-exact inputs, the first
    n_leaves of them differentiated"""
    out = []
    for kind in ('f64', 'f32', 'gpu'):
        if kind == 'gpu':
            ts = [dev(a, grad=i < n_leaves) for i, a in enumerate(arrays)]
            val = fn_kernel(*ts)
            gg = dev(g)
        else:
            dt = torch.float64 if kind == 'f64' else torch.float32
            ts = [cpu(a, dt, grad=i < n_leaves) for i, a in enumerate(arrays)]
            val = fn_oracle(*ts)
            gg = cpu(g, dt)
        grads = torch.autograd.grad((val * gg).sum(), ts[:n_leaves]) if n_leaves else ()
        out.append((val.detach(), grads))
    return out


@pytest.mark.parametrize('D,K', DK, ids=DK_IDS)
def test_gauss_nat_normalised_template_sweep(D, K):
    """gaussian.log_probability_nat with and without weights: gauss_nat_kernel<D>, normalised form - the in-wave log-sum-exp over
    scr[wave][rbase + j] at RPT = 64 / K rows per wave"""
    from oracle import dists
    from vmp_for_svae_amd.distributions import gaussian
    N = N_SWEEP
    r = rng_for(101, D, K)
    x, e1, A = f32(r.standard_normal((N, D))), f32(r.standard_normal((N, K, D))), f32(0.3 * r.standard_normal((N, K, D, D)))
    lw = r.standard_normal(K)
    w = f32(np.exp(lw - np.logaddexp.reduce(lw)))
    for weights in (None, w):
        o64, o32, got = three_ways(
            [x, e1, A] + ([weights] if weights is not None else []), np.zeros((N, K), np.float32),
            lambda x_, e_, A_, w_=None: dists.gauss_log_probability_nat(x_, e_, eta2_of(A_), w_),
            lambda x_, e_, A_, w_=None: gaussian.log_probability_nat(x_, e_, eta2_of(A_), w_), 0)
        check('gauss nat normalised' + (' +weights' if weights is not None else ''), got[0], o64[0], FWD, o32[0], (N, K, D))


@pytest.mark.parametrize('D,K', DK, ids=DK_IDS)
def test_gauss_per_samp_and_adjoint_template_sweep(D, K):
    """gaussian.log_probability_nat_per_samp and its adjoint: gauss_nat_kernel<D> (per-sample form), gauss_nat_bwd_kernel<D>"""
    from oracle import dists
    from vmp_for_svae_amd.distributions import gaussian
    N, S = N_SWEEP, S_SWEEP
    r = rng_for(102, D, K)
    x, e1, A = f32(r.standard_normal((N, K, S, D))), f32(r.standard_normal((N, K, D))), f32(0.3 * r.standard_normal((N, K, D, D)))
    g = f32(r.standard_normal((N, K, S)))
    o64, o32, got = three_ways([x, e1, A], g,
                               lambda x_, e_, A_: dists.gauss_log_probability_nat_per_samp(x_, e_, eta2_of(A_)),
                               lambda x_, e_, A_: gaussian.log_probability_nat_per_samp(x_, e_, eta2_of(A_)), 3)
    check('gauss per-samp value', got[0], o64[0], PER_SAMP, o32[0], (N, K, S, D))
    for n_, a_, b_, c_ in zip(('x', 'eta1', 'A(eta2)'), got[1], o64[1], o32[1]):
        check('gauss per-samp grad ' + n_, a_, b_, GRAD, c_, (N, K, S, D))


@pytest.mark.parametrize('D,K', DK, ids=DK_IDS)
def test_student_t_and_adjoint_template_sweep(D, K):
    """student_t.log_probability_per_samp and its adjoint: student_t_kernel<D>, student_t_bwd_kernel<D> (one partial block)"""
    from oracle import dists
    from vmp_for_svae_amd.distributions import student_t
    N, S = N_SWEEP, S_SWEEP
    r = rng_for(103, D, K)
    y, mu, B = f32(r.standard_normal((N, K, S, D))), f32(2 * r.standard_normal((K, D))), f32(0.4 * r.standard_normal((K, D, D)))
    v = f32(3.0 + 4.0 * r.random(K))
    g = f32(r.standard_normal((N, K, S)))
    o64, o32, got = three_ways([y, mu, B, v], g,
                               lambda y_, m_, B_, v_: dists.student_t_log_probability_per_samp(y_, m_, sigma_of(B_), v_),
                               lambda y_, m_, B_, v_: student_t.log_probability_per_samp(y_, m_, sigma_of(B_), v_), 3)
    check('student-t value', got[0], o64[0], PER_SAMP, o32[0], (N, K, S, D))
    for n_, a_, b_, c_ in zip(('y', 'mu', 'B(sigma)'), got[1], o64[1], o32[1]):
        check('student-t grad ' + n_, a_, b_, GRAD, c_, (N, K, S, D))


# ------------------------------------------------------------------------------------------------------------- Mahalanobis
@pytest.mark.parametrize('N,D,K', [(1, 1, 1), (257, 3, 5), (100, 8, 64), (513, 7, 33)])
@pytest.mark.parametrize('masking', ['nomask', 'mask30', 'hidden_row'])
def test_mahalanobis_shapes(N, D, K, masking):
    """gmm.compute_expct_mahalanobis_dist / compute_dev_missing_data (maha_kernel); a row whose entries are all missing is D / beta_k"""
    from oracle import mixtures
    from vmp_for_svae_amd.models import gmm
    r = rng_for(104, N, D, K)
    x, m = f32(2 * r.standard_normal((N, D))), f32(2 * r.standard_normal((K, D)))
    B = 0.4 * r.standard_normal((K, D, D))
    P = f32(B @ B.transpose(0, 2, 1) + 0.5 * np.eye(D))
    v, beta = f32(3.0 + 4.0 * r.random(K)), f32(0.5 + 2.0 * r.random(K))
    mask = None
    if masking != 'nomask':
        mask = r.random((N, D)) < 0.3
        if masking == 'hidden_row':
            mask[N // 2] = True
    want, ref32 = [mixtures.gmm_expct_mahalanobis(cpu(x, dt), cpu(beta, dt), cpu(m, dt), cpu(P, dt), cpu(v, dt),
                                                  None if mask is None else torch.as_tensor(mask)) for dt in (torch.float64, torch.float32)]
    dx, db, dm, dP, dv = dev(x), dev(beta), dev(m), dev(P), dev(v)
    if mask is None:
        got = gmm.compute_expct_mahalanobis_dist(dx, db, dm, dP, dv)
    else:
        got = gmm.compute_dev_missing_data(dx, db, dm, dP, dv, dev(mask, torch.bool))
    check('mahalanobis ' + masking, got, want, FWD, ref32, (N, D, K))
    if masking == 'hidden_row':
        # v_k * 0 + D / beta_k: one fp32 division (at most 2.5 ulp where it is not correctly rounded)
        row, exact = got[N // 2].double().cpu().numpy(), D / beta.astype(np.float64)
        assert np.all(np.abs(row - exact) <= 3 * 2.0 ** -24 * exact), (row, exact)


# --------------------------------------------------------------------------------- diagonal-Gaussian reconstruction term (A_nk)
S_LIST = (1, 7, 10, 33, 64, 65, 100)         # lanes per cell 1, 7, 10, 33, 64, 64 (+1 wrapped sample), 64; cells per wave 64, 9, 6, 1, 1, 1, 1


def diag_A(y, mean, var, eps):
    """A_nk = sum_{s,d} (y_nd - mean_nksd)^2 / var_nksd + log(var_nksd + eps)   (the kernel's header comment; vae.py:225,240)"""
    return ((y[:, None, None, :] - mean) ** 2 / var + torch.log(var + eps)).sum((2, 3))


def diag_inputs(N, K, S, Dy, *key):
    r = rng_for(105, N, K, S, Dy, *key)
    return (f32(r.standard_normal((N, Dy))), f32(r.standard_normal((N, K, S, Dy))), f32(0.05 + 1.5 * r.random((N, K, S, Dy))),
            f32(r.standard_normal((N, K))), r)


def diag_A_vs_oracle(y, mean, var, r):
    """the closed form against nets.expected_diagonal_gaussian_loglike, both of its branches, after the n,k-contraction"""
    from oracle import nets
    N, K, S, Dy = mean.shape
    y64, m64, v64 = cpu(y, torch.float64), cpu(mean, torch.float64), cpu(var, torch.float64)
    w = cpu(r.random((N, K)), torch.float64)
    agree(-0.5 * ((diag_A(y64, m64, v64, 1e-8) * w).sum() / S) - N * Dy / 2. * LOG2PI,
          nets.expected_diagonal_gaussian_loglike(y64, m64, v64, w), 'A_nk, weights branch')
    yy = y64[:, None, :].expand(N, K, Dy).reshape(N * K, Dy)
    agree(-0.5 * (diag_A(y64, m64, v64, 0.0).sum() / S) - N * K * Dy / 2. * LOG2PI,
          nets.expected_diagonal_gaussian_loglike(yy, m64.reshape(N * K, S, Dy), v64.reshape(N * K, S, Dy)), 'A_nk, plain branch')


@pytest.mark.parametrize('Dy', [1, 3, 4, 6, 8, 12])
@pytest.mark.parametrize('S', S_LIST)
def test_diag_gauss_loglike_shapes(S, Dy):
    """DiagGaussLoglikeFn forward and both gradients, eps in {1e-8, 0}: loglike_kernel<false/true>; Dy in {4, 8, 12} take the float4
    path (torch's allocations are 16-byte aligned), the others the scalar one"""
    from vmp_for_svae_amd.models import _svae_ops
    K = 1 if (S_LIST.index(S) + Dy) % 2 else 3
    N = 150 // K + 1                                  # 151 / 153 cells: not a multiple of any cells-per-wave above but 1
    y, mean, var, gA, r = diag_inputs(N, K, S, Dy)
    diag_A_vs_oracle(y, mean, var, r)
    for eps in (1e-8, 0.0):
        o64, o32, got = three_ways([mean, var, y], gA, lambda m_, v_, y_: diag_A(y_, m_, v_, eps),
                                   lambda m_, v_, y_: _svae_ops.DiagGaussLoglikeFn.apply(y_, m_, v_, eps), 2)
        tag = (N, K, S, Dy, eps)
        check('diag-gauss A', got[0], o64[0], FWD, o32[0], tag)
        check('diag-gauss grad mean', got[1][0], o64[1][0], GRAD, o32[1][0], tag)
        check('diag-gauss grad var', got[1][1], o64[1][1], GRAD, o32[1][1], tag)


def offset_by_one_float(t):
    """a copy of t whose first element sits 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device='cuda')
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize('S', [10, 100])
def test_diag_gauss_loglike_misaligned_pointers_take_the_scalar_path(S):
    """Dy = 8 through the raw C entry with mean, var and the two gradient buffers one float off a 16-byte boundary: the scalar
    fallback at Dy % 4 == 0.  Same element order as the float4 path: value and gradients are bit-identical to the aligned call's
    (and the value meets the bar against the oracle in both)."""
    L = L_()
    N, K, Dy = 51, 3, 8
    y, mean, var, gA, r = diag_inputs(N, K, S, Dy, 7)
    want = diag_A(cpu(y, torch.float64), cpu(mean, torch.float64), cpu(var, torch.float64), 1e-8)
    dy, dm, dv, dg = dev(y), dev(mean), dev(var), dev(gA)
    res = {}
    for form in ('aligned', 'offset'):
        m_, v_ = (dm, dv) if form == 'aligned' else (offset_by_one_float(dm), offset_by_one_float(dv))
        gm, gv = torch.full_like(dm, float('nan')), torch.full_like(dv, float('nan'))
        if form == 'offset':
            gm, gv = offset_by_one_float(gm), offset_by_one_float(gv)
        assert (m_.data_ptr() % 16 == 0) == (form == 'aligned') and (gm.data_ptr() % 16 == 0) == (form == 'aligned')
        A = torch.full((N, K), float('nan'), device='cuda')
        L.check(L.lib().vmp_diag_gauss_loglike_fwd(L.ptr(dy), L.ptr(m_), L.ptr(v_), N, K, S, Dy, 1e-8, L.ptr(A), L.stream()), 'fwd')
        L.check(L.lib().vmp_diag_gauss_loglike_bwd(L.ptr(dy), L.ptr(m_), L.ptr(v_), L.ptr(dg), N, K, S, Dy, 1e-8, L.ptr(gm), L.ptr(gv),
                                                   L.stream()), 'bwd')
        torch.cuda.synchronize()
        res[form] = (A, gm.clone(), gv.clone())
        check('diag-gauss A raw ' + form, A, want, FWD, None, (N, K, S, Dy))
    assert torch.equal(res['aligned'][1], res['offset'][1]) and torch.equal(res['aligned'][2], res['offset'][2])
    assert torch.equal(res['aligned'][0], res['offset'][0])              # the sum within a row runs in the same order


# ------------------------------------------------------------------------------------------------------- evaluation cell metrics
def cell_ref(y, mean, var, lw, mask, mask_mse, dt=np.float64):
    """the closed form of the kernel's header comment (losses.py:9-38, 83-145), per cell:
         mse_nk = mean_s sum_d m'_nd (y - mean)^2,   lse_nk = log 1/S sum_s exp(lw_nk(s) - 1/2 sum_d m_nd [(y - mean)^2 / var + log var + log 2pi])"""
    y, mean = y.astype(dt), mean.astype(dt)
    S = mean.shape[2]
    df2 = (y[:, None, None, :] - mean) ** 2
    m = dt(1) if mask is None else mask[:, None, None, :].astype(dt)
    mse = ((m if mask_mse else dt(1)) * df2).sum(3).mean(2)
    if var is None:
        return mse, None
    var = var.astype(dt)
    lp = (dt(-0.5) * m * (df2 / var + np.log(var) + dt(LOG2PI))).sum(3)
    if lw is not None:
        lw = lw.astype(dt)
        lp = lp + (lw[:, :, None] if lw.ndim == 2 else lw)
    with np.errstate(invalid='ignore'):
        lse = np.logaddexp.reduce(lp, axis=2) - dt(math.log(S))
    return mse, lse


def cell_ref_vs_oracle(y, mean, var, lw_nk, lw_nks, mask):
    from oracle import metrics
    T = lambda a: cpu(a, torch.float64)
    N = y.shape[0]
    rr = np.exp(lw_nk.astype(np.float64))
    mse, lse = cell_ref(y, mean, var, None, None, False)
    agree((mse * rr).sum(1).mean(), metrics.weighted_mse(T(y), T(mean), T(rr)), 'weighted_mse')
    agree(np.logaddexp.reduce(lse, axis=1).mean(), metrics.diagonal_gaussian_logprob(T(y), T(mean), T(var), T(np.zeros_like(lw_nk))), 'loli, no weights')
    for lw, m_ in ((lw_nk, None), (lw_nks, None), (lw_nk, mask), (lw_nks, mask)):
        _, lse = cell_ref(y, mean, var, lw, m_, False)
        agree(np.logaddexp.reduce(lse, axis=1).mean(),
              metrics.diagonal_gaussian_logprob(T(y), T(mean), T(var), T(lw), None if m_ is None else torch.as_tensor(m_)), 'loli')
    mse_m, _ = cell_ref(y, mean, None, None, mask, True)
    agree((mse_m * rr).sum() / N, metrics.imputation_mse(T(y), T(mean), T(rr), torch.as_tensor(mask)), 'imputation_mse')


def log_softmax(a, axis):
    return a - np.logaddexp.reduce(a, axis=axis, keepdims=True)


def cell_inputs(N, K, S, Dy, *key):
    r = rng_for(106, N, K, S, Dy, *key)
    y, mean, var = f32(r.standard_normal((N, Dy))), f32(r.standard_normal((N, K, S, Dy))), f32(0.05 + 1.5 * r.random((N, K, S, Dy)))
    lw_nk = f32(log_softmax(r.standard_normal((N, K)), 1))
    lw_nks = f32(log_softmax(r.standard_normal((N, K, S)), 1))
    mask = r.random((N, Dy)) < 0.3
    return y, mean, var, lw_nk, lw_nks, mask


def run_cells(y, mean, var, lw, mask, want_mse, want_lse, mask_mse):
    from vmp_for_svae_amd import losses
    return losses._cell_metrics(dev(y), dev(mean), None if var is None else dev(var), None if lw is None else dev(lw),
                                None if mask is None else dev(mask, torch.bool), want_mse, want_lse, mask_mse)


@pytest.mark.parametrize('Dy', [1, 5, 8])
@pytest.mark.parametrize('S', S_LIST)
def test_eval_cell_metrics_shapes(S, Dy):
    """losses._cell_metrics (vmp_eval_cell_metrics / eval_kernel): the (N,K) cell arrays for weights none / (N,K) / (N,K,S) x mask
    none / 30 % / 30 % with mask_mse, and the mse-only and lse-only calls"""
    K = 3 if (S_LIST.index(S) + Dy) % 2 else 1
    N = 150 // K + 1
    y, mean, var, lw_nk, lw_nks, mask = cell_inputs(N, K, S, Dy)
    cell_ref_vs_oracle(y, mean, var, lw_nk, lw_nks, mask)
    for wname, lw in (('none', None), ('nk', lw_nk), ('nks', lw_nks)):
        for mname, m_, mm in (('nomask', None, False), ('mask30', mask, False), ('mask30+mask_mse', mask, True)):
            tag = (N, K, S, Dy, wname, mname)
            want = cell_ref(y, mean, var, lw, m_, mm)
            r32 = cell_ref(y, mean, var, lw, m_, mm, np.float32)
            mse, lse = run_cells(y, mean, var, lw, m_, True, True, mm)
            check('cell mse', mse, want[0], FWD, r32[0], tag)
            check('cell lse', lse, want[1], FWD, r32[1], tag)
    want = cell_ref(y, mean, var, lw_nks, mask, True)
    mse, none = run_cells(y, mean, None, None, mask, True, False, True)                 # mse only: no var
    assert none is None
    check('cell mse (mse-only call)', mse, want[0], FWD, None, (N, K, S, Dy))
    none, lse = run_cells(y, mean, var, lw_nks, mask, False, True, True)                # lse only
    assert none is None
    check('cell lse (lse-only call)', lse, want[1], FWD, None, (N, K, S, Dy))


@pytest.mark.parametrize('S', [10, 64, 100])
def test_eval_cell_metrics_minus_inf_component_weight(S):
    """an (N,K) log-weight of -inf for a whole component: -inf in that component's cells, a finite metric"""
    from vmp_for_svae_amd import losses
    N, K, Dy = 51, 3, 5
    y, mean, var, lw_nk, _, mask = cell_inputs(N, K, S, Dy, 1)
    lw_nk = lw_nk.copy()
    lw_nk[:, 1] = -np.inf
    want = cell_ref(y, mean, var, lw_nk, None, False)
    assert np.isneginf(want[1][:, 1]).all() and np.isfinite(want[1][:, [0, 2]]).all()
    mse, lse = run_cells(y, mean, var, lw_nk, None, True, True, False)
    check('cell lse, -inf component', lse, want[1], FWD, cell_ref(y, mean, var, lw_nk, None, False, np.float32)[1], (N, K, S, Dy))
    assert torch.isneginf(lse[:, 1]).all().item()
    check('cell mse, -inf component', mse, want[0], FWD, None, (N, K, S, Dy))
    got = losses.diagonal_gaussian_logprob(dev(y), dev(mean), dev(var), dev(lw_nk))
    assert torch.isfinite(got).item()
    check('loli, -inf component', got, np.logaddexp.reduce(want[1], axis=1).mean(), FWD, None, (N, K, S, Dy))


@pytest.mark.parametrize('pattern', ['first64_of_odd_rows', 'last36_of_every_4th_row', 'alternating_samples'])
def test_eval_cell_metrics_minus_inf_per_sample_weights_s100(pattern):
    """S = 100 (a lane walks samples s and s + 64), per-sample log-weights of -inf: on samples 0..63 of every second row a lane's
    first term is -inf and its second finite - the online log-sum-exp must not turn exp(-inf - -inf) into NaN.  The oracle
    (metrics.diagonal_gaussian_logprob, fp64) is finite for these inputs."""
    from oracle import metrics
    from vmp_for_svae_amd import losses
    N, K, S, Dy = 51, 3, 100, 5
    y, mean, var, _, lw, mask = cell_inputs(N, K, S, Dy, 2)
    lw = lw.copy()
    if pattern == 'first64_of_odd_rows':
        lw[1::2, :, :64] = -np.inf
    elif pattern == 'last36_of_every_4th_row':
        lw[::4, :, 64:] = -np.inf
    else:
        lw[:, :, ::2] = -np.inf
    T = lambda a: cpu(a, torch.float64)
    oracle = metrics.diagonal_gaussian_logprob(T(y), T(mean), T(var), T(lw))
    assert torch.isfinite(oracle).item()
    want = cell_ref(y, mean, var, lw, None, False)
    assert np.isfinite(want[1]).all()
    agree(np.logaddexp.reduce(want[1], axis=1).mean(), oracle, 'loli with -inf per-sample weights')
    mse, lse = run_cells(y, mean, var, lw, None, True, True, False)
    check('cell lse, -inf per-sample weights', lse, want[1], FWD, cell_ref(y, mean, var, lw, None, False, np.float32)[1], pattern)
    check('cell mse, -inf per-sample weights', mse, want[0], FWD, None, pattern)
    got = losses.diagonal_gaussian_logprob(dev(y), dev(mean), dev(var), dev(lw))
    check('loli, -inf per-sample weights', got, oracle, FWD, None, pattern)
    # with the mask as well
    want_m = cell_ref(y, mean, var, lw, mask, False)
    _, lse_m = run_cells(y, mean, var, lw, mask, False, True, False)
    check('cell lse, -inf per-sample weights, mask', lse_m, want_m[1], FWD, None, pattern)


# ---------------------------------------------------------------------------------------------------------------- Bernoulli
def bern_rows(y, logits, mask):
    """rows_nks = sum_d m_nd * -softplus(-logit_nksd y_nd)   (vae.py:190-192, losses.py:61-69, evaluated stably)"""
    z = -logits * y[:, None, None, :]
    px = -torch.logaddexp(z, torch.zeros_like(z))
    if mask is not None:
        px = px * mask[:, None, None, :].to(px.dtype)
    return px.sum(-1)


def bern_rows_vs_oracle(y, logits, mask, r):
    """on logits without the +-60 / +-100 entries (the oracle's literal log(1 + exp(.)) overflows there)"""
    from oracle import metrics, nets
    N, K, S, D = logits.shape
    T = lambda a: cpu(a, torch.float64)
    rr = T(r.random((N, K)))
    lw = T(log_softmax(r.standard_normal((N, K)), 1))
    rows = bern_rows(T(y), T(logits), None)
    agree((rr * rows.mean(-1)).sum(), nets.expected_bernoulli_loglike(T(y), T(logits), rr), 'expected_bernoulli_loglike')
    tm = torch.as_tensor(mask)
    rows_m = bern_rows(T(y), T(logits), tm)
    want = (torch.logsumexp(torch.logsumexp(rows_m + lw[:, :, None], dim=1), dim=-1) - float(S)).mean()
    agree(want, metrics.bernoulli_logprob(T(y), T(logits), lw, tm), 'bernoulli_logprob')


@pytest.mark.parametrize('N,K,S', [(1, 1, 1), (7, 3, 3), (4, 4, 4), (5, 1, 13), (10, 3, 10)], ids=['R1', 'R63', 'R64', 'R65', 'R300'])
@pytest.mark.parametrize('D', [1, 6, 31, 32, 40, 64, 65, 130])
def test_bernoulli_rows_shapes(D, N, K, S):
    """BernoulliRowsFn forward and gradient: bern_kernel<false/true>, one lane per row below D = 32, one wave per row from D = 32
    (D = 32, 40: idle lanes; 64: full; 65, 130: the d += 64 stride); logits at +-60 / +-100 stay finite in value and gradient"""
    from vmp_for_svae_amd.models import _svae_ops
    r = rng_for(107, D, N, K, S)
    y = f32(np.where(r.random((N, D)) < 0.5, -1.0, 1.0))
    logits = f32(3 * r.standard_normal((N, K, S, D)))
    mask = r.random((N, D)) < 0.3
    bern_rows_vs_oracle(y, logits, mask, r)
    flat = logits.reshape(-1)
    ext = np.array([60.0, -60.0, 100.0, -100.0], np.float32)[:min(4, flat.size)]
    flat[r.permutation(flat.size)[:ext.size]] = ext
    g = f32(r.standard_normal((N, K, S)))
    for m_ in (None, mask):
        fo = lambda l_, y_: bern_rows(y_, l_, None if m_ is None else torch.as_tensor(m_))
        fk = lambda l_, y_: _svae_ops.BernoulliRowsFn.apply(y_, l_, None if m_ is None else dev(m_, torch.bool))
        o64, o32, got = three_ways([logits, y], g, fo, fk, 1)
        tag = (N, K, S, D, 'nomask' if m_ is None else 'mask30')
        assert torch.isfinite(got[0]).all().item() and torch.isfinite(got[1][0]).all().item()
        check('bernoulli rows', got[0], o64[0], FWD, o32[0], tag)
        check('bernoulli grad logits', got[1][0], o64[1][0], GRAD, o32[1][0], tag)


# ------------------------------------------------------------------------------------------------------------------ grid caps
# one case per launcher, D or Dy = 1; the caps are the launchers' own (csrc/vmp_density.hip, csrc/vmp_loglike.hip): the case is above
# the cap, so part of the work is done by the grid-stride loop's second trip, and its last tile is partial
def gauss_d1(x, e1, e2):
    """log N(x | eta1, eta2) at D = 1 (gaussian.py:74-105 with 1x1 matrices); x (N,K,S), e1, e2 (N,K)"""
    e1, e2 = e1[:, :, None], e2[:, :, None]
    return e1 * x + e2 * x * x + 0.25 * e1 * e1 / e2 - 0.5 * LOG2PI + 0.5 * torch.log(-2.0 * e2)


def gauss_d1_inputs(N, K, S, *key):
    r = rng_for(108, N, K, S, *key)
    a = 0.3 * r.standard_normal((N, K))
    return f32(r.standard_normal((N, K, S))), f32(r.standard_normal((N, K))), f32(-0.5 * (a * a + 0.5)), r


def test_grid_cap_gauss_nat_both_forms():
    """gauss_nat_kernel<1>, cap 4096 blocks x 4 waves = 16384 wave tiles; K = 64 is one row per tile: N = 16411"""
    from oracle import dists
    L = L_()
    T = lambda a: cpu(a, torch.float64)
    xs, s1, s2, r = gauss_d1_inputs(5, 64, 3, 0)                                                     # closed form vs oracle, small
    agree(gauss_d1(T(xs), T(s1), T(s2)), dists.gauss_log_probability_nat_per_samp(T(xs)[..., None], T(s1)[..., None], T(s2)[..., None, None]), 'gauss D=1')
    N, K = 16411, 64
    assert (N + 3) // 4 > 4096
    x, e1, e2, r = gauss_d1_inputs(N, K, 1)
    lw = f32(log_softmax(r.standard_normal(K), 0))
    xn = np.ascontiguousarray(x[:, 0, :])                                                            # (N, 1): the normalised form's x
    agree(torch.log_softmax(gauss_d1(T(xn[:5])[:, None, :].expand(5, K, 1), T(e1[:5]), T(e2[:5]))[..., 0] + T(lw), dim=1),
          dists.gauss_log_probability_nat(T(xn[:5]), T(e1[:5])[..., None], T(e2[:5])[..., None, None], torch.exp(T(lw))), 'gauss D=1 normalised')
    dx, dxn, d1, d2, dlw = dev(x), dev(xn), dev(e1), dev(e2), dev(lw)
    out = Guarded(N, K)
    run_twice('vmp_gauss_logprob_nat_per_samp', (L.ptr(dx), L.ptr(d1), L.ptr(d2), N, K, 1, 1, L.ptr(out.full), L.stream()), [out])
    refs = [gauss_d1(cpu(x, dt), cpu(e1, dt), cpu(e2, dt))[..., 0] for dt in (torch.float64, torch.float32)]
    check('grid cap: gauss per-samp', out.t, refs[0], PER_SAMP, refs[1], (N, K, 1, 1))
    for name, w_, p_ in (('', None, None), (' +weights', lw, dlw)):
        run_twice('vmp_gauss_logprob_nat', (L.ptr(dxn), L.ptr(d1), L.ptr(d2), L.ptr(p_), N, K, 1, L.ptr(out.full), L.stream()), [out])
        refs = []
        for dt in (torch.float64, torch.float32):
            lp = gauss_d1(cpu(xn, dt)[:, None, :].expand(N, K, 1), cpu(e1, dt), cpu(e2, dt))[..., 0]
            refs.append(torch.log_softmax(lp if w_ is None else lp + cpu(w_, dt), dim=1))
        check('grid cap: gauss nat normalised' + name, out.t, refs[0], FWD, refs[1], (N, K, 1))


def student_d1(y, mu, W, cst, nu):
    """the kernel's parametrisation at D = 1: cst_k - 1/2 (nu_k + 1) log1p((W_k (y - mu_k))^2 / nu_k); y (N,K,S), the rest (K)"""
    z = W[None, :, None] * (y - mu[None, :, None])
    return cst[None, :, None] - 0.5 * (nu[None, :, None] + 1.0) * torch.log1p(z * z / nu[None, :, None])


def student_d1_inputs(N, K, S, *key):
    from oracle import dists
    r = rng_for(109, N, K, S, *key)
    y, mu = f32(r.standard_normal((N, K, S))), f32(2 * r.standard_normal(K))
    sig = (0.4 * r.standard_normal(K)) ** 2 + 0.5
    nu = f32(3.0 + 4.0 * r.random(K))
    v64 = torch.tensor(nu.astype(np.float64))
    cst = torch.lgamma(0.5 * (v64 + 1)) - torch.lgamma(0.5 * v64) - 0.5 * torch.log(math.pi * v64) - 0.5 * torch.log(torch.tensor(sig))
    W = 1.0 / np.sqrt(sig)
    T = lambda a: cpu(a, torch.float64)
    n = min(N, 6)                                                                                    # closed form vs oracle, small
    agree(student_d1(T(y[:n]), T(mu), T(W), cst, v64),
          dists.student_t_log_probability_per_samp(T(y[:n])[..., None], T(mu)[:, None], T(sig)[:, None, None], v64), 'student-t D=1')
    return y, mu, f32(W), f32(cst.numpy()), nu, f32(r.standard_normal((N, K, S)))


def test_grid_cap_student_t():
    """student_t_kernel<1>, cap 8192 blocks x 256 lanes = 2 097 152 sample rows: (2051, 64, 16) = 2 100 224"""
    L = L_()
    N, K, S = 2051, 64, 16
    assert N * K * S > 8192 * 256
    y, mu, W, cst, nu, _ = student_d1_inputs(N, K, S)
    out = Guarded(N, K, S)
    d = [dev(a) for a in (y, mu, W, cst, nu)]                           # kept alive across the launches
    run_twice('vmp_student_t_logprob', tuple(L.ptr(t) for t in d) + (N, K, S, 1, L.ptr(out.full), L.stream()), [out])
    refs = [student_d1(*[cpu(a, dt) for a in (y, mu, W, cst, nu)]) for dt in (torch.float64, torch.float32)]
    check('grid cap: student-t', out.t, refs[0], PER_SAMP, refs[1], (N, K, S, 1))


def test_grid_cap_student_t_adjoint_partials():
    """student_t_bwd_kernel<1>: N S = 17000 > 64 blocks x 256 lanes; all 64 partial blocks in use, summed in a fixed order"""
    L = L_()
    N, K, S = 1700, 3, 10
    assert L.lib().vmp_student_t_bwd_blocks(N, S) == 64 and N * S > 64 * 256
    y, mu, W, cst, nu, g = student_d1_inputs(N, K, S)
    refs = []
    for dt in (torch.float64, torch.float32):
        ts = [cpu(a, dt, grad=True) for a in (y, mu, W, cst)]
        refs.append(torch.autograd.grad((student_d1(*ts, cpu(nu, dt)) * cpu(g, dt)).sum(), ts))
    gy, part = Guarded(N, K, S), Guarded(64, K, 3)
    d = [dev(a) for a in (y, mu, W, nu, g)]
    run_twice('vmp_student_t_logprob_bwd', tuple(L.ptr(t) for t in d) + (N, K, S, 1, L.ptr(gy.full), L.ptr(part.full), L.stream()),
              [gy, part])
    tot = part.t.double().sum(0)                                       # [d mu | d W | d cst] per component
    check('grid cap: student-t grad y', gy.t, refs[0][0], GRAD, refs[1][0], (N, K, S, 1))
    for i, n_ in enumerate(('mu', 'W', 'cst')):
        check('grid cap: student-t grad ' + n_, tot[:, i], refs[0][1 + i], GRAD, refs[1][1 + i], (N, K, S, 1))


def test_grid_cap_gauss_adjoint_and_mahalanobis():
    """gauss_nat_bwd_kernel<1> and maha_kernel, cap 8192 blocks x 256 lanes = 2 097 152 cells: N = 32771, K = 64 is 2 097 344"""
    from oracle import mixtures
    L = L_()
    N, K = 32771, 64
    assert N * K > 8192 * 256
    x, e1, e2, r = gauss_d1_inputs(N, K, 1, 1)
    g = f32(r.standard_normal((N, K, 1)))
    refs = []
    for dt in (torch.float64, torch.float32):
        ts = [cpu(a, dt, grad=True) for a in (x, e1, e2)]
        refs.append(torch.autograd.grad((gauss_d1(*ts) * cpu(g, dt)).sum(), ts))
    outs = [Guarded(N, K, 1), Guarded(N, K), Guarded(N, K)]
    d = [dev(a) for a in (x, e1, e2, g)]
    run_twice('vmp_gauss_logprob_nat_per_samp_bwd', tuple(L.ptr(t) for t in d) + (N, K, 1, 1, L.ptr(outs[0].full), L.ptr(outs[1].full),
                                                                                  L.ptr(outs[2].full), L.stream()), outs)
    for i, n_ in enumerate(('x', 'eta1', 'eta2')):
        check('grid cap: gauss per-samp grad ' + n_, outs[i].t, refs[0][i], GRAD, refs[1][i], (N, K, 1, 1))
    # Mahalanobis at the same cell count
    xm, m = f32(2 * r.standard_normal((N, 1))), f32(2 * r.standard_normal((K, 1)))
    P, v, beta = f32(0.5 + r.random((K, 1, 1))), f32(3.0 + 4.0 * r.random(K)), f32(0.5 + 2.0 * r.random(K))
    maha = lambda dt: cpu(v, dt)[None, :] * (cpu(xm, dt) - cpu(m, dt)[None, :, 0]) ** 2 * cpu(P, dt)[None, :, 0, 0] + 1.0 / cpu(beta, dt)[None, :]
    T = lambda a: cpu(a, torch.float64)
    agree(maha(torch.float64)[:7], mixtures.gmm_expct_mahalanobis(T(xm[:7]), T(beta), T(m), T(P), T(v)), 'mahalanobis D=1')
    out = Guarded(N, K)
    d = [dev(a) for a in (xm, m, P, v, beta)]
    run_twice('vmp_mix_mahalanobis', tuple(L.ptr(t) for t in d) + (None, N, 1, K, L.ptr(out.full), L.stream()), [out])
    check('grid cap: mahalanobis', out.t, maha(torch.float64), FWD, maha(torch.float32), (N, 1, K))


def test_grid_cap_loglike_and_eval():
    """loglike_kernel<false/true> and eval_kernel, cap 4096 blocks x 4 waves = 16384 wave tiles; S = 33 is one cell per tile:
    N K = 5471 x 3 = 16413 cells"""
    L = L_()
    N, K, S, Dy = 5471, 3, 33, 1
    assert N * K > 4096 * 4 and 64 // S == 1
    y, mean, var, gA, r = diag_inputs(N, K, S, Dy, 3)
    diag_A_vs_oracle(y[:9], mean[:9], var[:9], r)
    refs = []
    for dt in (torch.float64, torch.float32):
        ts = [cpu(a, dt, grad=True) for a in (mean, var)]
        A = diag_A(cpu(y, dt), ts[0], ts[1], 1e-8)
        refs.append((A.detach(),) + torch.autograd.grad((A * cpu(gA, dt)).sum(), ts))
    dy, dm, dv, dg = dev(y), dev(mean), dev(var), dev(gA)
    A, gm, gv = Guarded(N, K), Guarded(N, K, S, Dy), Guarded(N, K, S, Dy)
    run_twice('vmp_diag_gauss_loglike_fwd', (L.ptr(dy), L.ptr(dm), L.ptr(dv), N, K, S, Dy, 1e-8, L.ptr(A.full), L.stream()), [A])
    run_twice('vmp_diag_gauss_loglike_bwd', (L.ptr(dy), L.ptr(dm), L.ptr(dv), L.ptr(dg), N, K, S, Dy, 1e-8, L.ptr(gm.full), L.ptr(gv.full),
                                             L.stream()), [gm, gv])
    check('grid cap: diag-gauss A', A.t, refs[0][0], FWD, refs[1][0], (N, K, S, Dy))
    check('grid cap: diag-gauss grad mean', gm.t, refs[0][1], GRAD, refs[1][1], (N, K, S, Dy))
    check('grid cap: diag-gauss grad var', gv.t, refs[0][2], GRAD, refs[1][2], (N, K, S, Dy))
    lw = f32(log_softmax(r.standard_normal((N, K, S)), 1))
    cell_ref_vs_oracle(y[:9], mean[:9], var[:9], f32(log_softmax(r.standard_normal((9, K)), 1)), lw[:9], r.random((9, Dy)) < 0.3)
    mse, lse = Guarded(N, K), Guarded(N, K)
    dlw = dev(lw)
    run_twice('vmp_eval_cell_metrics', (L.ptr(dy), L.ptr(dm), L.ptr(dv), L.ptr(dlw), 1, None, 0, N, K, S, Dy, L.ptr(mse.full),
                                        L.ptr(lse.full), L.stream()), [mse, lse])
    want, r32 = cell_ref(y, mean, var, lw, None, False), cell_ref(y, mean, var, lw, None, False, np.float32)
    check('grid cap: cell mse', mse.t, want[0], FWD, r32[0], (N, K, S, Dy))
    check('grid cap: cell lse', lse.t, want[1], FWD, r32[1], (N, K, S, Dy))


@pytest.mark.parametrize('form,N,K,S,D', [('wave', 2345, 7, 1, 32), ('lane', 149799, 7, 1, 1)])
def test_grid_cap_bernoulli(form, N, K, S, D):
    """bern_kernel, cap 4096 blocks x 4 waves: the wave-per-row form (D = 32) at 16415 > 16384 rows, the lane-per-row form (D = 1) at
    1 048 593 > 1 048 576 rows"""
    L = L_()
    R = N * K * S
    assert R > 4096 * 4 * (1 if form == 'wave' else 64) and (D >= 32) == (form == 'wave')
    r = rng_for(110, N, K, S, D)
    y = f32(np.where(r.random((N, D)) < 0.5, -1.0, 1.0))
    logits = f32(3 * r.standard_normal((N, K, S, D)))
    mask = r.random((N, D)) < 0.3
    bern_rows_vs_oracle(y[:9], logits[:9], mask[:9], r)
    logits.reshape(-1)[r.permutation(logits.size)[:4]] = np.array([60.0, -60.0, 100.0, -100.0], np.float32)
    g = f32(r.standard_normal((N, K, S)))
    refs = []
    for dt in (torch.float64, torch.float32):
        lg = cpu(logits, dt, grad=True)
        rows = bern_rows(cpu(y, dt), lg, torch.as_tensor(mask))
        refs.append((rows.detach(), torch.autograd.grad((rows * cpu(g, dt)).sum(), [lg])[0]))
    dy, dl, dm, dg = dev(y), dev(logits), dev(mask, torch.uint8), dev(g)
    rows, gl = Guarded(N, K, S), Guarded(N, K, S, D)
    run_twice('vmp_bernoulli_rows_fwd', (L.ptr(dy), L.ptr(dl), L.ptr(dm), N, K, S, D, L.ptr(rows.full), L.stream()), [rows])
    run_twice('vmp_bernoulli_rows_bwd', (L.ptr(dy), L.ptr(dl), L.ptr(dm), L.ptr(dg), N, K, S, D, L.ptr(gl.full), L.stream()), [gl])
    check('grid cap: bernoulli rows (%s form)' % form, rows.t, refs[0][0], FWD, refs[1][0], (N, K, S, D))
    check('grid cap: bernoulli grad logits (%s form)' % form, gl.t, refs[0][1], GRAD, refs[1][1], (N, K, S, D))
