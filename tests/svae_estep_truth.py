"""Generic parameters and the fp64 truth of the SVAE E-step's N-sized forms (tests/test_svae_estep_forms_gpu.py, the direct-step
sweep of tests/test_smm_direct_step_gpu.py; checked by tests/test_svae_estep_truth.py).  CPU only: nothing here touches a GPU.

Why generic: svae.init_mm + svae.init_recognition_params give C = c I for every component, so the recognition L_k is diagonal and
P_k, W_k are the same multiple of the identity for all k - a transposed read of a triangle, a k / k' mix-up in a table, a wrong
packed stride or a dropped off-diagonal term all give the right answer there.  generic_params has none of these symmetries.

Everything goes through oracle.svae_ref.e_step and oracle.dists, in the dtype asked for (fp64: the truth; fp32: what the
reference's own arithmetic loses on the shape, which sets the bars).  `mutate` hooks exist for the sensitivity test alone."""
import contextlib

import numpy as np
import torch

from oracle import dists, philox, svae_ref

FWD_FORMS = ('none', 'fwd1', 'tile', 'pst', 'pst2', 'chunked', 'fwd3')             # FwdForm of csrc/vmp_svae.hip (vmp_svae_launch_plan)
BWD_FORMS = ('none', 'bwd1', 'ring', 'generic_one', 'generic_stream')              # BwdForm

# ---- the sweeps of tests/test_svae_estep_forms_gpu.py: (form, (N, K, L, S)); in-kernel noise, generic phi, Gaussian theta
FWD1_SHAPES = [(7, 3, 1, 4), (130, 7, 2, 6), (40, 4, 3, 8), (257, 16, 4, 5), (96, 5, 5, 4), (200, 16, 6, 10), (33, 33, 7, 8),
               (64, 10, 8, 10), (100, 16, 8, 15), (256, 64, 8, 16), (1, 1, 8, 1)]
RNG_CASES = ([('fwd1', s) for s in FWD1_SHAPES]
             + [('tile', s) for s in [(1600, 10, 8, 10), (1100, 16, 6, 10), (1100, 16, 4, 10), (5500, 3, 2, 10),               # ST = 10
                                      (1100, 16, 8, 4), (2400, 7, 5, 8), (300, 33, 3, 4), (1100, 16, 7, 4), (16500, 1, 1, 8)]]  # ST = 0
             + [('pst', s) for s in [(1100, 16, 8, 12), (1100, 16, 8, 13), (50, 16, 8, 20), (130, 9, 8, 20), (9, 16, 8, 100)]]
             + [('pst2', s) for s in [(1100, 16, 8, 10), (2400, 7, 8, 10), (2200, 8, 8, 10)]])
MOM_SHAPES = [(1100, 16, 8, 10), (1100, 16, 8, 12), (50, 16, 8, 20)]                # vmp_svae_fwd_mom_blocks > 0 is asserted there
# Student-t theta: one shape per form, fwd1 at L = 4 and L = 8, and the C5 minibatch
RNG_CASES_T = [('fwd1', (257, 16, 4, 5)), ('fwd1', (64, 10, 8, 10)), ('fwd1', (64, 16, 8, 10)), ('tile', (1100, 16, 6, 10)),
               ('pst', (50, 16, 8, 20)), ('pst2', (1100, 16, 8, 10))]
AT_CASE = ('tile', (40, 4, 3, 8), 1000)                                            # vmp_svae_estep_fwd_rng_at: (form, shape, row0)
# noise-tensor forms with a generic Gaussian theta: (forward form, backward form, shape, nblk: 'for' = vmp_svae_bwd_blocks_for, the
# autograd path's; 'blocks' = vmp_svae_bwd_blocks, vmp_svae_estep_bwd's)
TENSOR_CASES = [('tile', 'bwd1', (37, 10, 6, 10), 'for'), ('chunked', 'generic_one', (21, 10, 2, 100), 'for'),
                ('fwd3', 'bwd1', (5, 3, 2, 3), 'for'), ('tile', 'ring', (257, 16, 8, 10), 'blocks'),
                ('tile', 'generic_one', (64, 10, 8, 10), 'blocks'), ('tile', 'ring', (12500, 10, 8, 4), 'for'),
                ('tile', 'generic_stream', (40000, 10, 2, 10), 'blocks')]
# the direct-step sweep (tests/test_smm_direct_step_gpu.py): (N, K, L, U, Dy, S)
DIRECT_SHAPES = [(64, 16, 8, 50, 8, 10), (64, 10, 8, 50, 6, 16), (512, 8, 6, 50, 6, 10), (40, 20, 4, 32, 4, 6), (30, 33, 2, 16, 2, 4),
                 (37, 7, 4, 33, 3, 8), (5, 3, 2, 16, 1, 4),
                 (24, 3, 1, 16, 2, 4), (40, 4, 3, 24, 3, 8), (48, 5, 5, 40, 5, 4), (33, 33, 7, 48, 7, 8)]     # the odd latent sizes
NET_VARS = ('layer_0/kernel', 'layer_0/bias', 'layer_1/kernel', 'layer_1/bias', 'gaussian_output/kernel', 'gaussian_output/bias',
            'shortcut/W', 'shortcut/b1', 'shortcut/b2')


def case_seed(shape, student=False, salt=0):
    """The seed of a sweep case: parameters, inputs and the Philox key all derive from it.  SEED_BUMP holds the cases whose first seed
    put a row's uniform so close to a step of the cumulative r that the oracle's fp64 and fp32 picks differ (test_svae_estep_truth.py
    checks every case); the entry is the salt that cleared it."""
    N, K, L, S = shape[:4]
    base = 1000003 * N + 10007 * K + 101 * L + S + (500009 if student else 0)
    return base + 7919 * (salt + SEED_BUMP.get((tuple(shape), bool(student)), 0))


SEED_BUMP = {}


def _t(a, dt, grad=False):
    return torch.tensor(np.asarray(a), dtype=dt, requires_grad=grad)


class Params(object):
    """phi = [mu_k, L_raw, pi_raw]; theta = natural [alpha, A, b, beta, v_hat] (Gaussian) or [alpha_nat, mu_k, L_raw, dof] (Student-t);
    numpy fp64.  as_torch(dtype) gives CPU tensors: fp64 for the truth, fp32 contiguous - ready for .cuda() - for the device."""

    def __init__(self, phi, theta, student):
        self.phi, self.theta, self.student = [np.asarray(a, np.float64) for a in phi], [np.asarray(a, np.float64) for a in theta], student

    def as_torch(self, dtype):
        return [_t(a, dtype) for a in self.phi], [_t(a, dtype) for a in self.theta]


def generic_params(K, L, rng, student=False):
    """phi: mu_k ~ 2 N(0,1), full L_raw ~ 0.4 N(0,1), random pi_raw.  Gaussian theta: a standard NIW with its own SPD C_k = B B^T + L I
    (B ~ 0.6 N(0,1)), beta_k, v_k > L + 1 and alpha_k in (0.1, 3) all distinct, m_k ~ 2 N(0,1) - to natural form by the oracle's maps.
    Student-t theta: as tests/test_svae_gpu.py test_estep_vs_oracle_shapes_student_t."""
    phi = [rng.standard_normal((K, L)) * 2, rng.standard_normal((K, L, L)) * 0.4, rng.standard_normal(K)]
    if student:
        theta = [rng.random(K) * 3.0, rng.standard_normal((K, L)) * 1.5, np.tril(rng.standard_normal((K, L, L)) * 0.4) + 0.8 * np.eye(L),
                 2.5 + 5.0 * rng.random(K)]
        return Params(phi, theta, True)
    B = rng.standard_normal((K, L, L)) * 0.6
    C = B @ B.transpose(0, 2, 1) + L * np.eye(L)
    beta = 0.5 + 2.0 * (np.arange(K) + rng.random(K)) / K
    v = L + 1.5 + 3.0 * (rng.permutation(K) + rng.random(K)) / K
    m = rng.standard_normal((K, L)) * 2
    alpha = 0.1 + 2.9 * (rng.permutation(K) + rng.random(K)) / K
    f = lambda a: _t(a, torch.float64)
    A, b, beta_n, v_hat = dists.niw_standard_to_natural(f(beta), f(m), f(C), f(v))
    return Params(phi, [dists.dir_standard_to_natural(f(alpha)).numpy(), A.numpy(), b.numpy(), beta_n.numpy(), v_hat.numpy()], False)


def init_point_params(K, L, rng):
    """The point the older tests stand on: svae_ref.init_mm + init_recognition_params (C = c I for every component; the recognition
    variables are what init_recognition_params returns, svae.py:488-496)."""
    m_unif, pi_n = rng.random((K, L)), rng.standard_normal(K)
    _, theta = svae_ref.init_mm(K, L, _t(m_unif, torch.float64), torch.float64)
    phi = svae_ref.init_recognition_params(theta, _t(pi_n, torch.float64))
    return Params([p.numpy() for p in phi], [t.numpy() for t in theta], False)


def inputs(shape, rng):
    """encoder outputs (eta1, eta2 diagonal) and the probe weights wx of a case"""
    N, K, L, S = shape
    return rng.standard_normal((N, L)), -0.5 * (0.3 + rng.random((N, L))), rng.standard_normal((N, K, S, L))


def sweep_case(shape, student=False):
    """(params, eta1, eta2d, wx, seed) of a sweep case: everything derives from case_seed, which is also the Philox key"""
    seed = case_seed(shape, student)
    rng = np.random.Generator(np.random.PCG64(seed))
    params = generic_params(shape[1], shape[2], rng, student)
    e1, e2, wx = inputs(shape, rng)
    return params, e1, e2, wx, seed


def recognition_P(phi, dtype=torch.float64):
    """P_k = L_k L_k^T of phi (K, L, L)"""
    return -2.0 * svae_ref.unpack_recognition_gmm([_t(a, dtype) for a in phi])[1]


def theta_W(theta, dtype=torch.float64):
    """the packed W_k of a Gaussian theta: lower, W^T W = E[Sigma_k]^-1 (include/vmp_hip.h vmp_svae_estep_fwd)"""
    th = [_t(a, dtype) for a in theta]
    _, sigma = dists.niw_expected_values(*dists.niw_natural_to_standard(*th[1:]))
    return dists.inv(dists.chol(sigma))


# ---- mutations (the sensitivity test): what a wrong kernel would compute, applied inside the oracle's own graph
def mut_P_transposed(e1k, e2k, pi):
    """The lower-triangular factor of P_k read transposed.  (P_k itself is symmetric - its own transpose is no mutation - so the
    transposed read is taken where it bites: L_k^T L_k in place of L_k L_k^T.)"""
    Lc = dists.chol(-2.0 * e2k)
    return e1k, -0.5 * (Lc.transpose(-1, -2) @ Lc), pi


def mut_P_swapped(e1k, e2k, pi):
    """P_0 and P_1 swapped in the table (h_k, pi_k stay)"""
    idx = list(range(e2k.shape[0]))
    idx[0], idx[1] = 1, 0
    return e1k, e2k[idx], pi


def mut_W_offdiag(W):
    """one off-diagonal of every W_k dropped"""
    W = W.clone()
    W[:, -1, 0] = 0.0
    return W


@contextlib.contextmanager
def _mutated_unpack(fn):
    if fn is None:
        yield
        return
    orig = svae_ref.unpack_recognition_gmm
    svae_ref.unpack_recognition_gmm = lambda phi_gmm: fn(*orig(phi_gmm))
    try:
        yield
    finally:
        svae_ref.unpack_recognition_gmm = orig


def _theta_logp(x, theta, student, mut_W=None):
    """log p(x_nks, z = k | theta) (N,K,S): svae.py:229-243 (Gaussian, stop_gradient) / 288-300 (Student-t)"""
    N, K, S, L = x.shape
    if student:
        mu, sig = svae_ref.unpack_smm(theta[1:3])
        elp = dists.dir_expected_log_pi(dists.dir_natural_to_standard(theta[0]))
        return dists.student_t_log_probability_per_samp(x, mu, sig, theta[3]) + elp.view(1, K, 1)
    mu, sig = dists.niw_expected_values(*dists.niw_natural_to_standard(*theta[1:]))
    e1t, e2t = dists.gauss_standard_to_natural(mu, sig)
    if mut_W is not None:
        W = mut_W(dists.inv(dists.chol(sig)))
        e2t = -0.5 * (W.transpose(-1, -2) @ W)
        e1t = (-2.0 * e2t @ mu.unsqueeze(-1)).reshape(mu.shape)
    elp = dists.dir_expected_log_pi(dists.dir_natural_to_standard(theta[0]))
    return dists.gauss_log_probability_nat_per_samp(x, e1t.unsqueeze(0).repeat(N, 1, 1), e2t.unsqueeze(0).repeat(N, 1, 1, 1)) + elp.view(1, K, 1)


def estep_truth(params, e1, e2, noise, wx=None, dtype=torch.float64, mut_unpack=None, mut_W=None):
    """x (N,K,S,L), log z, T', r of the E-step and - when the probe weights wx are given - the gradients of the probe loss
    (x wx).sum() + (exp(lz) (T' + lz)).sum() w.r.t. eta1, eta2d, mu_k, L_k, log_pi_k (Student-t: also theta/mu_k, theta/L_k).
    `noise` (N,K,L,S): the device's own materialised stream raised to `dtype`."""
    phi, theta = params.as_torch(dtype)
    grad = wx is not None
    oe1, oe2 = _t(e1, dtype, grad), _t(e2, dtype, grad)
    phi = [p.requires_grad_(grad) for p in phi]
    wrt = [oe1, oe2] + phi
    if params.student and grad:
        theta[1].requires_grad_(True)
        theta[2].requires_grad_(True)
        wrt += [theta[1], theta[2]]
    with contextlib.ExitStack() as st:
        if not grad:
            st.enter_context(torch.no_grad())
        st.enter_context(_mutated_unpack(mut_unpack))
        x, lz, pt, _ = svae_ref.e_step((oe1, oe2), phi, torch.as_tensor(noise).to(dtype))
        N, K, S, L = x.shape
        num = dists.gauss_log_probability_nat_per_samp(x, pt[0].reshape(N, K, L), pt[1])
        Tp = (num - _theta_logp(x, theta, params.student, mut_W)).mean(-1)
        out = dict(x=x.detach(), lz=lz.detach(), Tp=Tp.detach(), r=torch.exp(lz.detach()))
        if grad:
            loss = (x * _t(wx, dtype)).sum() + (torch.exp(lz) * (Tp + lz)).sum()
            out['grads'] = [g.detach() for g in torch.autograd.grad(loss, wrt)]
    return out


GRAD_NAMES = ('eta1', 'eta2d', 'mu_k', 'L_k', 'log_pi_k', 'theta/mu_k', 'theta/L_k')


def bars(t64, t32):
    """The project's clauses (tests/test_svae_gpu.py): x and T' relative to their largest entry, r absolute, each
    max(1e-5, 3 |oracle fp64 - oracle fp32|) on this very shape.  Returns (bars, the fp32 oracle's own loss)."""
    ref = dict(x=float((t32['x'].double() - t64['x']).abs().max() / t64['x'].abs().max()),
               r=float((t32['r'].double() - t64['r']).abs().max()),
               Tp=float((t32['Tp'].double() - t64['Tp']).abs().max() / t64['Tp'].abs().max()))
    return {k: max(1e-5, 3 * v) for k, v in ref.items()}, ref


def grad_bar(S, g64=None, g32=None):
    """fp32 accumulation over N S sample adjoints: 2e-4 of max-abs at S <= 10, growing as sqrt(S / 10) - or, where the reference's
    own fp32 arithmetic loses more on this very gradient, 3 x that (the clause of x, r and T').  That happens to log_pi_k at generic
    parameters: its gradient is what is left of terms r (T' + log z) of size |T'| ~ 1e2 after the softmax's projection - at
    (96, 5, 5, 4) a largest entry of 1.2e-2, of which the fp32 oracle loses 1.8e-4.  Returns (bar, the fp32 oracle's loss or None)."""
    base = 2e-4 * max(1.0, S / 10.0) ** 0.5
    if g64 is None:
        return base, None
    o32 = float((g32.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-300))
    return max(base, 3 * o32), o32


# ---- epilogue: the one-draw sub-sample, the M-step's raw moments, the CVI step
def picks(r, seed, margin=None):
    """z_n = inverse CDF of oracle.philox.subsample_uniforms(seed) on the cumulative r (csrc/vmp_svae.hip subsample_kernel).
    margin: also the rows whose uniform lies within `margin` of a step of the cumulative r (bool mask)."""
    N, K = r.shape
    u = torch.as_tensor(philox.subsample_uniforms(int(seed) & 0xFFFFFFFFFFFFFFFF, N, 1)[:, 0]).double()
    cdf = torch.cumsum(r.double(), dim=1)[:, :K - 1]
    z = (cdf <= u[:, None]).sum(1)
    if margin is None:
        return z
    near = ((cdf - u[:, None]).abs() <= margin).any(1) if K > 1 else torch.zeros(N, dtype=torch.bool)
    return z, near


def raw_moments(x_s, r):
    """sum_n r_nk [1 | 1 | x | x x^T] (K, 2 + L + L L), the vmp_mix_stats layout, in fp64; and the same sum of absolute values"""
    xd, rd = x_s.double(), r.double()
    K, L = rd.shape[1], xd.shape[1]
    n = rd.sum(0)[:, None]
    mom = torch.cat([n, n, rd.t() @ xd, torch.einsum('nk,ni,nj->kij', rd, xd, xd).reshape(K, L * L)], dim=1)
    scale = torch.cat([n, n, rd.t() @ xd.abs(), torch.einsum('nk,ni,nj->kij', rd, xd.abs(), xd.abs()).reshape(K, L * L)], dim=1)
    return mom, scale


def moment_bar(t64, t32, z):
    """Per element: the 2e-6 of sum r |x||x| the kernel meets against its OWN samples (tests/test_philox.py
    test_estep_epilogue_equals_the_standalone_kernels) plus 3 x the fp32 oracle's loss on x and r carried through the sum,
    sum_n |dr| |x_i||x_j| + r (|dx_i||x_j| + |x_i||dx_j|).  Measured on the fp32 oracle, never on the kernel.  Plus the number
    format's floor: r is an fp32 output and the device flushes what lies below the smallest normal fp32 (at generic parameters whole
    components have N_k of 1e-40 .. 1e-200), so every r_nk may be off by FLT_MIN: sum_n FLT_MIN |x_i||x_j|."""
    n = torch.arange(z.shape[0])
    x64, x32 = t64['x'][n, z, 0, :], t32['x'][n, z, 0, :].double()
    r64, dr = t64['r'], (t32['r'].double() - t64['r']).abs()
    dx, ax = (x32 - x64).abs(), x64.abs()
    K, L = r64.shape[1], x64.shape[1]
    _, scale = raw_moments(x64, r64)
    one = torch.ones_like(ax[:, :1])
    lin = dr.t() @ ax + r64.t() @ dx
    quad = (torch.einsum('nk,ni,nj->kij', dr, ax, ax) + torch.einsum('nk,ni,nj->kij', r64, dx, ax)
            + torch.einsum('nk,ni,nj->kij', r64, ax, dx)).reshape(K, L * L)
    loss = torch.cat([dr.sum(0)[:, None], dr.sum(0)[:, None], lin, quad], dim=1)
    flt_min = float(np.finfo(np.float32).tiny)
    floor = flt_min * torch.cat([one.sum(0), one.sum(0), ax.sum(0), torch.einsum('ni,nj->ij', ax, ax).reshape(L * L)])[None, :]
    return 2e-6 * scale + 3 * loss + floor, loss


def cvi_truth(prior, theta, x_s, r, rho):
    """theta* = svae_ref.m_step on the drawn sample and theta after update_gmm_params, in the dtype of the inputs"""
    star = svae_ref.m_step(prior, x_s, r)
    return star, svae_ref.update_gmm_params(theta, star, rho)


def oracle_prior(K, L, dtype=torch.float64):
    """the prior of svae_ref.init_mm (it does not depend on the uniform draw: m_scale = 0)"""
    return svae_ref.init_mm(K, L, torch.zeros(K, L, dtype=dtype), dtype)[0]


# ---- the direct step: every tensor the trainer starts from, built on the CPU so that the oracle's picks can be checked without a GPU
def direct_setup(shape, smm):
    """dict(w: the 18 network tensors, m_unif, pi_norm, y, params: generic_params, seed) for one case of the direct-step sweep"""
    from oracle import nets
    N, K, L, U, Dy, S = shape
    seed = case_seed((N, K, L, S), smm, salt=17)
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {}
    for scope, din, dout in (('encoder_net', Dy, L), ('decoder_net', L, Dy)):
        shapes = {'layer_0/kernel': (din, U), 'layer_0/bias': (U,), 'layer_1/kernel': (U, U), 'layer_1/bias': (U,),
                  'gaussian_output/kernel': (U, 2 * dout), 'gaussian_output/bias': (2 * dout,), 'shortcut/b1': (dout,), 'shortcut/b2': (dout,)}
        for n_, shp in shapes.items():
            w[scope + '/' + n_] = (rng.standard_normal(shp) * 0.3 / np.sqrt(max(1, shp[0] if len(shp) > 1 else 1) / 4.0)).astype(np.float32)
        w[scope + '/shortcut/W'] = nets.rand_partial_isometry(din, dout, 1., 0).astype(np.float32)
    c = rng.standard_normal((K, Dy)) * 2.0
    y = (c[rng.integers(0, K, N)] + 0.5 * rng.standard_normal((N, Dy))).astype(np.float32)
    return dict(w=w, m_unif=rng.random((K, L)).astype(np.float32), pi_norm=rng.standard_normal(K).astype(np.float32), y=y,
                params=generic_params(K, L, rng, smm), seed=seed, model_seed=3)


def direct_oracle_logz(setup, shape, key, dtype):
    """log z of the oracle's inference on the step's own noise (oracle.philox.cell_noise of `key`)"""
    N, K, L, U, Dy, S = shape
    phi, _ = setup['params'].as_torch(torch.float32)                       # the trainer holds fp32 tensors: the fp32 values are the inputs
    enc = {v: torch.as_tensor(setup['w']['encoder_net/' + v]).to(dtype) for v in NET_VARS}
    dec = {v: torch.as_tensor(setup['w']['decoder_net/' + v]).to(dtype) for v in NET_VARS}
    noise = torch.as_tensor(philox.cell_noise(key, np.arange(N * K), L, S)).reshape(N, K, L, S).to(dtype)
    with torch.no_grad():
        return svae_ref.inference(torch.as_tensor(setup['y']).to(dtype), [p.to(dtype) for p in phi], enc, dec, noise,
                                  torch.zeros(N, S, dtype=torch.int64))[4]
