"""fp64 truth, hard parameter families and bars of the SVAE step's K-sized parameter maps (csrc/vmp_prep_parts.h, vmp_prep.hip, vmp_step_parts.h):
recognition unpacking forward / backward, NIW / Dirichlet and Student-t theta packing, the fixed-order reductions of the E-step's partial rows,
the CVI update.  Used by tests/test_svae_kmaps_gpu.py; checked on the CPU by tests/test_svae_kmaps_truth.py.  Nothing here touches a GPU.

Every value is a restatement through oracle.svae_ref / oracle.dists in the dtype asked for - fp64: the truth; fp32: what the reference's own
arithmetic loses on the very case, which sets the bar (`bar`) - and every gradient is torch autograd of a probe loss  sum(out * g_out).  The
inputs are the fp32 values the device sees, raised to fp64 (`Case.as_torch`).  `mut` names ONE deliberate error (MUTATIONS): what a wrong
kernel would compute; the sensitivity test alone passes it.

bias_k is stated as include/vmp_hip.h states it, on the factor L_k = tril(raw) with a softplus diagonal (the three lines of
svae_ref.unpack_recognition_gmm: `recognition_L`) and not through a Cholesky factorisation of P: at the small_diag family P_k has a condition
number of 1e3 and more, its fp32 factorisation loses that many of its seven digits, and the bar - three times that loss - would pass the
1e-3 cap.  The CPU test holds L_k L_k^T equal to the oracle's own P in every family, and L_k to chol(P) wherever P can be factorised."""
import math

import numpy as np
import torch

import svae_estep_truth as E
from oracle import dists, nets, svae_ref

F64, F32 = torch.float64, torch.float32
FAMILIES = ('generic', 'init', 'small_diag', 'large_diag', 'wide_pi', 'alpha_pole', 'low_nu', 'cancelling_b', 'dof_ends')
FAMILY_TABLE = {
    'generic': 'svae_estep_truth.generic_params: full L_raw ~ 0.4 N(0,1), SPD C_k = B B^T + L I, distinct beta_k, v_k, alpha_k',
    'init': 'svae_estep_truth.init_point_params: svae.init_mm + init_recognition_params (C = c I for every k)',
    'small_diag': 'raw diagonal of phi L_k uniform in [-7, -3] (softplus 1e-3 .. 5e-2), sub-diagonal 0.01 N(0,1): cond(P_k) > 1e3',
    'large_diag': 'raw diagonal of phi L_k uniform in [20, 45]: softplus(x) = x to fp64, log1p(exp(-x)) vanishes',
    'wide_pi': 'pi_raw a permutation of linspace(-40, 40, K): min log pi_k = -80',
    'alpha_pole': 'standard alpha_k = alpha_nat + 1 a permutation of logspace(-3, 6, K) (Gaussian and Student-t theta): both ends of digamma',
    'low_nu': 'nu_k = v_hat - (L + 2) uniform in (0.05, 1)',
    'cancelling_b': 'm_k scaled until |b b^T / beta| = 1e3 |C_k| (2-norms): A - b b^T / beta loses three digits',
    'dof_ends': 'Student-t dof a permutation of logspace(log10 2.01, log10 300, K) (1e4 narrowed: fp32 lgamma((nu+L)/2) - lgamma(nu/2) loses 1e-3 there)',
}
# floors: the bars tests/test_prep_gpu.py asserts.  L_k (not asserted there) is one fp32 rounding of an fp64 softplus, 2^-24 relative: the 1e-6 of h_k.
FLOORS = dict(L_k=1e-6, h_k=1e-6, m=1e-6, theta=1e-6, theta_star=1e-6, P=2e-6, bias=2e-6, kappa=2e-6, W=5e-6)
GRAD_FLOOR = 5e-6
BAR_CAP = 1e-3
MUTATIONS = ('L_transposed', 'softplus_grad_dropped', 'gP_lower_only', 'logpi_unnormalised', 'dirichlet_plus1_dropped', 'nu_off_by_one',
             'W_offdiag_zeroed', 'W_upper_nonzero', 'kappa_logdiag_sign', 'smm_gkappa_term_dropped', 'reduce_row_left_out', 'gW_symmetrised')


class Case(object):
    """phi = [mu_k, L_raw, pi_raw]; theta = natural [alpha, A, b, beta, v_hat]; theta_t = [alpha_nat, mu_k, L_raw, dof]; numpy fp64 holding
    fp32-representable values (what the device is given)."""

    def __init__(self, phi, theta, theta_t):
        r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
        self.phi, self.theta, self.theta_t = [r32(a) for a in phi], [r32(a) for a in theta], [r32(a) for a in theta_t]

    def as_torch(self, which, dtype):
        return [torch.tensor(a, dtype=dtype) for a in getattr(self, which)]


def _set_diag(M, d):
    M = M.copy()
    i = np.arange(M.shape[-1])
    M[:, i, i] = d
    return M


def family(name, K, L, rng):
    """A Case of the named family: generic parameters (Gaussian and Student-t theta) with the one hard feature of FAMILY_TABLE."""
    if name == 'init':
        g = E.init_point_params(K, L, rng)
    else:
        g = E.generic_params(K, L, rng)
    phi, theta = [a.copy() for a in g.phi], [a.copy() for a in g.theta]
    theta_t = [a.copy() for a in E.generic_params(K, L, rng, student=True).theta]
    f = lambda a: torch.tensor(a, dtype=F64)
    if name == 'small_diag':
        phi[1] = _set_diag(np.tril(rng.standard_normal((K, L, L)) * 0.01, -1), rng.uniform(-7.0, -3.0, (K, L)))
    elif name == 'large_diag':
        phi[1] = _set_diag(phi[1], rng.uniform(20.0, 45.0, (K, L)))
    elif name == 'wide_pi':
        phi[2] = rng.permutation(np.linspace(-40.0, 40.0, K)) if K > 1 else np.array([40.0])
    elif name == 'alpha_pole':
        theta[0] = rng.permutation(np.logspace(-3.0, 6.0, K)) - 1.0
        theta_t[0] = rng.permutation(np.logspace(-3.0, 6.0, K)) - 1.0
    elif name == 'low_nu':
        theta[4] = L + 2.0 + rng.uniform(0.05, 1.0, K)
    elif name == 'cancelling_b':
        beta, m, C, v = [t.numpy() for t in dists.niw_natural_to_standard(*[f(a) for a in theta[1:]])]
        C = 0.5 * (C + C.transpose(0, 2, 1))
        nC = np.linalg.norm(C, 2, axis=(1, 2))
        m = m / np.linalg.norm(m, axis=1, keepdims=True) * np.sqrt(1e3 * nC / beta)[:, None]
        theta[1:] = [t.numpy() for t in dists.niw_standard_to_natural(f(beta), f(m), f(C), f(v))]
    elif name == 'dof_ends':
        theta_t[3] = rng.permutation(np.logspace(math.log10(2.01), math.log10(300.0), K))
    elif name not in ('generic', 'init'):
        raise KeyError(name)
    return Case(phi, theta, theta_t)


def case_rng(name, K, L):
    return np.random.Generator(np.random.PCG64(7919 * FAMILIES.index(name) + 101 * K + L))


def recognition_L(L_raw):
    """L_k of svae_ref.unpack_recognition_gmm (svae.py:347-352): tril(raw) with a softplus diagonal"""
    Lm = torch.tril(L_raw)
    dg = torch.diagonal(Lm, dim1=-2, dim2=-1)
    return Lm - torch.diag_embed(dg) + torch.diag_embed(nets.softplus(dg))


def _probe(outs, gs):
    return sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, gs))


def phi_truth(mu, L_raw, pi_raw, g=None, dtype=F64, mut=None):
    """dict(L_k, P, bias, logpi [, g_mu, g_Lraw, g_piraw]) of the recognition unpacking (svae.py:342-358, 70-92); g = (g_hk, g_P, g_bias), g_P the
    gradient w.r.t. the full matrix P."""
    t = [torch.as_tensor(a).to(dtype).clone().requires_grad_(g is not None) for a in (mu, L_raw, pi_raw)]
    e1, e2, _ = svae_ref.unpack_recognition_gmm(t)
    Lk, P = recognition_L(t[1]), -2.0 * e2
    if mut == 'L_transposed':
        P = Lk.transpose(-1, -2) @ Lk
    logpi = t[2] if mut == 'logpi_unnormalised' else torch.log_softmax(t[2], -1)
    sol = torch.linalg.solve_triangular(Lk, e1.unsqueeze(-1), upper=False).squeeze(-1)
    bias = -0.5 * (sol * sol).sum(-1) + torch.log(torch.diagonal(Lk, dim1=-2, dim2=-1)).sum(-1) + logpi
    out = dict(L_k=Lk.detach(), P=P.detach(), bias=bias.detach(), logpi=logpi.detach())
    if g is not None:
        g_hk, g_P, g_b = [torch.as_tensor(a).to(dtype) for a in g]
        if mut == 'gP_lower_only':
            g_P = torch.tril(g_P)
        gm, gL, gp = torch.autograd.grad(_probe((e1, P, bias), (g_hk, g_P, g_b)), t)
        if mut == 'softplus_grad_dropped':
            i = torch.arange(gL.shape[-1])
            gL = gL.clone()
            gL[:, i, i] = gL[:, i, i] / torch.sigmoid(t[1].detach()[:, i, i])
        out.update(g_mu=gm, g_Lraw=gL, g_piraw=gp)
    return out


def theta_C(theta, dtype=F64):
    """C_k = A - b b^T / beta of a natural NIW theta, symmetrised"""
    _, _, C, _ = dists.niw_natural_to_standard(*[torch.as_tensor(a).to(dtype) for a in theta[1:]])
    return 0.5 * (C + C.transpose(-1, -2))


def theta_truth(alpha, A, b, beta, v_hat, dtype=F64, mut=None):
    """dict(m, W, kappa): theta side of compute_elbo (svae.py:205-214; niw.py:8-43, dirichlet.py:8-22).  W lower, W^T W = E[Sigma]^-1;
    kappa = sum log W_ii - L/2 log 2 pi + E log pi."""
    th = [torch.as_tensor(a).to(dtype) for a in (alpha, A, b, beta, v_hat)]
    Ld = th[2].shape[-1]
    bk, mk, Ck, vk = dists.niw_natural_to_standard(*th[1:])
    if mut == 'nu_off_by_one':
        vk = vk + 1.0
    mu, sigma = dists.niw_expected_values(bk, mk, Ck, vk)
    W = dists.inv(dists.chol(0.5 * (sigma + sigma.transpose(-1, -2))))
    W = torch.tril(W)                                      # inv of a lower factor: the strict upper triangle is rounding noise of the LU
    elp = dists.dir_expected_log_pi(th[0] if mut == 'dirichlet_plus1_dropped' else dists.dir_natural_to_standard(th[0]))
    ld = torch.log(torch.diagonal(W, dim1=-2, dim2=-1)).sum(-1)
    kappa = (-ld if mut == 'kappa_logdiag_sign' else ld) - 0.5 * Ld * math.log(2 * math.pi) + elp
    return dict(m=mu, W=_mut_W(W, mut), kappa=kappa)


def _mut_W(W, mut):
    if W.shape[-1] == 1:                                   # no off-diagonal, no upper triangle
        return W
    if mut == 'W_offdiag_zeroed':
        W = W.clone()
        W[:, -1, 0] = 0.0
    elif mut == 'W_upper_nonzero':
        W = W.clone()
        W[:, 0, -1] = W[:, -1, 0]
    return W


def smm_theta_truth(alpha, mu, L_raw, dof, g=None, dtype=F64, mut=None):
    """dict(W, kappa [, g_mu, g_Lraw]) of the Student-t theta packing (svae.py:268-277, student_t.py:31-37): W = L_k^-1 (0 above the diagonal),
    kappa_k = lgamma((nu+L)/2) - lgamma(nu/2) - L/2 log(pi nu) - sum log diag L_k + E[log pi_k] - which is the oracle's Student-t log density AT
    its location plus E[log pi_k].  g = (g_m, g_W, g_kappa): gradients w.r.t. theta/mu_k and theta/L_k raw (m = mu_k itself)."""
    al, dofs = torch.as_tensor(alpha).to(dtype), torch.as_tensor(dof).to(dtype)
    t = [torch.as_tensor(a).to(dtype).clone().requires_grad_(g is not None) for a in (mu, L_raw)]
    K, Ld = t[0].shape
    mu_t, sigma = svae_ref.unpack_smm(t)
    Lc = dists.chol(sigma)                                 # = L_k: the factor with a positive diagonal is unique
    eye = torch.eye(Ld, dtype=dtype).expand(K, Ld, Ld)
    W = torch.linalg.solve_triangular(Lc, eye, upper=False)
    elp = dists.dir_expected_log_pi(al if mut == 'dirichlet_plus1_dropped' else dists.dir_natural_to_standard(al))
    at_loc = dists.student_t_log_probability_per_samp(mu_t.detach().view(1, K, 1, Ld), mu_t, sigma, dofs)[0, :, 0]
    if mut == 'kappa_logdiag_sign':
        at_loc = at_loc + dists.logdet(sigma)
    kappa = at_loc + elp
    out = dict(W=_mut_W(W.detach(), mut), kappa=kappa.detach())
    if g is not None:
        g_m, g_W, g_k = [torch.as_tensor(a).to(dtype) for a in g]
        kap = kappa.detach() if mut == 'smm_gkappa_term_dropped' else kappa
        gm, gL = torch.autograd.grad(_probe((mu_t, W, kap), (g_m, g_W, g_k)), t)
        out.update(g_mu=gm, g_Lraw=gL)
    return out


def partial_words(L):
    return 2 * (L + L * (L + 1) // 2 + 1)


def reduce_truth(partials, K, L, theta_side, mut=None):
    """fp64 column sums of the (nblk, K, 2 (L + TRI + 1)) partial rows [g_hk | g_P lower packed | g_bias | g_mk | g_W lower packed | g_kappa],
    unpacked as svae_bwd_reduce_kernel documents: g_P symmetric from the packed lower value, g_W lower with zeros above.  Returns (sums, the same
    sums of |p|): dicts of g_hk, g_P, g_bias [, g_mk, g_W, g_kappa]."""
    p = torch.as_tensor(partials).double()
    nblk = p.shape[0]
    TRI = L * (L + 1) // 2
    TH = L + TRI + 1
    assert tuple(p.shape) == (nblk, K, 2 * TH)
    if mut == 'reduce_row_left_out':
        p = p[:-1]
    ii, jj = torch.tril_indices(L, L)

    def unpack(tot, o, names, sym):
        M = torch.zeros(K, L, L, dtype=F64)
        M[:, ii, jj] = tot[:, o + L:o + L + TRI]
        if sym:
            M[:, jj, ii] = tot[:, o + L:o + L + TRI]
        return {names[0]: tot[:, o:o + L].clone(), names[1]: M, names[2]: tot[:, o + L + TRI].clone()}
    out = []
    for tot in (p.sum(0), p.abs().sum(0)):
        d = unpack(tot, 0, ('g_hk', 'g_P', 'g_bias'), True)
        if theta_side:
            d.update(unpack(tot, TH, ('g_mk', 'g_W', 'g_kappa'), mut == 'gW_symmetrised'))
        out.append(d)
    return out[0], out[1]


def reduce_bar(want, sabs, nblk):
    """per element: fp64 accumulation of nblk fp32 values in ANY order (<= nblk 2^-52 sum |p|, first order, with room) and one rounding to fp32"""
    return 2.0 ** -23 * want.abs() + nblk * 2.0 ** -52 * sabs


def cvi_truth(prior, theta, x_s, r, rho):
    """(theta*, theta after the convex step) - svae_estep_truth.cvi_truth: svae_ref.m_step + update_gmm_params, in the dtype of the inputs"""
    return E.cvi_truth(prior, theta, x_s, r, rho)


def rel(got, want):
    """max |got - want| relative to the largest |want|"""
    want = torch.as_tensor(want).detach().double().cpu()
    return float((torch.as_tensor(got).detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def floor_of(name):
    return GRAD_FLOOR if name.startswith('g_') else FLOORS[name]


def bar(name, t64, t32):
    """max(floor, 3 |oracle fp32 - oracle fp64|) relative to the tensor's largest entry - the clause of svae_estep_truth.bars: measured on the
    reference's own arithmetic, never on the kernel.  Returns (bar, the fp32 oracle's loss)."""
    o32 = rel(t32, t64)
    return max(floor_of(name), 3.0 * o32), o32


def bars(t64, t32, names=None):
    """{name: bar} and {name: oracle loss} over the tensors two truth dicts share"""
    names = [n for n in t64 if n != 'logpi'] if names is None else names
    b = {n: bar(n, t64[n], t32[n]) for n in names}
    return {n: v[0] for n, v in b.items()}, {n: v[1] for n, v in b.items()}


def upstream(K, L, rng):
    """(g_hk, g_P, g_bias) of a phi backward case, fp32-representable; g_P is a FULL non-symmetric matrix"""
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    return r32(rng.standard_normal((K, L))), r32(rng.standard_normal((K, L, L))), r32(rng.standard_normal(K))


def phi_pair(case, g):
    """(fp64 truth, fp32 oracle) of the recognition unpacking of a case"""
    return phi_truth(*case.phi, g=g), phi_truth(*case.phi, g=g, dtype=F32)


def theta_pair(case):
    return theta_truth(*case.theta), theta_truth(*case.theta, dtype=F32)


def smm_pair(case, g=None):
    return smm_theta_truth(*case.theta_t, g=g), smm_theta_truth(*case.theta_t, g=g, dtype=F32)


CVI_ROWS, CVI_RHO = 37, 0.17


def cvi_inputs(K, L, rng, N=CVI_ROWS):
    """(x_samples (N,L), r (N,K)) of a CVI case, fp32-representable"""
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    lg = rng.standard_normal((N, K)) * 2.0
    r = np.exp(lg - lg.max(1, keepdims=True))
    return r32(rng.standard_normal((N, L)) * 2.0), r32(r / r.sum(1, keepdims=True))


def cvi_pair(case, x_s, r, rho=CVI_RHO):
    """((theta*, theta) in fp64, the same from the fp32 oracle) with the prior of svae_ref.init_mm"""
    K, L = case.theta[2].shape
    out = []
    for dt in (F64, F32):
        prior = E.oracle_prior(K, L, dt)
        out.append(cvi_truth(prior, case.as_torch('theta', dt), torch.tensor(x_s, dtype=dt), torch.tensor(r, dtype=dt), rho))
    return out[0], out[1]


def cvi_bars(t64, t32):
    """[bar per tensor of theta*], [bar per tensor of theta]; and the fp32 oracle's losses in the same layout"""
    b = [[bar(n, a, c) for a, c in zip(x64, x32)] for n, x64, x32 in (('theta_star', t64[0], t32[0]), ('theta', t64[1], t32[1]))]
    return [[v[0] for v in row] for row in b], [[v[1] for v in row] for row in b]
