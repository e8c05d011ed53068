"""Variational mixture of Student-t (Archambeau & Verleysen 2007) - mirror of reference models/smm.py:25-245.
Same kernels as gmm.py with the scale variables u_nk: weights w = r*u, W_k = sum w (smm.py:30-50),
v_k without the +1 (smm.py:73-76), Cholesky log-det without guard (smm.py:99-110)."""
import math

import torch

from .. import _klinalg, _lib as L
from . import _mix


# ---- the individual update functions of reference smm.py:25-137 (API parity; m_step / e_step / inference are fused) ----
def update_Nk(r_nk):
    """reference smm.py:25-27 (eq. 34)."""
    from . import gmm
    return gmm.update_Nk(r_nk)


def update_Wk(ru_nk):
    """reference smm.py:30-32 (eq. 35)."""
    from . import gmm
    return gmm.update_Nk(ru_nk)


def update_xk(x, ru_nk, W_k, eps=1e-20):
    """reference smm.py:35-40 (eq. 32)."""
    from . import gmm
    _, sx, _ = gmm._centred_moments(x, ru_nk, W_k, None, eps)
    return (sx / (W_k.double()[:, None] + eps)).to(x.dtype)


def update_Sk(x, ru_nk, W_k, x_k, eps=1e-20):
    """reference smm.py:43-50 (eq. 33)."""
    from . import gmm
    sw, sx, sxx = gmm._centred_moments(x, ru_nk, W_k, x_k, eps)
    a = x_k.double()
    S = sxx - sx[:, :, None] * a[:, None, :] - a[:, :, None] * sx[:, None, :] + sw[:, None, None] * a[:, :, None] * a[:, None, :]
    return (S / (W_k.double()[:, None, None] + eps)).to(x.dtype)


def update_alphak(alpha_0, N_k):
    return alpha_0 + N_k                       # eq. 27, smm.py:53-55


def update_betak(beta_0, W_k):
    return beta_0 + W_k                        # eq. 28, smm.py:58-60


def update_mk(beta_0, m_0, W_k, x_k, beta_k):
    return (beta_0.reshape(-1, 1) * m_0 + W_k[:, None] * x_k) / beta_k[:, None]      # eq. 29, smm.py:63-71


def update_vk(v_0, N_k):
    return v_0 + N_k                           # eq. 30 (no +1 here), smm.py:73-76


def update_Ck(C_0, x_k, W_k, m_0, beta_0, beta_k, S_k):
    dx = x_k - m_0                             # eq. 31, smm.py:78-85
    w = (beta_0.reshape(-1) * W_k / beta_k)[:, None, None]
    return C_0 + W_k[:, None, None] * S_k + w * (dx[:, :, None] * dx[:, None, :])


def expct_mahalanobis_dist(x, beta_k, m_k, P_k, v_k):
    """reference smm.py:88-96."""
    from . import gmm
    return gmm._mahalanobis(x, beta_k, m_k, P_k, v_k)


def expct_log_det_prec(v_k, P_k):
    """reference smm.py:99-110: Cholesky log-det (no guard), digamma arguments without the +1."""
    P = P_k.double()
    D = P.shape[-1]
    ld = 2.0 * torch.log(torch.diagonal(_klinalg.cholesky(P), dim1=-2, dim2=-1)).sum(-1)
    i = torch.arange(D, dtype=torch.float64, device=P.device)
    sdg = torch.special.digamma(0.5 * (v_k.double()[:, None] + i[None, :])).sum(1)
    return (sdg + D * math.log(2.0) + ld).to(P_k.dtype)


def expct_log_pi(alpha_k):
    """reference smm.py:113-116."""
    return torch.special.digamma(alpha_k) - torch.special.digamma(alpha_k.sum())


def compute_rnk(expct_log_pi, expct_log_det_prec, expct_m_dist, kappa_k, D):
    """reference smm.py:119-128 (eq. 19)."""
    log_r = torch.lgamma((D + kappa_k) / 2.) - torch.lgamma(kappa_k / 2.) - (D / 2.) * torch.log(kappa_k * math.pi)
    log_r = log_r + expct_log_pi + 0.5 * expct_log_det_prec
    log_r = log_r - (0.5 * (D + kappa_k) * expct_m_dist - torch.log(kappa_k))
    return torch.exp(log_r - torch.logsumexp(log_r, dim=1, keepdim=True))


def compute_expct_unk(expct_m_dist, kappa_k, D):
    """reference smm.py:131-137 (eqs. 24-25)."""
    return 0.5 * (D + kappa_k) / (0.5 * (expct_m_dist + kappa_k))


def m_step(x, r_nk, u_nk, alpha_0, beta_0, m_0, C_0, v_0, name='m_step'):
    """reference smm.py:167-196.  Returns (alpha_k, beta_k, m_k, C_k, v_k, x_k, S_k)."""
    stats = _mix.raw_stats(x, r_nk, u_nk)
    kap = torch.ones(r_nk.shape[1], dtype=torch.float32, device=x.device)       # not used by the M-part
    p = _mix.finalize(stats, (alpha_0, beta_0, m_0, C_0, v_0), L.VMP_SMM, kappa=kap, want_pack=False)
    return p['alpha'], p['beta'], p['m'], p['C'], p['v'], p['xbar'], p['S']


def e_step(x, alpha_k, beta_k, m_k, P_k, v_k, kappa_k, name='e_step'):
    """reference smm.py:140-164.  Returns (r_nk, u_nk, exp(E log pi))."""
    pack, pi = _mix.pack_from_params(alpha_k, beta_k, m_k, P_k, v_k, L.VMP_SMM, kappa=kappa_k)
    r, u, _, _ = _mix.estep(x, pack, L.VMP_SMM)
    return r, u, pi


def heldout_logprob(x, alpha_k, beta_k, m_k, C_k, v_k, kappa_k, return_resp=False):
    """Plug-in log score of the Student-t mixture at the rows of x (N,D) from inference()'s theta
    (alpha_k, beta_k, m_k, C_k, v_k, kappa_k): the mixture of student_t.logprob_smm_mixture (student_t.py:42-56) + a
    log-sum-exp over k, with the point estimates
      mu_k = m_k,   sigma_k = C_k / v_k  (the inverse of the expected precision v_k P_k that smm.py:88-97 uses),
      nu_k = kappa_k,   log_w_k = log(alpha_k / sum alpha)
    (beta_k does not enter a plug-in score).  One streaming HIP pass (vmp_mix_score_pack_t + vmp_mix_score).  Returns
    (logp (N,), total) - total a 0-dim fp64 device tensor, sum_n logp_n, no host synchronisation - plus resp (N,K) when asked."""
    N, D, K = _mix._score_dims(x, m_k, 'heldout_logprob')
    for t, n, shp in ((alpha_k, 'alpha_k', (K,)), (beta_k, 'beta_k', (K,)), (C_k, 'C_k', (K, D, D)), (v_k, 'v_k', (K,)),
                      (kappa_k, 'kappa_k', (K,))):
        _mix._kd(t, n, shp)
    pack = _mix.score_pack_t(torch.log(alpha_k / alpha_k.sum()), m_k, C_k / v_k[:, None, None], kappa_k)
    logp, resp, total = _mix.mixture_score(x, pack, want_resp=return_resp)
    return (logp, total, resp) if return_resp else (logp, total)


def heldout_impute(x, miss, alpha_k, beta_k, m_k, C_k, v_k, kappa_k, return_resp=False):
    """Fill the missing entries of the rows of x (N,D) (miss (N,D), nonzero = missing) from the plug-in Student-t mixture of
    heldout_logprob (mu_k = m_k, sigma_k = C_k / v_k, nu_k = kappa_k, log_w_k = log(alpha_k / sum alpha)): the conditional mean of the
    missing block given the observed one, averaged with the responsibilities of the observed entries' marginal density (for
    kappa_k <= 1, where a Student-t has no mean, the conditional location).  One streaming HIP pass (vmp_mixture_impute_pack_t +
    vmp_mixture_impute).  Returns (x_filled (N,D), logp (N,)) plus resp (N,K) when asked."""
    N, D, K = _mix._impute_dims(x, miss, m_k, 'heldout_impute')
    for t, n, shp in ((alpha_k, 'alpha_k', (K,)), (beta_k, 'beta_k', (K,)), (C_k, 'C_k', (K, D, D)), (v_k, 'v_k', (K,)),
                      (kappa_k, 'kappa_k', (K,))):
        _mix._kd(t, n, shp)
    pack = _mix.impute_pack_t(torch.log(alpha_k / alpha_k.sum()), m_k, C_k / v_k[:, None, None], kappa_k)
    x_out, logp, resp, _ = _mix.mixture_impute(x, miss, pack, want_resp=return_resp)
    return (x_out, logp, resp) if return_resp else (x_out, logp)


def _plugin_pack(K, D, alpha_k, beta_k, m_k, C_k, v_k, kappa_k):
    """impute pack of the plug-in mixture of heldout_impute, its operands' shapes checked first"""
    for t, n, shp in ((alpha_k, 'alpha_k', (K,)), (beta_k, 'beta_k', (K,)), (m_k, 'm_k', (K, D)), (C_k, 'C_k', (K, D, D)),
                      (v_k, 'v_k', (K,)), (kappa_k, 'kappa_k', (K,))):
        _mix._kd(t, n, shp)
    return _mix.impute_pack_t(torch.log(alpha_k / alpha_k.sum()), m_k, C_k / v_k[:, None, None], kappa_k)


def heldout_sample(n, seed, alpha_k, beta_k, m_k, C_k, v_k, kappa_k, want_z=False):
    """n seeded rows (n,D) from the plug-in Student-t mixture of heldout_logprob (mu_k = m_k, sigma_k = C_k / v_k, nu_k = kappa_k,
    log_w_k = log(alpha_k / sum alpha)) in one streaming HIP pass (vmp_mixture_impute_pack_t + vmp_mixture_sample); with want_z
    also the (n,) int32 components.  Row i is a function of (seed, i) only."""
    if not torch.is_tensor(m_k) or m_k.dim() != 2:
        raise L.VmpError('heldout_sample: m_k must be (K,D)')
    pack = _plugin_pack(m_k.shape[0], m_k.shape[1], alpha_k, beta_k, m_k, C_k, v_k, kappa_k)
    x, z = _mix.mixture_draw(n, pack, seed, want_z=want_z)
    return (x, z) if want_z else x


def heldout_impute_draws(x, miss, draws, seed, alpha_k, beta_k, m_k, C_k, v_k, kappa_k, want_z=False):
    """Multiple imputation under the plug-in Student-t mixture of heldout_impute: `draws` completed copies (draws,N,D) of the rows of
    x (N,D) (miss (N,D), nonzero = missing), the missing entries drawn from p(x_m | x_o), where heldout_impute fills in the
    conditional location.  One streaming HIP pass (vmp_mixture_impute_pack_t + vmp_mixture_sample); with want_z also the (draws,N)
    int32 components."""
    N, D, K = _mix._impute_dims(x, miss, m_k, 'heldout_impute_draws')
    pack = _plugin_pack(K, D, alpha_k, beta_k, m_k, C_k, v_k, kappa_k)
    xd, z = _mix.mixture_sample(x, miss, pack, seed, draws=draws, want_z=want_z)
    return (xd, z) if want_z else xd


def inference(x, K, kappa_init, seed, name='inference', r_init=None, init='random'):
    """reference smm.py:199-245: as gmm.inference with u_nk initialised to ones and constant kappa (init='kmeans++' as there)."""
    _mix.check_init(init)
    N, D = x.shape
    if r_init is None and init == 'kmeans++':
        r_init = _mix.seeded_r_init(x, K, seed)
    if r_init is None:
        g = torch.Generator(device='cpu').manual_seed(int(seed))
        e = -torch.log(torch.rand(N, K, generator=g).clamp_min(1e-30))
        r_init = (e / e.sum(1, keepdim=True)).to(x.device)
    kappa = torch.full((K,), float(kappa_init), dtype=torch.float32, device=x.device)
    loop = _mix.VMPLoop(x, r_init, L.VMP_SMM, kappa=kappa)
    from .gmm import _Handle

    def step():
        return loop.step(want_logr=True)

    def theta():
        return loop.theta() + (kappa,)

    return (step, _Handle(lambda: loop.logr), _Handle(theta), _Handle(loop.aux))
