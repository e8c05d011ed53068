"""Variational mixture of Gaussians (Bishop, PRML 10.2) - mirror of reference models/gmm.py:25-269.

N-sized work (statistics over the data, responsibilities) runs in the HIP kernels of csrc/vmp_mix.hip;
K-sized updates are available both as the reference's individual ``update_*`` functions (torch) and fused
on the device (vmp_mix_finalize, used by m_step / inference).
"""
import torch

from .. import _klinalg, _lib as L
from . import _mix


# ---- K-sized posterior updates (reference gmm.py:25-81), torch --------------------------------------
def update_Nk(r_nk):
    """reference gmm.py:25-27: N_k = sum_n r_nk (N-sized reduction -> the HIP stats kernel, D=1 dummy data)."""
    ones = torch.ones(r_nk.shape[0], 1, dtype=torch.float32, device=r_nk.device)
    return _mix.raw_stats(ones, r_nk)[:, 0].to(r_nk.dtype)


def _centred_moments(x, w, W_k, a_k, eps):
    """sum_n w_nk x_n / (W_k + eps) and sum_n w_nk (x_n - a_k)(x_n - a_k)^T / (W_k + eps) from the raw moments of the HIP stats
    kernel (fp64: sxx - sx a^T - a sx^T + (sum w) a a^T); returns the un-normalised sums too."""
    st = _mix.raw_stats(x, w)                                   # (K, 2+D+D*D) fp64: [sum w | . | sum w x | sum w x x^T]
    D = x.shape[1]
    sw, sx, sxx = st[:, 0], st[:, 2:2 + D], st[:, 2 + D:].reshape(-1, D, D)
    return sw, sx, sxx


def update_xk(x, r_nk, N_k):
    """reference gmm.py:30-36 (Bishop 10.52): sum_n r_nk x_n / N_k, un-normalised where N_k == 0 (NaN fallback)."""
    _, sx, _ = _centred_moments(x, r_nk, N_k, None, 0.0)
    normed = sx / N_k.double()[:, None]
    return torch.where(torch.isnan(normed), sx, normed).to(x.dtype)


def update_Sk(x, r_nk, N_k, x_k):
    """reference gmm.py:39-46 (Bishop 10.53): sum_n r_nk (x_n - x_k)(x_n - x_k)^T / N_k with the same NaN fallback."""
    sw, sx, sxx = _centred_moments(x, r_nk, N_k, x_k, 0.0)
    a = x_k.double()
    S = sxx - sx[:, :, None] * a[:, None, :] - a[:, :, None] * sx[:, None, :] + sw[:, None, None] * a[:, :, None] * a[:, None, :]
    normed = S / N_k.double()[:, None, None]
    return torch.where(torch.isnan(normed), S, normed).to(x.dtype)


def update_alphak(alpha_0, N_k):
    return alpha_0 + N_k                       # Bishop 10.58, reference gmm.py:49-51


def update_betak(beta_0, N_k):
    return beta_0 + N_k                        # Bishop 10.60, reference gmm.py:54-56


def update_mk(beta_0, m_0, N_k, x_k, beta_k):
    b0 = beta_0.reshape(-1, 1)                 # Bishop 10.61, reference gmm.py:59-68
    return (b0 * m_0 + N_k[:, None] * x_k) / beta_k[:, None]


def update_Ck(C_0, x_k, N_k, m_0, beta_0, beta_k, S_k):
    dx = x_k - m_0                             # Bishop 10.62, reference gmm.py:71-76
    w = (beta_0.reshape(-1) * N_k / beta_k)[:, None, None]
    return C_0 + N_k[:, None, None] * S_k + w * (dx[:, :, None] * dx[:, None, :])


def update_vk(v_0, N_k):
    return v_0 + N_k + 1                       # Bishop 10.63 with the reference's +1, gmm.py:79-81


def compute_expct_log_det_prec(v_k, P_k):
    """reference gmm.py:117-131, including the det <= 1e-20 -> log det := 0 guard (K-sized, torch fp64)."""
    P = P_k.double()
    D = P.shape[-1]
    sign, lad = _klinalg.slogdet(P)
    thresh = torch.log(torch.tensor(1e-20, dtype=torch.float64, device=P.device))
    ld = torch.where((sign > 0) & (lad > thresh), lad, torch.zeros_like(lad))
    i = torch.arange(D, dtype=torch.float64, device=P.device)
    sdg = torch.special.digamma(0.5 * (v_k.double()[:, None] + 1.0 + i[None, :])).sum(1)
    return (sdg + D * torch.log(torch.tensor(2.0, dtype=torch.float64)).item() + ld).to(P_k.dtype)


def compute_log_pi(alpha_k):
    """reference gmm.py:134-138."""
    return torch.special.digamma(alpha_k) - torch.special.digamma(alpha_k.sum())


# ---- steps ---------------------------------------------------------------------------------------------
def m_step(x, r_nk, alpha_0, beta_0, m_0, C_0, v_0, name='m_step'):
    """reference gmm.py:201-227.  Returns (alpha_k, beta_k, m_k, C_k, v_k, x_k, S_k)."""
    stats = _mix.raw_stats(x, r_nk)
    p = _mix.finalize(stats, (alpha_0, beta_0, m_0, C_0, v_0), L.VMP_GMM, want_pack=False)
    return p['alpha'], p['beta'], p['m'], p['C'], p['v'], p['xbar'], p['S']


def e_step(x, alpha_k, beta_k, m_k, P_k, v_k, name='e_step'):
    """reference gmm.py:154-174.  Returns (r_nk, exp(E log pi))."""
    pack, pi = _mix.pack_from_params(alpha_k, beta_k, m_k, P_k, v_k, L.VMP_GMM)
    r, _, _, _ = _mix.estep(x, pack, L.VMP_GMM)
    return r, pi


def e_step_missing_data(x, alpha_k, beta_k, m_k, P_k, v_k, missing_data_mask, name='e_step_imp'):
    """reference gmm.py:177-198: entries flagged in the (N,D) mask are ignored in the Mahalanobis term."""
    pack, pi = _mix.pack_from_params(alpha_k, beta_k, m_k, P_k, v_k, L.VMP_GMM)
    r, _, _, _ = _mix.estep(x, pack, L.VMP_GMM, miss_mask=missing_data_mask)
    return r, pi


def _mahalanobis(x, beta_k, m_k, P_k, v_k, mask=None):
    x = L.dev_f32(x, 'x')
    N, D = x.shape
    K = m_k.shape[0]
    m, P, v, b = (L.dev_f32(m_k.detach().float(), 'm_k', (K, D)), L.dev_f32(P_k.detach().float(), 'P_k', (K, D, D)),
                  L.dev_f32(v_k.detach().float(), 'v_k', (K,)), L.dev_f32(beta_k.detach().float(), 'beta_k', (K,)))
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    out = torch.empty(N, K, dtype=torch.float32, device=x.device)
    L.check(L.lib().vmp_mix_mahalanobis(L.ptr(x), L.ptr(m), L.ptr(P), L.ptr(v), L.ptr(b), L.ptr(m8), N, D, K, L.ptr(out),
                                        L.stream()), 'vmp_mix_mahalanobis')
    return out


def compute_expct_mahalanobis_dist(x, beta_k, m_k, P_k, v_k):
    """reference gmm.py:84-94 (Bishop 10.64), stand-alone: (N,K).  Inside e_step / inference the distance never leaves
    the fused pass kernel."""
    return _mahalanobis(x, beta_k, m_k, P_k, v_k)


def compute_dev_missing_data(x, beta_k, m_k, P_k, v_k, missing_data_mask):
    """reference gmm.py:97-114: as above with the missing entries of (x - m_k) zeroed."""
    return _mahalanobis(x, beta_k, m_k, P_k, v_k, missing_data_mask)


def compute_rnk(expct_log_pi, expct_log_det_cov, expct_dev):
    """reference gmm.py:141-151 (Bishop 10.49): max-shifted softmax over k of E log pi + 1/2 E log det - 1/2 E dev."""
    return torch.softmax(expct_log_pi + 0.5 * expct_log_det_cov - 0.5 * expct_dev, dim=1)


def predictive_logprob(x, alpha_k, beta_k, m_k, C_k, v_k, return_resp=False):
    """Log posterior predictive density of the variational GMM (Bishop, PRML 10.81-10.82) at the rows of x (N,D), from the NIW
    posterior (alpha_k, beta_k, m_k, C_k, v_k) that inference()'s theta handle returns (C_k is the inverse scale, gmm.py:260):
    a mixture of Student-t densities with nu' = v_k + 1 - D degrees of freedom, evaluated in one streaming HIP pass
    (vmp_mix_score_pack_niw + vmp_mix_score).  Returns (logp (N,), total) - total a 0-dim fp64 DEVICE tensor holding
    sum_n logp_n (deterministic; no host synchronisation) - plus resp (N,K), the predictive responsibilities, when asked."""
    _mix._score_dims(x, m_k, 'predictive_logprob')
    pack = _mix.score_pack_niw(alpha_k, beta_k, m_k, C_k, v_k)
    logp, resp, total = _mix.mixture_score(x, pack, want_resp=return_resp)
    return (logp, total, resp) if return_resp else (logp, total)


def lower_bound(x, alpha_k, beta_k, m_k, C_k, v_k, miss=None, prior=None, weights=None):
    """The variational lower bound (free energy, nats) of the NIW posterior (alpha_k, beta_k, m_k, C_k, v_k) that inference()'s theta
    handle returns, on the rows of x (N,D): what the iteration optimises, to judge convergence without held-out rows and to compare
    fits of the same data (another K, seed or init).  miss (N,D), nonzero = missing, for the theta of inference_missing(); prior
    defaults to the one inference() hard-codes.  Two K-sized launches (vmp_mixture_fit_pack, vmp_mixture_bound_terms) and one
    streaming HIP pass over x with its one-wave sum (vmp_mixture_bound_pass).  Returns a 0-dim fp64 DEVICE tensor (deterministic; no host synchronisation).
    weights (N,) fp32 >= 0 on x's device, for the theta of inference_weighted(): row n counts w_n times in the data term, a row of
    weight 0 not at all (the bound-only form of vmp_mixture_wfit_pass); weights=None is the unweighted pass, unchanged."""
    return _mix.lower_bound(x, (alpha_k, beta_k, m_k, C_k, v_k), prior=prior, miss=miss, weights=weights)


def predictive_impute(x, miss, alpha_k, beta_k, m_k, C_k, v_k, return_resp=False):
    """Fill the missing entries of the rows of x (N,D) - miss (N,D), nonzero = missing, the convention of missing_data_mask - from
    the posterior predictive of the variational GMM (the Student-t mixture predictive_logprob scores): each missing block gets
    sum_k r_nk E[x_m | x_o, k] with r_nk the responsibilities that follow from the MARGINAL density of the observed entries (unlike
    e_step_missing_data, which zeroes the missing differences inside the full precision).  One streaming HIP pass
    (vmp_mixture_impute_pack_niw + vmp_mixture_impute).  Returns (x_filled (N,D), logp (N,)) - logp the marginal log density of the
    observed entries - plus resp (N,K) when asked.  What the missing slots of x hold is never read into arithmetic."""
    _mix._impute_dims(x, miss, m_k, 'predictive_impute')
    pack = _mix.impute_pack_niw(alpha_k, beta_k, m_k, C_k, v_k)
    x_out, logp, resp, _ = _mix.mixture_impute(x, miss, pack, want_resp=return_resp)
    return (x_out, logp, resp) if return_resp else (x_out, logp)


def predictive_sample(n, seed, alpha_k, beta_k, m_k, C_k, v_k, want_z=False):
    """n seeded rows (n,D) from the posterior predictive of the variational GMM (the Student-t mixture predictive_logprob scores), in
    one streaming HIP pass (vmp_mixture_impute_pack_niw + vmp_mixture_sample); with want_z also the (n,) int32 components.  Row i
    is a function of (seed, i) only."""
    pack = _mix.impute_pack_niw(alpha_k, beta_k, m_k, C_k, v_k)
    x, z = _mix.mixture_draw(n, pack, seed, want_z=want_z)
    return (x, z) if want_z else x


def predictive_impute_draws(x, miss, draws, seed, alpha_k, beta_k, m_k, C_k, v_k, want_z=False):
    """Multiple imputation: `draws` completed copies (draws,N,D) of the rows of x (N,D) - miss (N,D), nonzero = missing - with the
    missing entries drawn from p(x_m | x_o) under the posterior predictive of the variational GMM, where predictive_impute fills in
    its mean.  One streaming HIP pass (vmp_mixture_impute_pack_niw + vmp_mixture_sample); with want_z also the (draws,N) int32
    components.  What the missing slots of x hold is never read into arithmetic."""
    _mix._impute_dims(x, miss, m_k, 'predictive_impute_draws')
    pack = _mix.impute_pack_niw(alpha_k, beta_k, m_k, C_k, v_k)
    xd, z = _mix.mixture_sample(x, miss, pack, seed, draws=draws, want_z=want_z)
    return (xd, z) if want_z else xd


class _Handle(object):
    """Stand-in for a TF fetch: call it to get the current value."""

    def __init__(self, fn):
        self._fn = fn

    def __call__(self):
        return self._fn()


def _dirichlet_init(N, K, seed, device):
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    e = -torch.log(torch.rand(N, K, generator=g).clamp_min(1e-30))
    return (e / e.sum(1, keepdim=True)).to(device)


def inference_missing(x, miss, K, seed, name='inference_missing', r_init=None, init='random'):
    """inference() on partly observed rows: miss (N,D), nonzero = missing, on x's device; what the missing slots of x hold is never
    read into arithmetic.  The missing entries are latent variables of the variational posterior, q(z_n, x_n,m) = q(z_n) q(x_n,m | z_n):
    every iteration is the NIW update of inference() on the moments of the completed rows (conditional means and covariances) and an
    E-step on the marginal of the observed entries, in one streaming HIP pass (csrc/vmp_missfit.hip) - unlike e_step_missing_data,
    which zeroes the missing differences inside the full precision and cannot feed an M-step.  Returns (step, log_r_nk, theta,
    (x_k, S_k, pi), x_filled): inference()'s four, and a handle for x with its missing entries replaced by sum_k r_nk E[x_m | x_o, k].
    init='kmeans++': r_init comes from _mix.seed_centers / seed_assign on the observed entries, as in inference()."""
    _mix.check_init(init)
    N, D = x.shape
    if r_init is None and init == 'kmeans++':
        _mix.VMPLoop._check_miss(x, miss, L.VMP_GMM, False)
        r_init = _mix.seeded_r_init(x, K, seed, miss=miss)
    if r_init is None:
        r_init = _dirichlet_init(N, K, seed, x.device)
    loop = _mix.VMPLoop(x, r_init, L.VMP_GMM, miss=miss)

    def step():
        return loop.step(want_logr=True)

    return (step, _Handle(lambda: loop.logr), _Handle(loop.theta), _Handle(loop.aux), _Handle(loop.filled))


def inference_weighted(x, weights, K, seed, miss=None, r_init=None, init='random'):
    """inference() on weighted rows: weights (N,) fp32 on x's device, finite, >= 0, not all zero - row n counts as w_n identical rows
    (counts of binned or de-duplicated data, coresets, importance weights; a 0/1 vector is a fold over the same resident x, and a row
    of weight 0 reaches nothing the fit adds up, whatever it holds).  A weight does not enter a row's own responsibilities; it scales
    the row's share of the moments and of the lower bound, in one streaming HIP pass (csrc/vmp_wfit.hip).  miss (N,D), nonzero =
    missing, as in inference_missing().  Returns (step, log_r_nk, theta, (x_k, S_k, pi), x_filled) as inference_missing() does;
    x_filled() is for a fit with a mask.  init='kmeans++': r_init from _mix.seed_centers / seed_assign; that seeding is unweighted."""
    _mix.check_init(init)
    N, D = x.shape
    if r_init is None:
        _mix.VMPLoop._check_weighted(x, weights, L.VMP_GMM, False)                   # before anything is seeded
        if miss is not None:
            _mix.VMPLoop._check_miss(x, miss, L.VMP_GMM, False)
        r_init = _mix.seeded_r_init(x, K, seed, miss=miss) if init == 'kmeans++' else _dirichlet_init(N, K, seed, x.device)
    loop = _mix.VMPLoop(x, r_init, L.VMP_GMM, miss=miss, weights=weights)

    def step():
        return loop.step(want_logr=True)

    return (step, _Handle(lambda: loop.logr), _Handle(loop.theta), _Handle(loop.aux), _Handle(loop.filled))


def inference(x, K, seed, name='inference', r_init=None, init='random'):
    """reference gmm.py:230-269.  Returns (step, log_r_nk, theta, (x_k, S_k, pi)) where `step()` executes one
    VMP iteration (M-step, E-step, assign) and returns the new r_nk; the other three are handles that are
    CALLED to fetch the values of the last executed iteration.  `r_init` replaces the TF-RNG Dirichlet(1)
    draw of gmm.py:246-249 (default: torch Dirichlet(1) with `seed`).  init='kmeans++' (when no r_init is given): r_init is built on
    the device instead - k-means++ centres drawn with `seed` and the one-hot responsibilities of the nearest centre
    (_mix.seed_centers / seed_assign): no host random numbers, no copy, and a start that already separates the clusters."""
    _mix.check_init(init)
    N, D = x.shape
    if r_init is None and init == 'kmeans++':
        r_init = _mix.seeded_r_init(x, K, seed)
    if r_init is None:
        g = torch.Generator(device='cpu').manual_seed(int(seed))
        e = -torch.log(torch.rand(N, K, generator=g).clamp_min(1e-30))
        r_init = (e / e.sum(1, keepdim=True)).to(x.device)
    loop = _mix.VMPLoop(x, r_init, L.VMP_GMM)

    def step():
        return loop.step(want_logr=True)

    return (step, _Handle(lambda: loop.logr), _Handle(loop.theta), _Handle(loop.aux))


def inference_diag(x, K, seed, iterations=1, r_init=None, prior=None, init='random'):
    """inference() for the diagonal-covariance Gaussian mixture on wide rows: x (N, D <= 64), one precision per component and
    coordinate (include/vmp_hip.h "Diagonal-covariance mixture fitting on wide rows"; csrc/vmp_diagfit.hip).  Returns (step, log_r_nk,
    theta, (x_k, S_k, pi)) as inference() does: `step()` runs `iterations` VMP iterations enqueued by one call and returns the new
    r_nk; theta() = (alpha_k, beta_k, m_k, a_k, b_k); S_k (K,D) holds the per-coordinate variances.  init='random': a host-side
    Dirichlet(1) draw with `seed`; an explicit r_init wins.  prior = (alpha_0, beta_0, m_0, a_0, b_0), default
    _mix.default_diag_prior.  init='kmeans++' (when no r_init is given): the start of _mix.DiagLoop.from_seed(x, K, seed) - k-means++
    centres and their nearest-centre responsibilities, built on the device by the kernels of csrc/vmp_diagseed.hip, so x must be on a
    GPU for it; 'random' is the only start that is drawn on the host."""
    _mix.check_init(init)
    iterations = int(iterations)
    if iterations < 1:
        raise L.VmpError('inference_diag: iterations must be >= 1')
    if not torch.is_tensor(x) or x.dim() != 2:
        raise L.VmpError('inference_diag: x must be (N,D)')
    if r_init is None and init == 'kmeans++':
        if not x.is_cuda:
            raise L.VmpError("inference_diag: init='kmeans++' seeds in HIP kernels on x's device and x is on %s (no CPU fallback) - "
                             "only 'random' is drawn on the host" % (x.device,))
        loop = _mix.DiagLoop.from_seed(x, K, seed, prior=prior)
    else:
        loop = _mix.DiagLoop(x, _dirichlet_init(x.shape[0], K, seed, x.device) if r_init is None else r_init, prior=prior)

    def step():
        if iterations > 1:
            loop.run(iterations - 1)
        return loop.step(want_logr=True)

    return (step, _Handle(lambda: loop.logr), _Handle(loop.theta), _Handle(loop.aux))


def _diag_fit_handles(loop):
    def step():
        return loop.step(want_logr=True)

    def filled():
        return loop.filled()

    return (step, _Handle(lambda: loop.logr), _Handle(loop.theta), _Handle(loop.aux), _Handle(filled))


def inference_diag_missing(x, miss, K, seed, r_init=None, prior=None):
    """inference_diag() on partly observed rows: miss (N,D), nonzero = missing, on x's device; what the missing slots of x hold is
    never read into arithmetic.  The missing entries are latent variables with a one-dimensional Gaussian q(x_nd | z_n) each, so the
    posterior keeps its shape and every iteration is the finalize of inference_diag() on the moments of the completed rows and an
    E-step on the observed entries, in one streaming HIP pass (csrc/vmp_diagmfit.hip; _mix.DiagFitLoop).  Returns (step, log_r_nk,
    theta, (x_k, S_k, pi), x_filled): inference_diag()'s four and a handle for x with its missing entries replaced by sum_k r_nk
    m_kd.  The start is a host-side Dirichlet(1) draw with `seed` unless r_init is given; k-means++ on masked wide rows is not built."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise L.VmpError('inference_diag_missing: x must be (N,D)')
    if miss is None:
        raise L.VmpError('inference_diag_missing: needs the missing-data mask (complete rows: inference_diag)')
    loop = _mix.DiagFitLoop(x, _dirichlet_init(x.shape[0], K, seed, x.device) if r_init is None else r_init, miss=miss, prior=prior)
    return _diag_fit_handles(loop)


def inference_diag_weighted(x, weights, K, seed, miss=None, r_init=None, prior=None, init='random'):
    """inference_diag() on weighted rows: weights (N,) fp32 on x's device, finite, >= 0, not all zero - row n counts as w_n identical
    rows (binned counts, coresets, a 0/1 fold over the same resident x; a row of weight 0 reaches nothing the fit adds up, whatever
    it holds).  A weight does not enter a row's own responsibilities.  miss (N,D) as in inference_diag_missing().  Returns (step,
    log_r_nk, theta, (x_k, S_k, pi), x_filled); x_filled() is for a fit with a mask.  init='kmeans++' (no r_init, no mask): the
    unweighted seeded start of _mix.DiagFitLoop.from_seed."""
    _mix.check_init(init)
    if not torch.is_tensor(x) or x.dim() != 2:
        raise L.VmpError('inference_diag_weighted: x must be (N,D)')
    if weights is None:
        raise L.VmpError('inference_diag_weighted: needs the weights (unweighted rows: inference_diag / inference_diag_missing)')
    if r_init is None and init == 'kmeans++':
        loop = _mix.DiagFitLoop.from_seed(x, K, seed, weights=weights, prior=prior, miss=miss)
    else:
        loop = _mix.DiagFitLoop(x, _dirichlet_init(x.shape[0], K, seed, x.device) if r_init is None else r_init, miss=miss,
                                weights=weights, prior=prior)
    return _diag_fit_handles(loop)


def lower_bound_diag(x, alpha_k, beta_k, m_k, a_k, b_k, prior=None, miss=None, weights=None):
    """The variational lower bound (nats) of the diagonal posterior that inference_diag()'s theta handle returns, on the rows of x:
    two K-sized launches and the bound-only form of the streaming pass.  Returns a 0-dim fp64 DEVICE tensor (deterministic; no host
    synchronisation).  miss (N,D), nonzero = missing, and / or weights (N,) fp32 >= 0, for the theta of inference_diag_missing() /
    inference_diag_weighted(): the bound those fits optimise (bound-only form of vmp_mixture_diag_mfit_pass); without them the call
    is unchanged."""
    return _mix.diag_lower_bound(x, (alpha_k, beta_k, m_k, a_k, b_k), prior=prior, miss=miss, weights=weights)


def predictive_logprob_diag(x, alpha_k, beta_k, m_k, a_k, b_k, miss=None):
    """Log posterior predictive density of the diagonal-covariance mixture at the rows of x (N, D <= 64), from the posterior
    (alpha_k, beta_k, m_k, a_k, b_k) that inference_diag()'s theta handle returns: given the component a product of one-dimensional
    Student-t densities with 2 a_k degrees of freedom (include/vmp_hip.h "Diagonal-covariance mixture: scoring and filling wide
    rows").  miss (N,D), nonzero = missing: the density of the observed entries.  One K-sized launch and one streaming HIP pass
    (csrc/vmp_diagscore.hip).  Returns logp (N,); no host synchronisation."""
    return _mix.diag_predictive_logprob(x, (alpha_k, beta_k, m_k, a_k, b_k), miss=miss)


def predictive_impute_diag(x, miss, alpha_k, beta_k, m_k, a_k, b_k):
    """Fill the missing entries of the rows of x (N, D <= 64) - miss (N,D), nonzero = missing - from the posterior predictive of the
    diagonal-covariance mixture: each gets sum_k r_nk m_kd with r_nk the responsibilities that follow from the density of the observed
    entries.  Returns (x_filled (N,D), logp (N,)); what the missing slots of x hold is never read into arithmetic."""
    return _mix.diag_predictive_impute(x, miss, (alpha_k, beta_k, m_k, a_k, b_k))
