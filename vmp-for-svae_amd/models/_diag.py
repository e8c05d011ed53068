"""Host side of the diagonal-covariance Gaussian mixture on wide rows (csrc/vmp_diagfit.hip; include/vmp_hip.h "Diagonal-covariance
mixture fitting on wide rows"): thin wrappers over the vmp_mixture_diag_* C ABI and the loop that drives them.  D up to
_lib.DIAG_MAX_D = 64, K up to _lib.MAX_K.  theta = (alpha (K), beta (K), m (K,D), a (K), b (K,D)); a prior has the same five."""
import torch

from .. import _lib as L

NAMES = ('alpha', 'beta', 'm', 'a', 'b')
_POST = NAMES + ('xbar', 'S', 'pi')          # the outputs of the finalize, in the order of the C ABI


def _check_dk(D, K):
    if not (1 <= D <= L.DIAG_MAX_D):
        raise L.VmpError('D=%d outside the compiled range 1..%d of the diagonal-covariance mixture' % (D, L.DIAG_MAX_D))
    if not (1 <= K <= L.MAX_K):
        raise L.VmpError('K=%d outside the compiled range 1..%d' % (K, L.MAX_K))


def _x_dims(x, what):
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1:
        raise L.VmpError('%s: x must be (N >= 1, D), got %s' % (what, tuple(x.shape) if torch.is_tensor(x) else type(x)))
    return x.shape


def _shapes(K, D):
    return ((K,), (K,), (K, D), (K,), (K, D))


def _five(ops, K, D, what, suffix=''):
    """the five tensors of a posterior or a prior: shapes refused BEFORE the library or a device is touched"""
    if len(ops) != 5:
        raise L.VmpError('%s: expected (alpha, beta, m, a, b)' % what)
    for t, n, shp in zip(ops, NAMES, _shapes(K, D)):
        if not torch.is_tensor(t) or tuple(t.shape) != shp:
            raise L.VmpError('%s: %s%s has shape %s, expected %s' % (what, n, suffix, tuple(t.shape) if torch.is_tensor(t) else type(t), shp))
    return ops


def _dev5(ops, dev, suffix=''):
    return [L.dev_f32(t.detach().to(dev, torch.float32), n + suffix) for t, n in zip(ops, NAMES)]


def _miss_dims(miss, N, D, what):
    if not torch.is_tensor(miss) or tuple(miss.shape) != (N, D):
        raise L.VmpError('%s: the missing-data mask must be (%d,%d), got %s' % (what, N, D, tuple(miss.shape) if torch.is_tensor(miss) else type(miss)))


def observed_column_means(x, miss=None, weights=None):
    """((D,) fp64 weighted means of the observed entries of the rows of positive weight - 0 for a column without one -, live (N,D)
    bool or None): what a missing slot or a row of weight 0 holds (NaN included) is selected out, never multiplied.  Torch plumbing."""
    if miss is None and weights is None:
        return x.double().mean(0), None
    N, D = x.shape
    live = torch.ones(N, D, dtype=torch.bool, device=x.device) if miss is None else (miss == 0)
    w = torch.ones(N, dtype=torch.float64, device=x.device) if weights is None else weights.double()
    live = live & (w > 0)[:, None]
    num = (torch.where(live, x.double(), torch.zeros((), dtype=torch.float64, device=x.device)) * w[:, None]).sum(0)
    den = (live.double() * w[:, None]).sum(0)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num)), live


def default_diag_prior(x, K, miss=None, weights=None):
    """alpha_0 = 0.05 / K, beta_0 = 0.5, m_0 = the column means of x, a_0 = 1, b_0 = 1 - on x's device.  With miss (N,D; nonzero =
    missing) and / or weights (N,): the weighted means of the observed entries (observed_column_means)."""
    N, D = _x_dims(x, 'default_diag_prior')
    f32 = dict(dtype=torch.float32, device=x.device)
    if miss is not None:
        _miss_dims(miss, N, D, 'default_diag_prior')
    mean = observed_column_means(x, miss, weights)[0].to(torch.float32)
    return (torch.full((K,), 0.05 / K, **f32), torch.full((K,), 0.5, **f32), mean[None, :].expand(K, D).contiguous(),
            torch.ones(K, **f32), torch.ones(K, D, **f32))


def diag_pack(alpha, beta, m, a, b):
    """The E-step pack (K, 2 D + 1) fp32 = [ m | lbar = a / b | c ] of a posterior (vmp_mixture_diag_pack); fp64 inside, rounded
    once.  A component with a non-positive b, a or beta gets a NaN row.  One K-block launch, no host synchronisation."""
    if not torch.is_tensor(m) or m.dim() != 2:
        raise L.VmpError('diag_pack: m must be (K,D)')
    K, D = m.shape
    _check_dk(D, K)
    theta = _dev5(_five((alpha, beta, m, a, b), K, D, 'diag_pack'), m.device)
    pack = torch.empty(K, L.lib().vmp_mixture_diag_pack_words(D), dtype=torch.float32, device=m.device)
    L.check(L.lib().vmp_mixture_diag_pack(D, K, *[L.ptr(t) for t in theta], L.ptr(pack), L.stream()), 'vmp_mixture_diag_pack')
    return pack


def _pass_dims(x, pack, what):
    N, D = _x_dims(x, what)
    if not torch.is_tensor(pack) or pack.dim() != 2 or pack.shape[1] != 2 * D + 1:
        raise L.VmpError('%s: no diagonal pack for D=%d (shape %s, expected (K,%d): diag_pack)'
                         % (what, D, tuple(pack.shape) if torch.is_tensor(pack) else type(pack), 2 * D + 1))
    K = pack.shape[0]
    _check_dk(D, K)
    return N, D, K


def mixture_diag_pass(x, pack, r_in=None, want_r=True, want_logr=False, want_stats=True, want_bound=False):
    """One streaming pass (vmp_mixture_diag_pass) over the rows of x (N,D) under a diagonal pack: (r (N,K), logr (N,K), stats
    (K, 1 + 2 D) fp64 = [Nk | sx | sxx], bound 0-dim fp64 = the data term of the lower bound); outputs that are not wanted are None.
    want_r=False is the fast form: the pass then moves x alone, and stats are still the moments of the responsibilities it computes.
    r_in (N,K): the moments of the caller's responsibilities instead (stats only).  stats and bound are the same bits from run to
    run and for every set of outputs.  No host synchronisation."""
    what = 'mixture_diag_pass'
    N, D, K = _pass_dims(x, pack, what)
    if not (want_r or want_logr or want_stats or want_bound):
        raise L.VmpError('%s: no output requested' % what)
    if want_logr and not want_r:
        raise L.VmpError('%s: want_logr needs want_r' % what)
    if r_in is not None:
        if not torch.is_tensor(r_in) or tuple(r_in.shape) != (N, K):
            raise L.VmpError('%s: r_in has shape %s, expected %s' % (what, tuple(r_in.shape) if torch.is_tensor(r_in) else type(r_in), (N, K)))
        if want_r or want_logr or want_bound:
            raise L.VmpError('%s: r_in gives the moments only (want_r, want_logr and want_bound must be False)' % what)
    x = L.dev_f32(x, 'x')
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, 2 * D + 1))
    if pack.device != dev:
        raise L.VmpError('pack is on %s, x on %s' % (pack.device, dev))
    if r_in is not None:
        r_in = L.dev_f32(r_in, 'r_in', (N, K))
    f32 = dict(dtype=torch.float32, device=dev)
    r = torch.empty(N, K, **f32) if want_r else None
    logr = torch.empty(N, K, **f32) if want_logr else None
    stats = torch.empty(K, 1 + 2 * D, dtype=torch.float64, device=dev) if want_stats else None
    bound = torch.empty((), dtype=torch.float64, device=dev) if want_bound else None
    nb = L.lib().vmp_mixture_diag_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_diag_pass(L.ptr(x), N, D, K, L.ptr(pack), L.ptr(r_in), L.ptr(r), L.ptr(logr), L.ptr(stats), L.ptr(bound),
                                          L.ptr(ws), nb, L.stream()), 'vmp_mixture_diag_pass')
    return r, logr, stats, bound


def _stats_dims(stats, what):
    if not torch.is_tensor(stats) or stats.dim() != 2 or stats.shape[1] < 3 or stats.shape[1] % 2 != 1:
        raise L.VmpError('%s: stats must be (K, 1 + 2 D) fp64' % what)
    K, D = stats.shape[0], (stats.shape[1] - 1) // 2
    _check_dk(D, K)
    return K, D


def _post_buffers(K, D, dev):
    f32 = dict(dtype=torch.float32, device=dev)
    return dict(alpha=torch.empty(K, **f32), beta=torch.empty(K, **f32), m=torch.empty(K, D, **f32), a=torch.empty(K, **f32),
                b=torch.empty(K, D, **f32), xbar=torch.empty(K, D, **f32), S=torch.empty(K, D, **f32), pi=torch.empty(K, **f32))


def diag_finalize(stats, prior):
    """Posterior dict(alpha, beta, m, a, b, xbar, S, pi) from raw stats (K, 1 + 2 D) fp64 and a prior (vmp_mixture_diag_finalize)."""
    K, D = _stats_dims(stats, 'diag_finalize')
    _five(prior, K, D, 'diag_finalize', '_0')
    if stats.dtype != torch.float64:
        raise L.VmpError('diag_finalize: stats must be float64 (got %s)' % stats.dtype)
    if not stats.is_cuda:
        raise L.VmpError('stats is on %s: the diagonal mixture only runs in HIP kernels on a GPU (no CPU fallback)' % stats.device)
    dev = stats.device
    prior = _dev5(prior, dev, '_0')
    out = _post_buffers(K, D, dev)
    L.check(L.lib().vmp_mixture_diag_finalize(L.ptr(stats.contiguous()), D, K, *[L.ptr(t) for t in prior],
                                              *[L.ptr(out[n]) for n in _POST], L.stream()), 'vmp_mixture_diag_finalize')
    return out


def diag_bound_terms(prior, theta):
    """(2 + K,) fp64 device tensor [ KL(q(pi) || p(pi)) | sum_kd KL(q(mu, lambda)_kd || p) | the K per-component sums ]
    (vmp_mixture_diag_bound_terms); fp64 inside, the sums in d and k order.  One launch, no host synchronisation."""
    if len(theta) != 5 or not torch.is_tensor(theta[2]) or theta[2].dim() != 2:
        raise L.VmpError('diag_bound_terms: theta is (alpha, beta, m (K,D), a, b)')
    K, D = theta[2].shape
    _five(theta, K, D, 'diag_bound_terms')
    _five(prior, K, D, 'diag_bound_terms', '_0')
    _check_dk(D, K)
    dev = theta[2].device
    theta, prior = _dev5(theta, dev), _dev5(prior, dev, '_0')
    out = torch.empty(2 + K, dtype=torch.float64, device=dev)
    L.check(L.lib().vmp_mixture_diag_bound_terms(D, K, *[L.ptr(t) for t in prior], *[L.ptr(t) for t in theta], L.ptr(out), L.stream()),
            'vmp_mixture_diag_bound_terms')
    return out


def diag_lower_bound(x, theta, prior=None, miss=None, weights=None):
    """The variational lower bound of the diagonal posterior theta on the rows of x: a 0-dim fp64 device tensor, data - kl_pi -
    sum_kd kl_ng_kd, with q(z) at its optimum for theta.  Pack, the bound-only pass, the terms, one subtraction: no host
    synchronisation.  miss (N,D; nonzero = missing) and / or weights (N,) fp32 >= 0: the bound of a DiagFitLoop fit (q(x_missing | z)
    at its optimum too), through the bound-only form of mixture_diag_mfit_pass; without them the call is what it was."""
    if miss is not None or weights is not None:
        return _mfit_lower_bound(x, theta, prior, miss, weights)
    N, D = _x_dims(x, 'lower_bound_diag')
    if len(theta) != 5 or not torch.is_tensor(theta[2]) or theta[2].dim() != 2:
        raise L.VmpError('lower_bound_diag: theta is (alpha, beta, m (K,D), a, b)')
    K = theta[2].shape[0]
    _five(theta, K, D, 'lower_bound_diag')
    _check_dk(D, K)
    prior = default_diag_prior(x, K) if prior is None else _five(prior, K, D, 'lower_bound_diag', '_0')
    x = L.dev_f32(x, 'x')
    terms = diag_bound_terms(prior, theta)
    data = mixture_diag_pass(x, diag_pack(*theta), want_r=False, want_stats=False, want_bound=True)[3]
    return data - (terms[0] + terms[1])


def diag_score_pack(alpha, beta, m, a, b):
    """The score pack (K, 3 D + 3) fp32 = [ m | g | h | log w | a + 1/2 | c ] of a posterior (vmp_mixture_diag_score_pack; include/vmp_hip.h
    "Diagonal-covariance mixture: scoring and filling wide rows"); fp64 inside, rounded once.  A component with a non-positive alpha,
    beta, a or b gets a NaN row.  One K-block launch, no host synchronisation."""
    if not torch.is_tensor(m) or m.dim() != 2:
        raise L.VmpError('diag_score_pack: m must be (K,D)')
    K, D = m.shape
    _check_dk(D, K)
    theta = _dev5(_five((alpha, beta, m, a, b), K, D, 'diag_score_pack'), m.device)
    pack = torch.empty(K, L.lib().vmp_mixture_diag_score_pack_words(D), dtype=torch.float32, device=m.device)
    L.check(L.lib().vmp_mixture_diag_score_pack(D, K, *[L.ptr(t) for t in theta], L.ptr(pack), L.stream()), 'vmp_mixture_diag_score_pack')
    return pack


def _score_dims(x, pack, miss, what):
    """(N, D, K) of a scoring pass, refused BEFORE the library or a device is touched"""
    N, D = _x_dims(x, what)
    if x.dtype != torch.float32:
        raise L.VmpError('%s: x must be float32 (got %s)' % (what, x.dtype))
    if not torch.is_tensor(pack) or pack.dim() != 2 or pack.shape[1] != 3 * D + 3:
        raise L.VmpError('%s: no diagonal score pack for D=%d (shape %s, expected (K,%d): diag_score_pack)'
                         % (what, D, tuple(pack.shape) if torch.is_tensor(pack) else type(pack), 3 * D + 3))
    K = pack.shape[0]
    _check_dk(D, K)
    if miss is not None and (not torch.is_tensor(miss) or tuple(miss.shape) != (N, D)):
        raise L.VmpError('%s: the missing-data mask must be (%d,%d), got %s' % (what, N, D, tuple(miss.shape) if torch.is_tensor(miss) else type(miss)))
    return N, D, K


_mask_u8 = L.mask_u8


def mixture_diag_score(x, pack, miss=None, want_logp=True, want_resp=False, want_fill=False, want_sum=False, inplace=False):
    """One streaming pass (vmp_mixture_diag_score) over the rows of x (N,D) under a diagonal score pack, with an optional mask miss (N,D;
    nonzero / True = missing): (logp (N,), resp (N,K), x_filled (N,D), total 0-dim fp64 = sum_n logp_n); outputs that are not wanted
    are None.  logp is the log posterior predictive density of the observed entries; x_filled (needs miss) is x with its missing
    entries replaced by sum_k resp_k m_k, observed entries copied bit for bit; inplace=True writes into x itself (a contiguous fp32
    GPU tensor) and returns it.  What a missing slot of x holds is never read into arithmetic.  Every output has the same bits from
    run to run and for every set of outputs.  No host synchronisation."""
    what = 'mixture_diag_score'
    N, D, K = _score_dims(x, pack, miss, what)
    if not (want_logp or want_resp or want_fill or want_sum):
        raise L.VmpError('%s: no output requested' % what)
    if want_fill and miss is None:
        raise L.VmpError('%s: want_fill needs miss (without a mask there is nothing to fill)' % what)
    if inplace and not want_fill:
        raise L.VmpError('%s: inplace=True needs want_fill' % what)
    xin = x
    x = L.dev_f32(x, 'x')
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, 3 * D + 3))
    if pack.device != dev:
        raise L.VmpError('pack is on %s, x on %s' % (pack.device, dev))
    mask = None
    if miss is not None:
        if miss.device != dev:
            raise L.VmpError('the missing-data mask is on %s, x on %s' % (miss.device, dev))
        mask = _mask_u8(miss)
    x_out = None
    if want_fill:
        if inplace and x.data_ptr() != xin.data_ptr():
            raise L.VmpError('inplace=True needs a contiguous x')
        x_out = x if inplace else torch.empty_like(x)
    logp = torch.empty(N, dtype=torch.float32, device=dev) if want_logp else None
    resp = torch.empty(N, K, dtype=torch.float32, device=dev) if want_resp else None
    total, ws, nb = None, None, 0
    if want_sum:
        total = torch.empty((), dtype=torch.float64, device=dev)
        nb = L.lib().vmp_mixture_diag_score_workspace_bytes(N, D, K)
        ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_diag_score(L.ptr(x), L.ptr(mask), N, D, K, L.ptr(pack), L.ptr(logp), L.ptr(resp), L.ptr(x_out), L.ptr(total),
                                           L.ptr(ws), nb, L.stream()), 'vmp_mixture_diag_score')
    return logp, resp, (xin if (want_fill and inplace) else x_out), total


def _theta_dims(x, theta, what):
    N, D = _x_dims(x, what)
    if len(theta) != 5 or not torch.is_tensor(theta[2]) or theta[2].dim() != 2:
        raise L.VmpError('%s: theta is (alpha, beta, m (K,D), a, b)' % what)
    K = theta[2].shape[0]
    if theta[2].shape[1] != D:
        raise L.VmpError('%s: x has %d columns, m %d' % (what, D, theta[2].shape[1]))
    _check_dk(D, K)
    _five(theta, K, D, what)
    return N, D, K


def diag_predictive_logprob(x, theta, miss=None):
    """logp (N,) of the rows of x under the posterior predictive of the diagonal posterior theta (gmm.predictive_logprob_diag)"""
    N, D, K = _theta_dims(x, theta, 'predictive_logprob_diag')
    if miss is not None and (not torch.is_tensor(miss) or tuple(miss.shape) != (N, D)):
        raise L.VmpError('predictive_logprob_diag: the missing-data mask must be (%d,%d)' % (N, D))
    L.dev_f32(x, 'x')
    return mixture_diag_score(x, diag_score_pack(*theta), miss=miss)[0]


def diag_predictive_impute(x, miss, theta):
    """(x_filled (N,D), logp (N,)) of the partly observed rows of x under the diagonal posterior theta (gmm.predictive_impute_diag)"""
    N, D, K = _theta_dims(x, theta, 'predictive_impute_diag')
    if not torch.is_tensor(miss) or tuple(miss.shape) != (N, D):
        raise L.VmpError('predictive_impute_diag: the missing-data mask must be (%d,%d), got %s'
                         % (N, D, tuple(miss.shape) if torch.is_tensor(miss) else type(miss)))
    L.dev_f32(x, 'x')
    logp, _, x_out, _ = mixture_diag_score(x, diag_score_pack(*theta), miss=miss, want_fill=True)
    return x_out, logp


def nearest_center_r(x, centers, smooth=0.0):
    """r (N,K) fp32 of the nearest of centers (K,D) by squared distance (torch.cdist + argmin, ties to the lowest k) with the
    smoothing rule of _mix.seed_assign: r_nk = (1 - smooth) [k = z_n] + smooth / K.  Plumbing in torch, not a kernel."""
    smooth = float(smooth)
    if not 0.0 <= smooth < 1.0:
        raise L.VmpError('smooth must be in [0, 1) (got %r)' % smooth)
    N, D = _x_dims(x, 'from_centers')
    if not torch.is_tensor(centers) or centers.dim() != 2 or centers.shape[1] != D:
        raise L.VmpError('from_centers: centers has shape %s, expected (K,%d)' % (tuple(centers.shape) if torch.is_tensor(centers) else type(centers), D))
    if centers.device != x.device:
        raise L.VmpError('from_centers: centers is on %s, x on %s' % (centers.device, x.device))
    K = centers.shape[0]
    _check_dk(D, K)
    d2 = torch.cdist(x.double(), centers.double())
    # argmin does not promise the first of equal minima: the lowest k among them, explicitly
    k_idx = torch.arange(K, device=x.device)[None, :].expand(N, K)
    z = torch.where(d2 == d2.min(1, keepdim=True).values, k_idx, torch.full_like(k_idx, K)).min(1).values
    r = torch.full((N, K), smooth / K, dtype=torch.float32, device=x.device)
    r[torch.arange(N, device=x.device), z] = (1.0 - smooth) + smooth / K
    return r


def diag_seed_centers(x, K, seed, want_index=False, want_mind2=False):
    """K seeded k-means++ centres (D^2-seeding) from the complete rows of x (N, D <= 64) on the device (vmp_mixture_diag_seed_centers;
    include/vmp_hip.h "Diagonal-covariance mixture: seeded start on wide rows"): (centers (K,D), index (K,) int64 or None, mind2 (N,)
    or None) - the chosen rows and every row's squared distance to its nearest centre.  A pure function of (seed, row index, round),
    the stream and the rules of _mix.seed_centers: for D <= 8 the same rows.  K + 1 launches enqueued by one call, no host
    synchronisation."""
    K, seed = int(K), int(seed)
    if not 0 <= seed < 1 << 64:
        raise L.VmpError('seed must be in 0 .. 2^64 - 1 (got %d)' % seed)
    N, D = _x_dims(x, 'diag_seed_centers')
    _check_dk(D, K)
    x = L.dev_f32(x, 'x')
    dev = x.device
    centers = torch.empty(K, D, dtype=torch.float32, device=dev)
    index = torch.empty(K, dtype=torch.int64, device=dev) if want_index else None
    mind2 = torch.empty(N, dtype=torch.float32, device=dev) if want_mind2 else None
    nb = L.lib().vmp_mixture_diag_seed_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_diag_seed_centers(L.ptr(x), N, D, K, seed, L.ptr(centers), L.ptr(index), L.ptr(mind2), L.ptr(ws), nb,
                                                  L.stream()), 'vmp_mixture_diag_seed_centers')
    return centers, index, mind2


def diag_seed_assign(x, centers, smooth=0.0, want_z=False):
    """Responsibilities of the nearest centre on wide rows (vmp_mixture_diag_seed_assign): (r (N,K), z (N,) int32 or None) with z_n the
    nearest of centers (K,D) by the fp32 squared distance of diag_seed_centers (ties to the lowest k) and r_nk = (1 - smooth)
    [k = z_n] + smooth / K, 0 <= smooth < 1.  One streaming launch, no host synchronisation."""
    smooth = float(smooth)
    if not 0.0 <= smooth < 1.0:
        raise L.VmpError('smooth must be in [0, 1) (got %r)' % smooth)
    N, D = _x_dims(x, 'diag_seed_assign')
    if not torch.is_tensor(centers) or centers.dim() != 2 or centers.shape[1] != D:
        raise L.VmpError('diag_seed_assign: centers has shape %s, expected (K,%d)'
                         % (tuple(centers.shape) if torch.is_tensor(centers) else type(centers), D))
    if centers.device != x.device:
        raise L.VmpError('diag_seed_assign: centers is on %s, x on %s' % (centers.device, x.device))
    K = centers.shape[0]
    _check_dk(D, K)
    x = L.dev_f32(x, 'x')
    centers = L.dev_f32(centers, 'centers', (K, D))
    r = torch.empty(N, K, dtype=torch.float32, device=x.device)
    z = torch.empty(N, dtype=torch.int32, device=x.device) if want_z else None
    L.check(L.lib().vmp_mixture_diag_seed_assign(L.ptr(x), N, D, K, L.ptr(centers), smooth, L.ptr(r), L.ptr(z), L.stream()),
            'vmp_mixture_diag_seed_assign')
    return r, z


class DiagLoop(object):
    """The VMP iteration of the diagonal-covariance Gaussian mixture on x (N, D <= 64), started from responsibilities r_init (N,K):
    M-step from the moments of the current r (vmp_mixture_diag_finalize), the E-step pack, and one streaming pass that computes the
    new r, its moments and the data term of the lower bound.  run(n) enqueues n iterations in one call and leaves r in the kernel
    (the pass then moves x alone); step() also writes r.  Both updates are exact coordinate ascent: lower_bound() never falls.
    from_seed(x, K, seed) starts the loop from the data alone: k-means++ centres and their nearest-centre responsibilities, both in
    kernels (csrc/vmp_diagseed.hip); from_centers() takes the caller's centres (torch plumbing).
    Rows the loop was not fitted on: heldout() (mean log predictive density), heldout_logprob() (per row, with the predictive
    responsibilities on request), fill() (conditional means of missing entries) and run_until() (stop on a validation set) - one
    streaming pass each (csrc/vmp_diagscore.hip).  Masked or weighted rows are refused here and fitted by the subclass DiagFitLoop.
    Out of scope, refused: the Student-t flavour, accurate=True; score / impute keep refusing and name heldout / heldout_logprob / fill, sampling (sample / impute_draws) is not
    built."""

    def __init__(self, x, r_init, prior=None, miss=None, weights=None, flavour=L.VMP_GMM, accurate=False):
        if miss is not None:
            raise L.VmpError('DiagLoop: no masks - this loop fits complete rows only (DiagFitLoop fits partly observed rows)')
        if weights is not None:
            raise L.VmpError('DiagLoop: no weights - this loop has no weighted pass (DiagFitLoop fits weighted rows)')
        if flavour != L.VMP_GMM:
            raise L.VmpError('DiagLoop: Gaussian mixture only (no Student-t flavour)')
        if accurate:
            raise L.VmpError('DiagLoop: no accurate=True mode')
        N, D = _x_dims(x, 'DiagLoop')
        if not torch.is_tensor(r_init) or r_init.dim() != 2 or r_init.shape[0] != N:
            raise L.VmpError('DiagLoop: r_init has shape %s, expected (%d,K)' % (tuple(r_init.shape) if torch.is_tensor(r_init) else type(r_init), N))
        K = r_init.shape[1]
        _check_dk(D, K)
        if prior is not None:
            _five(prior, K, D, 'DiagLoop', '_0')
        self.x = L.dev_f32(x, 'x')
        dev = self.x.device
        r_init = L.dev_f32(r_init, 'r_init', (N, K))
        self.N, self.D, self.K = N, D, K
        self.prior = _dev5(default_diag_prior(self.x, K) if prior is None else prior, dev, '_0')
        self.post = _post_buffers(K, D, dev)
        self.pack = torch.zeros(K, 2 * D + 1, dtype=torch.float32, device=dev)
        self._data = torch.zeros((), dtype=torch.float64, device=dev)
        self._r = torch.empty(N, K, dtype=torch.float32, device=dev)
        self._logr = None
        self._r_ok = self._logr_ok = False
        self.iterations = 0
        # the moments of r_init: the r_in form of the pass (the pack's values are not read)
        self._stats = mixture_diag_pass(self.x, self.pack, r_in=r_init, want_r=False)[2]

    @classmethod
    def from_centers(cls, x, centers, smooth=0.0, prior=None):
        """start from the responsibilities of the nearest of `centers` (K,D) (nearest_center_r)"""
        return cls(x, nearest_center_r(x, centers, smooth), prior=prior)

    @classmethod
    def from_seed(cls, x, K, seed, smooth=0.0, prior=None):
        """The loop started from the data: r_init = diag_seed_assign on the K centres of diag_seed_centers(x, K, seed) - k-means++ on
        the device, a pure function of (x, K, seed) - then the constructor's r_in pass.  K + 3 launches, no host synchronisation, and
        no buffer of the seeding larger than r_init (N,K) fp32; with prior=None the constructor takes default_diag_prior(x, K), whose
        column means go through an fp64 copy of x as for every DiagLoop - pass a prior to avoid it."""
        centers, _, _ = diag_seed_centers(x, K, seed)
        return cls(x, diag_seed_assign(x, centers, smooth)[0], prior=prior)

    def _iterate(self, iterations, want_r, want_logr):
        if want_logr and self._logr is None:
            self._logr = torch.empty_like(self._r)
        nb = L.lib().vmp_mixture_diag_workspace_bytes(self.N, self.D, self.K)
        ws = L.workspace(self.x.device, nb)
        p = self.post
        L.check(L.lib().vmp_mixture_diag_iterate(
            L.ptr(self.x), self.N, self.D, self.K, *[L.ptr(t) for t in self.prior], L.ptr(self._r if want_r else None),
            L.ptr(self._logr if want_logr else None), *[L.ptr(p[n]) for n in _POST], L.ptr(self.pack), L.ptr(self._stats),
            L.ptr(self._data), L.ptr(ws), nb, iterations, L.stream()), 'vmp_mixture_diag_iterate')
        self.iterations += iterations
        self._r_ok, self._logr_ok = want_r, want_logr

    def step(self, want_logr=False):
        """one iteration; returns the new r (N,K)"""
        self._iterate(1, True, want_logr)
        return self._r

    def run(self, iterations):
        """`iterations` iterations enqueued by one call, r left in the kernel; r / logr are produced by one pass on demand"""
        iterations = int(iterations)
        if iterations < 0:
            raise L.VmpError('iterations must not be negative')
        if iterations:
            self._iterate(iterations, False, False)

    def _need_iteration(self, what):
        if self.iterations == 0:
            raise L.VmpError('%s: no posterior yet - run at least one iteration' % what)

    def _refresh(self):
        """r and log r of the current posterior by one pass under the current pack (the moments it would give are self._stats)"""
        self._need_iteration('r')
        if self._logr is None:
            self._logr = torch.empty_like(self._r)
        nb = L.lib().vmp_mixture_diag_workspace_bytes(self.N, self.D, self.K)
        ws = L.workspace(self.x.device, nb)
        L.check(L.lib().vmp_mixture_diag_pass(L.ptr(self.x), self.N, self.D, self.K, L.ptr(self.pack), None, L.ptr(self._r), L.ptr(self._logr),
                                              None, None, L.ptr(ws), nb, L.stream()), 'vmp_mixture_diag_pass')
        self._r_ok = self._logr_ok = True

    @property
    def r(self):
        if not self._r_ok:
            self._refresh()
        return self._r

    @property
    def logr(self):
        if not self._logr_ok:
            self._refresh()
        return self._logr

    @property
    def stats(self):
        """raw moments (K, 1 + 2 D) fp64 of the current r"""
        return self._stats.clone()

    def theta(self):
        p = self.post
        return p['alpha'], p['beta'], p['m'], p['a'], p['b']

    def aux(self):
        p = self.post
        return p['xbar'], p['S'], p['pi']

    def lower_bound(self):
        """The variational lower bound (nats) of the state the last iteration left.  The pass wrote its data term: one K-sized launch
        and one scalar read-back."""
        self._need_iteration('lower_bound')
        terms = diag_bound_terms(self.prior, self.theta())
        return (self._data - (terms[0] + terms[1])).item()

    def run_until_bound(self, tol, check_every=5, max_iterations=1000):
        """run(check_every) and lower_bound() in turn until the bound improves by less than tol * max(1, |bound|) over the previous
        check, or `max_iterations` iterations of this call are done (the rule of VMPLoop.run_until_bound).  Returns
        [(iterations, bound), ...]."""
        return L.check_until(self, self.lower_bound, lambda v, prev: v - prev < tol * max(1.0, abs(v)), check_every, max_iterations)

    def predictive_pack(self):
        """score pack of the CURRENT posterior (diag_score_pack on theta())"""
        self._need_iteration('predictive_pack')
        return diag_score_pack(*self.theta())

    def _new_rows(self, x_new, miss, what, need_miss=False):
        self._need_iteration(what)
        if not torch.is_tensor(x_new) or x_new.dim() != 2 or x_new.shape[1] != self.D or x_new.shape[0] < 1:
            raise L.VmpError('%s: x has shape %s, expected (M >= 1, %d)' % (what, tuple(x_new.shape) if torch.is_tensor(x_new) else type(x_new), self.D))
        if need_miss and miss is None:
            raise L.VmpError('%s: needs the missing-data mask' % what)
        if miss is not None and (not torch.is_tensor(miss) or tuple(miss.shape) != tuple(x_new.shape)):
            raise L.VmpError('%s: the missing-data mask must be %s' % (what, tuple(x_new.shape)))

    def heldout(self, x_val, miss=None):
        """Mean log posterior predictive density (nats per row) of the rows of x_val (M,D) - of their observed entries with a mask miss
        (M,D), nonzero = missing - under the current posterior.  One streaming launch with its one-wave sum, one scalar read-back."""
        self._new_rows(x_val, miss, 'heldout')
        total = mixture_diag_score(x_val, self.predictive_pack(), miss=miss, want_logp=False, want_sum=True)[3]
        return total.item() / x_val.shape[0]

    def heldout_logprob(self, x_new, miss=None, want_resp=False):
        """logp (M,) of the rows of x_new under the current posterior, and the predictive responsibilities (M,K) with want_resp - what
        gmm.predictive_logprob_diag gives on theta().  One streaming launch, no host synchronisation."""
        self._new_rows(x_new, miss, 'heldout_logprob')
        logp, resp, _, _ = mixture_diag_score(x_new, self.predictive_pack(), miss=miss, want_resp=want_resp)
        return (logp, resp) if want_resp else logp

    def fill(self, x_new, miss):
        """(x_filled (M,D), logp (M,)) of the partly observed rows x_new with mask miss (M,D; nonzero = missing) under the current
        posterior - gmm.predictive_impute_diag on theta().  One streaming launch, no host synchronisation."""
        self._new_rows(x_new, miss, 'fill', need_miss=True)
        logp, _, x_out, _ = mixture_diag_score(x_new, self.predictive_pack(), miss=miss, want_fill=True)
        return x_out, logp

    def run_until(self, x_val, tol, check_every=5, max_iterations=1000):
        """run(check_every) and heldout(x_val) in turn until the score improves by less than `tol` (absolute, nats per row) over the
        previous check, or `max_iterations` iterations of this call are done (the rule of VMPLoop.run_until).  Returns
        [(iterations, score), ...] with `iterations` the loop's running count."""
        return L.check_until(self, lambda: self.heldout(x_val), lambda v, prev: v - prev < tol, check_every, max_iterations)

    def _refuse_score(self, *args, **kw):
        raise L.VmpError('DiagLoop: score and impute are not built for the diagonal mixture under these names - use heldout / '
                         'heldout_logprob / fill')

    def _refuse_sample(self, *args, **kw):
        raise L.VmpError('DiagLoop: sampling (sample, impute_draws) is not built for the diagonal mixture')

    score = impute = _refuse_score
    sample = impute_draws = _refuse_sample


# ---- partly observed and weighted rows (csrc/vmp_diagmfit.hip; include/vmp_hip.h "Diagonal-covariance mixture: fitting partly observed
# and weighted rows") ----

def diag_mfit_pack(alpha, beta, m, a, b):
    """The E-step pack (K, 3 D + 1) fp32 = [ m | lbar = a / b | hl = -1/2 log lbar | c ] of a posterior for the pass on partly observed
    and weighted rows (vmp_mixture_diag_mfit_pack); fp64 inside, rounded once.  A component with a non-positive b, a or beta gets a NaN
    row.  One K-block launch, no host synchronisation."""
    if not torch.is_tensor(m) or m.dim() != 2:
        raise L.VmpError('diag_mfit_pack: m must be (K,D)')
    K, D = m.shape
    _check_dk(D, K)
    theta = _dev5(_five((alpha, beta, m, a, b), K, D, 'diag_mfit_pack'), m.device)
    pack = torch.empty(K, L.lib().vmp_mixture_diag_mfit_pack_words(D), dtype=torch.float32, device=m.device)
    L.check(L.lib().vmp_mixture_diag_mfit_pack(D, K, *[L.ptr(t) for t in theta], L.ptr(pack), L.stream()), 'vmp_mixture_diag_mfit_pack')
    return pack


def _mfit_dims(x, pack, miss, weights, what):
    """(N, D, K) of a pass on masked / weighted rows, refused BEFORE the library or a device is touched"""
    from ._mix import _weights_dims
    N, D = _x_dims(x, what)
    if not torch.is_tensor(pack) or pack.dim() != 2 or pack.shape[1] != 3 * D + 1:
        raise L.VmpError('%s: no masked-fit diagonal pack for D=%d (shape %s, expected (K,%d): diag_mfit_pack)'
                         % (what, D, tuple(pack.shape) if torch.is_tensor(pack) else type(pack), 3 * D + 1))
    K = pack.shape[0]
    _check_dk(D, K)
    if miss is not None:
        _miss_dims(miss, N, D, what)
        if miss.device != x.device:
            raise L.VmpError('%s: the missing-data mask is on %s, x on %s' % (what, miss.device, x.device))
    if weights is not None:
        _weights_dims(x, weights, what)
    return N, D, K


def mixture_diag_mfit_pass(x, pack, miss=None, weights=None, want_r=True, want_logr=False, want_fill=False, want_stats=True,
                           want_bound=False):
    """One streaming pass (vmp_mixture_diag_mfit_pass) over the rows of x (N,D) with an optional mask miss (N,D; nonzero = missing)
    and optional weights (N,) fp32 >= 0 under a diag_mfit_pack: (r (N,K), logr (N,K), x_fill (N,D), stats (K, 1 + 2 D) fp64 = [Nk | sx
    | sxx] of the completed rows, every row counted w_n times, bound 0-dim fp64 = the data term sum_n w_n (logsumexp_k log rho_nk -
    1/2 D_o(n) log 2 pi)); outputs that are not wanted are None.  r and logr are unweighted: a weight does not enter a row's own
    responsibilities.  A row of weight 0 reaches neither stats nor bound whatever it holds; what a missing slot of x holds never
    enters arithmetic.  want_r=False is the fast form: the pass moves x, mask and weights alone.  want_logr needs want_r, want_fill
    needs miss.  The weights are taken as they are (check_weights is the loop's business).  stats and bound are the same bits from
    run to run and for every set of outputs.  No host synchronisation."""
    what = 'mixture_diag_mfit_pass'
    N, D, K = _mfit_dims(x, pack, miss, weights, what)
    if not (want_r or want_logr or want_fill or want_stats or want_bound):
        raise L.VmpError('%s: no output requested' % what)
    if want_logr and not want_r:
        raise L.VmpError('%s: want_logr needs want_r' % what)
    if want_fill and miss is None:
        raise L.VmpError('%s: want_fill needs miss (a complete row has nothing to fill)' % what)
    x = L.dev_f32(x, 'x')
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, 3 * D + 1))
    if pack.device != dev:
        raise L.VmpError('pack is on %s, x on %s' % (pack.device, dev))
    mask = None if miss is None else _mask_u8(miss)
    w = None if weights is None else weights.contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    r = torch.empty(N, K, **f32) if want_r else None
    logr = torch.empty(N, K, **f32) if want_logr else None
    fill = torch.empty(N, D, **f32) if want_fill else None
    stats = torch.empty(K, 1 + 2 * D, dtype=torch.float64, device=dev) if want_stats else None
    bound = torch.empty((), dtype=torch.float64, device=dev) if want_bound else None
    nb = L.lib().vmp_mixture_diag_mfit_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_diag_mfit_pass(L.ptr(x), L.ptr(mask), L.ptr(w), N, D, K, L.ptr(pack), L.ptr(r), L.ptr(logr), L.ptr(fill),
                                               L.ptr(stats), L.ptr(bound), L.ptr(ws), nb, L.stream()), 'vmp_mixture_diag_mfit_pass')
    return r, logr, fill, stats, bound


def _mfit_lower_bound(x, theta, prior, miss, weights):
    what = 'lower_bound_diag'
    N, D, K = _theta_dims(x, theta, what)
    if miss is not None:
        _miss_dims(miss, N, D, what)
    if weights is not None:
        from ._mix import _weights_dims
        _weights_dims(x, weights, what)
    if prior is not None:
        _five(prior, K, D, what, '_0')
    x = L.dev_f32(x, 'x')
    if prior is None:
        prior = default_diag_prior(x, K, miss=miss, weights=weights)
    terms = diag_bound_terms(prior, theta)
    data = mixture_diag_mfit_pass(x, diag_mfit_pack(*theta), miss=miss, weights=weights, want_r=False, want_stats=False, want_bound=True)[4]
    return data - (terms[0] + terms[1])


class DiagFitLoop(DiagLoop):
    """DiagLoop on partly observed and / or weighted rows: miss (N,D), nonzero = missing, and weights (N,) fp32, finite, >= 0, not all
    zero, both on x's device; at least one of the two.  The missing entries are latent variables with q(x_nd | z_n = k) = N(m_kd,
    b_kd / a_k): the posterior keeps its shape, the M-step is the finalize of DiagLoop on the moments of the completed rows, the E-step
    runs on the observed entries, and both stay exact coordinate ascent - lower_bound() never falls (csrc/vmp_diagmfit.hip, one
    streaming pass per iteration).  Row n counts w_n times in the moments and in the bound; a weight does not enter a row's own
    responsibilities, and a row of weight 0 reaches nothing the fit adds up, whatever it holds.  What a missing slot of x holds is
    never read into arithmetic.  The surface is DiagLoop's (step, run, r, logr, stats, theta, aux, lower_bound, run_until_bound,
    run_until, heldout, heldout_logprob, fill, predictive_pack) plus filled(): x with its missing entries replaced by sum_k r_nk m_kd.
    The start: the moments of r_init * w on x with every missing entry (and every row of weight 0) replaced by its column's weighted
    mean over the observed entries - linear in r, no variance term at the start - through the r_in form of mixture_diag_pass."""

    def __init__(self, x, r_init, miss=None, weights=None, prior=None):
        what = 'DiagFitLoop'
        if miss is None and weights is None:
            raise L.VmpError('DiagFitLoop: neither miss nor weights given - complete unweighted rows are fitted by DiagLoop')
        N, D = _x_dims(x, what)
        if not torch.is_tensor(r_init) or r_init.dim() != 2 or r_init.shape[0] != N:
            raise L.VmpError('%s: r_init has shape %s, expected (%d,K)' % (what, tuple(r_init.shape) if torch.is_tensor(r_init) else type(r_init), N))
        K = r_init.shape[1]
        _check_dk(D, K)
        if prior is not None:
            _five(prior, K, D, what, '_0')
        if miss is not None:
            _miss_dims(miss, N, D, what)
            if miss.device != x.device:
                raise L.VmpError('%s: the missing-data mask is on %s, x on %s' % (what, miss.device, x.device))
        if weights is not None:
            from ._mix import check_weights
            check_weights(x, weights)
        self.x = L.dev_f32(x, 'x')
        dev = self.x.device
        r_init = L.dev_f32(r_init, 'r_init', (N, K))
        self.N, self.D, self.K = N, D, K
        self.miss = None if miss is None else _mask_u8(miss)
        self.weights = None if weights is None else weights.contiguous()
        mean, live = observed_column_means(self.x, self.miss, self.weights)
        if prior is None:
            prior = default_diag_prior(self.x, K, miss=self.miss, weights=self.weights)
        self.prior = _dev5(prior, dev, '_0')
        self.post = _post_buffers(K, D, dev)
        self.pack = torch.zeros(K, 3 * D + 1, dtype=torch.float32, device=dev)
        self._data = torch.zeros((), dtype=torch.float64, device=dev)
        self._r = torch.empty(N, K, dtype=torch.float32, device=dev)
        self._logr = None
        self._fill = None if miss is None else torch.empty(N, D, dtype=torch.float32, device=dev)
        self._r_ok = self._logr_ok = False
        self.iterations = 0
        # the moments of r_init * w on the mean-filled rows: the r_in form of the complete-row pass (its pack's values are not read)
        x_start = torch.where(live, self.x, mean.to(torch.float32)[None, :])
        r_start = r_init if self.weights is None else r_init * self.weights[:, None]
        self._stats = mixture_diag_pass(x_start, torch.zeros(K, 2 * D + 1, dtype=torch.float32, device=dev), r_in=r_start, want_r=False)[2]

    @classmethod
    def from_centers(cls, x, centers, smooth=0.0, weights=None, prior=None, miss=None):
        """start from the responsibilities of the nearest of `centers` (K,D) (nearest_center_r, unweighted); complete rows only"""
        if miss is not None:
            raise L.VmpError('DiagFitLoop.from_centers: nearest centres of masked wide rows are not built - pass an r_init')
        return cls(x, nearest_center_r(x, centers, smooth), weights=weights, prior=prior)

    @classmethod
    def from_seed(cls, x, K, seed, weights=None, smooth=0.0, prior=None, miss=None):
        """The weighted loop started from the data: the unweighted k-means++ centres of diag_seed_centers(x, K, seed) and their
        nearest-centre responsibilities diag_seed_assign, then the constructor.  Seeding on masked wide rows is not built (a later
        change): with miss= this refuses."""
        if miss is not None:
            raise L.VmpError('DiagFitLoop.from_seed: k-means++ seeding on masked wide rows is not built yet (a later pull request) - '
                             'pass an r_init, or seed complete rows with weights=')
        if weights is None:
            raise L.VmpError('DiagFitLoop.from_seed: neither miss nor weights given - complete unweighted rows are seeded by DiagLoop.from_seed')
        from ._mix import check_weights
        check_weights(x, weights)                                            # before anything is seeded
        centers, _, _ = diag_seed_centers(x, K, seed)
        return cls(x, diag_seed_assign(x, centers, smooth)[0], weights=weights, prior=prior)

    def _outputs(self, want_r, want_logr):
        if want_logr and self._logr is None:
            self._logr = torch.empty_like(self._r)
        return (L.ptr(self._r if want_r else None), L.ptr(self._logr if want_logr else None),
                L.ptr(self._fill if want_r else None))

    def _iterate(self, iterations, want_r, want_logr):
        r, logr, fill = self._outputs(want_r, want_logr)
        nb = L.lib().vmp_mixture_diag_mfit_workspace_bytes(self.N, self.D, self.K)
        ws = L.workspace(self.x.device, nb)
        p = self.post
        L.check(L.lib().vmp_mixture_diag_mfit_iterate(
            L.ptr(self.x), L.ptr(self.miss), L.ptr(self.weights), self.N, self.D, self.K, *[L.ptr(t) for t in self.prior], r, logr, fill,
            *[L.ptr(p[n]) for n in _POST], L.ptr(self.pack), L.ptr(self._stats), L.ptr(self._data), L.ptr(ws), nb, iterations,
            L.stream()), 'vmp_mixture_diag_mfit_iterate')
        self.iterations += iterations
        self._r_ok, self._logr_ok = want_r, want_logr

    def _refresh(self):
        """r, log r and the fill of the current posterior by one pass under the current pack"""
        self._need_iteration('r')
        r, logr, fill = self._outputs(True, True)
        nb = L.lib().vmp_mixture_diag_mfit_workspace_bytes(self.N, self.D, self.K)
        ws = L.workspace(self.x.device, nb)
        L.check(L.lib().vmp_mixture_diag_mfit_pass(L.ptr(self.x), L.ptr(self.miss), L.ptr(self.weights), self.N, self.D, self.K,
                                                   L.ptr(self.pack), r, logr, fill, None, None, L.ptr(ws), nb, L.stream()),
                'vmp_mixture_diag_mfit_pass')
        self._r_ok = self._logr_ok = True

    def filled(self):
        """x with its missing entries replaced by sum_k r_nk m_kd under the current posterior (observed entries bit for bit); written
        by the pass that writes r.  A fit without a mask has nothing to fill."""
        if self.miss is None:
            raise L.VmpError('DiagFitLoop.filled: the loop has no mask - nothing to fill')
        if not self._r_ok:
            self._refresh()
        return self._fill
