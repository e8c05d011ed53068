"""Host-side engine of the pure mixture VMP (T1): thin wrappers over the vmp_mix_* C ABI
(include/vmp_hip.h) shared by models/gmm.py and models/smm.py."""
import os

import torch

from .. import _lib as L


def _dims(x, K):
    N, D = x.shape
    if not (1 <= D <= L.MAX_D):
        raise L.VmpError('D=%d outside the compiled range 1..%d' % (D, L.MAX_D))
    if not (1 <= K <= L.MAX_K):
        raise L.VmpError('K=%d outside the compiled range 1..%d' % (K, L.MAX_K))
    return N, D


def _ws(x, N, D, K):
    nbytes = L.lib().vmp_mix_workspace_bytes(N, D, K)
    return L.workspace(x.device, nbytes), nbytes


def pivot_of(x):
    """(D,) fp32 pivot near the data mean (vmp_mix_pivot) - see include/vmp_hip.h."""
    x = L.dev_f32(x, 'x')
    N, D = x.shape
    pv = torch.empty(D, dtype=torch.float32, device=x.device)
    L.check(L.lib().vmp_mix_pivot(L.ptr(x), N, D, L.ptr(pv), L.stream()), 'vmp_mix_pivot')
    return pv


SMALL_STATS_MAX_N = 512        # csrc/vmp_mix.hip: small_stats_kernel


def raw_stats(x, r, u=None, pivot=None):
    """(K, 2+D+D*D) fp64 raw moments [Nk | Wk | sum w x | sum w x x^T] (vmp_mix_stats).
    pivot=None: the data are shifted by a pivot near their mean before the products are formed (vmp_mix_pivot; what makes the
    one-pass moments match the reference's two-pass CENTRED S_k of gmm.py:39-46); pivot=False: no shift - for callers that use
    the raw moments as they are (the SVAE M-step in natural parameters, svae.py:154-176: theta* = prior + raw moments)."""
    x = L.dev_f32(x, 'x')
    N, K = r.shape
    if pivot is False:
        pivot = None
    elif pivot is None and N > SMALL_STATS_MAX_N:        # small batches: the library sums them directly in fp64 (one launch)
        pivot = pivot_of(x)
    _, D = _dims(x, K)
    r = L.dev_f32(r, 'r_nk', (N, K))
    if u is not None:
        u = L.dev_f32(u, 'u_nk', (N, K))
    stats = torch.empty((K, L.lib().vmp_mix_stats_words(D)), dtype=torch.float64, device=x.device)
    ws, nb = _ws(x, N, D, K)
    L.check(L.lib().vmp_mix_stats(L.ptr(x), L.ptr(r), L.ptr(u), L.ptr(pivot), N, D, K, L.ptr(stats), L.ptr(ws), nb,
                                  L.stream()), 'vmp_mix_stats')
    return stats


def _prior(prior, K, D, dev):
    a0, b0, m0, C0, v0 = prior
    return (L.dev_f32(a0.to(dev, torch.float32), 'alpha_0', (K,)), L.dev_f32(b0.to(dev, torch.float32).reshape(K), 'beta_0', (K,)),
            L.dev_f32(m0.to(dev, torch.float32), 'm_0', (K, D)), L.dev_f32(C0.to(dev, torch.float32), 'C_0', (K, D, D)),
            L.dev_f32(v0.to(dev, torch.float32), 'v_0', (K,)))


_POST = ('alpha', 'beta', 'm', 'C', 'v', 'xbar', 'S', 'pi', 'pack')      # the posterior outputs, in the order of the C ABI


def _post_buffers(K, D, device, want_pack=True):
    f32 = dict(dtype=torch.float32, device=device)
    return dict(alpha=torch.empty(K, **f32), beta=torch.empty(K, **f32), m=torch.empty(K, D, **f32),
                C=torch.empty(K, D, D, **f32), v=torch.empty(K, **f32), xbar=torch.empty(K, D, **f32),
                S=torch.empty(K, D, D, **f32), pi=torch.empty(K, **f32),
                pack=torch.empty(K, L.lib().vmp_mix_pack_words(D), **f32) if want_pack else None)


def _fin_tail(D, K, flavour, prior, kappa, post):
    """(D, K, flavour, prior x 5, kappa, posterior x 9): what every finalize entry point takes behind its source (post=None: no
    posterior output, the reduction-only form)"""
    return ([D, K, flavour] + [L.ptr(t) for t in prior] + [L.ptr(kappa)]
            + [L.ptr(post[k]) if post is not None else None for k in _POST])


def finalize(stats, prior, flavour, kappa=None, want_pack=True):
    """Posterior (alpha, beta, m, C, v, xbar, S, pi) and the E-step pack from raw stats (vmp_mix_finalize)."""
    K = stats.shape[0]
    dev = stats.device
    D = prior[2].shape[1]
    out = _post_buffers(K, D, dev, want_pack)
    kap = None if kappa is None else L.dev_f32(kappa.to(dev, torch.float32), 'kappa', (K,))
    L.check(L.lib().vmp_mix_finalize(L.ptr(stats), *_fin_tail(D, K, flavour, _prior(prior, K, D, dev), kap, out), L.stream()),
            'vmp_mix_finalize')
    return out


def pack_from_params(alpha_k, beta_k, m_k, P_k, v_k, flavour, kappa=None):
    K, D = m_k.shape
    dev = m_k.device
    f32 = dict(dtype=torch.float32, device=dev)
    args = [L.dev_f32(t.to(torch.float32), n) for t, n in ((alpha_k, 'alpha_k'), (beta_k, 'beta_k'), (m_k, 'm_k'),
                                                           (P_k, 'P_k'), (v_k, 'v_k'))]
    kap = None if kappa is None else L.dev_f32(kappa.to(dev, torch.float32), 'kappa', (K,))
    pack = torch.empty(K, L.lib().vmp_mix_pack_words(D), **f32)
    pi = torch.empty(K, **f32)
    L.check(L.lib().vmp_mix_pack_from_params(D, K, flavour, *[L.ptr(t) for t in args], L.ptr(kap), L.ptr(pack),
                                             L.ptr(pi), L.stream()), 'vmp_mix_pack_from_params')
    return pack, pi


def estep(x, pack, flavour, miss_mask=None, want_logr=False, want_stats=False, r_out=None, u_out=None):
    """Responsibilities (and SMM scales) for all rows; optionally fused raw stats of the new r."""
    x = L.dev_f32(x, 'x')
    K = pack.shape[0]
    N, D = _dims(x, K)
    f32 = dict(dtype=torch.float32, device=x.device)
    r = torch.empty(N, K, **f32) if r_out is None else r_out
    u = None
    if flavour == L.VMP_SMM:
        u = torch.empty(N, K, **f32) if u_out is None else u_out
    logr = torch.empty(N, K, **f32) if want_logr else None
    stats = torch.empty((K, L.lib().vmp_mix_stats_words(D)), dtype=torch.float64, device=x.device) if want_stats else None
    ws, nb, pivot = (None, 0, None)
    if want_stats:
        ws, nb = _ws(x, N, D, K)
        pivot = pivot_of(x)
    mask = None
    if miss_mask is not None:
        if not miss_mask.is_cuda:
            raise L.VmpError('missing_data_mask must be on the GPU')
        mask = miss_mask.to(torch.uint8).contiguous()
    L.check(L.lib().vmp_mix_estep(L.ptr(x), N, D, K, flavour, L.ptr(pack), L.ptr(mask), L.ptr(r), L.ptr(u), L.ptr(logr),
                                  L.ptr(pivot), L.ptr(stats), L.ptr(ws), nb, L.stream()), 'vmp_mix_estep')
    return r, u, logr, stats


def _kd(t, name, shape):
    """shape check of a K-sized operand BEFORE the library or the device is touched (CPU tensors fail here too)"""
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise L.VmpError('%s has shape %s, expected %s' % (name, tuple(t.shape) if torch.is_tensor(t) else type(t), tuple(shape)))
    return t


def _score_dims(x, m, what):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise L.VmpError('%s: x must be (N,D)' % what)
    if not torch.is_tensor(m) or m.dim() != 2 or m.shape[1] != x.shape[1]:
        raise L.VmpError('%s: the component locations must be (K,%d), got %s' % (what, x.shape[1], tuple(m.shape) if torch.is_tensor(m) else type(m)))
    K = m.shape[0]
    N, D = _dims(x, K)
    if N < 1:
        raise L.VmpError('%s: x has no rows' % what)
    return N, D, K


_NIW = (('alpha_k', 'beta_k', 'm_k', 'C_k', 'v_k'), lambda K, D: ((K,), (K,), (K, D), (K, D, D), (K,)))
_STUDENT = (('log_w', 'mu', 'sigma', 'nu'), lambda K, D: ((K,), (K, D), (K, D, D), (K,)))


def _k_pack(entry, words_entry, ops, names, shapes, device):
    """One K-sized pack (score, impute or fit) from K-sized operands: shapes checked BEFORE the library or the device is touched,
    then dev_f32, the (K, words_entry(D)) buffer and the C entry point"""
    K, D = next(shp for shp in shapes if len(shp) == 2)
    ops = [_kd(t, n, shp) for t, n, shp in zip(ops, names, shapes)]
    ops = [L.dev_f32(t.detach().to(torch.float32), n) for t, n in zip(ops, names)]
    pack = torch.empty(K, getattr(L.lib(), words_entry)(D), dtype=torch.float32, device=device)
    L.check(getattr(L.lib(), entry)(D, K, *[L.ptr(t) for t in ops], L.ptr(pack), L.stream()), entry)
    return pack


def score_pack_niw(alpha_k, beta_k, m_k, C_k, v_k):
    """Score pack of the GMM posterior predictive (vmp_mix_score_pack_niw; Bishop 10.81-10.82) from the NIW posterior
    (alpha (K), beta (K), m (K,D), C (K,D,D), v (K)) = gmm.inference's theta."""
    return _k_pack('vmp_mix_score_pack_niw', 'vmp_mix_pack_words', (alpha_k, beta_k, m_k, C_k, v_k), _NIW[0], _NIW[1](*m_k.shape),
                   m_k.device)


def score_pack_t(log_w, mu, sigma, nu):
    """Score pack of an explicit Student-t mixture (vmp_mix_score_pack_t; reference student_t.py:31-37): log_w (K), mu (K,D),
    sigma (K,D,D) scale matrices, nu (K) degrees of freedom."""
    return _k_pack('vmp_mix_score_pack_t', 'vmp_mix_pack_words', (log_w, mu, sigma, nu), _STUDENT[0], _STUDENT[1](*mu.shape), mu.device)


def mixture_score(x, pack, want_logp=True, want_resp=False, want_sum=True):
    """One streaming pass (vmp_mix_score): (logp (N,) fp32, resp (N,K) fp32, total 0-dim fp64) of the rows of x under a score
    pack; outputs that are not wanted are None.  Everything stays on the device: no host synchronisation."""
    x = L.dev_f32(x, 'x')
    K = pack.shape[0]
    N, D = _dims(x, K)
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, L.lib().vmp_mix_pack_words(D)))      # an impute pack is wider: not interchangeable
    logp = torch.empty(N, dtype=torch.float32, device=dev) if want_logp else None
    resp = torch.empty(N, K, dtype=torch.float32, device=dev) if want_resp else None
    total, ws, nb = None, None, 0
    if want_sum:
        total = torch.empty((), dtype=torch.float64, device=dev)
        nb = L.lib().vmp_mix_score_workspace_bytes(N, D, K)
        ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mix_score(L.ptr(x), N, D, K, L.ptr(pack), L.ptr(logp), L.ptr(resp), L.ptr(total), L.ptr(ws), nb,
                                  L.stream()), 'vmp_mix_score')
    return logp, resp, total


def _impute_dims(x, miss, m, what):
    """shapes of (x, miss, component locations) BEFORE the library or the device is touched"""
    N, D, K = _score_dims(x, m, what)
    if not torch.is_tensor(miss) or tuple(miss.shape) != (N, D):
        raise L.VmpError('%s: the missing-data mask must be (%d,%d), got %s' % (what, N, D, tuple(miss.shape) if torch.is_tensor(miss) else type(miss)))
    return N, D, K


def impute_pack_niw(alpha_k, beta_k, m_k, C_k, v_k):
    """Impute pack of the GMM posterior predictive (vmp_mixture_impute_pack_niw) from the NIW posterior (alpha (K), beta (K), m (K,D),
    C (K,D,D), v (K)) = gmm.inference's theta: the mixture score_pack_niw scores."""
    return _k_pack('vmp_mixture_impute_pack_niw', 'vmp_mixture_impute_pack_words', (alpha_k, beta_k, m_k, C_k, v_k), _NIW[0],
                   _NIW[1](*m_k.shape), m_k.device)


def impute_pack_t(log_w, mu, sigma, nu):
    """Impute pack of an explicit Student-t mixture (vmp_mixture_impute_pack_t): log_w (K), mu (K,D), sigma (K,D,D) scale matrices,
    nu (K) degrees of freedom."""
    return _k_pack('vmp_mixture_impute_pack_t', 'vmp_mixture_impute_pack_words', (log_w, mu, sigma, nu), _STUDENT[0],
                   _STUDENT[1](*mu.shape), mu.device)


def _masked_operands(x, miss, pack, words_entry, hint):
    """(x fp32 on the device, uint8 mask, pack, N, D, K) of a streaming pass over partly observed rows, validated: a pack of another
    kind (a score pack is D + D(D+1)/2 + 4 words) would make the kernel read past its end"""
    x = L.dev_f32(x, 'x')
    if not torch.is_tensor(pack) or pack.dim() != 2:
        raise L.VmpError('pack must be a (K, words) tensor from %s' % hint)
    K = pack.shape[0]
    N, D = _dims(x, K)
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, getattr(L.lib(), words_entry)(D)))
    if pack.device != dev:
        raise L.VmpError('pack is on %s, x on %s' % (pack.device, dev))
    if not torch.is_tensor(miss) or tuple(miss.shape) != (N, D):
        raise L.VmpError('the missing-data mask must be (%d,%d)' % (N, D))
    if miss.device != dev:
        raise L.VmpError('the missing-data mask is on %s, x on %s' % (miss.device, dev))
    return x, _mask_u8(miss), pack, N, D, K


def mixture_impute(x, miss, pack, want_x=True, want_logp=True, want_resp=False, want_sum=False, inplace=False):
    """One streaming pass (vmp_mixture_impute) over the rows of x (N,D) and their mask miss (N,D; nonzero / True = missing) under an
    impute pack: (x_out (N,D), logp (N,), resp (N,K), total 0-dim fp64); outputs that are not wanted are None.
      x_out - x with its missing entries replaced by sum_k resp_k (mu_m - Lambda_mm^-1 Lambda_mo (x_o - mu_o))_k, the conditional mean
              (for nu <= 1, where no mean exists, the conditional location); observed entries are copied bit for bit; inplace=True
              writes into x itself (which must then be a contiguous fp32 GPU tensor) and returns it;
      logp  - the marginal log density of the observed entries (log 1 = the log-sum-exp of the weights for a row without any);
      resp  - exp(term_nk - logp_n).
    What a missing slot of x holds is never read into arithmetic (NaN there is fine).  A row whose every weight is -inf gets
    logp = -inf, resp = 0 and 0 in its missing entries.  Everything stays on the device: no host synchronisation."""
    xin = x
    x, mask, pack, N, D, K = _masked_operands(x, miss, pack, 'vmp_mixture_impute_pack_words', 'impute_pack_niw / impute_pack_t')
    dev = x.device
    x_out = None
    if want_x:
        if inplace and x.data_ptr() != xin.data_ptr():
            raise L.VmpError('inplace=True needs a contiguous x')
        x_out = x if inplace else torch.empty_like(x)
    logp = torch.empty(N, dtype=torch.float32, device=dev) if want_logp else None
    resp = torch.empty(N, K, dtype=torch.float32, device=dev) if want_resp else None
    total, ws, nb = None, None, 0
    if want_sum:
        total = torch.empty((), dtype=torch.float64, device=dev)
        nb = L.lib().vmp_mixture_impute_workspace_bytes(N, D, K)
        ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_impute(L.ptr(x), L.ptr(mask), N, D, K, L.ptr(pack), L.ptr(x_out), L.ptr(logp), L.ptr(resp),
                                       L.ptr(total), L.ptr(ws), nb, L.stream()), 'vmp_mixture_impute')
    return (xin if (want_x and inplace) else x_out), logp, resp, total


def _draw_counts(seed, draws, row0):
    """(seed, draws, row0) of a sampling pass as Python ints, refused BEFORE the library or the device is touched"""
    seed, draws, row0 = int(seed), int(draws), int(row0)
    if not 0 <= seed < 1 << 64:
        raise L.VmpError('seed must be in 0 .. 2^64 - 1 (got %d)' % seed)
    if draws < 1:
        raise L.VmpError('draws must be >= 1 (got %d)' % draws)
    if row0 < 0:
        raise L.VmpError('row0 must be >= 0 (got %d)' % row0)
    return seed, draws, row0


def _impute_pack_dim(pack):
    """D of an impute pack, from its width (2 D + D (D + 1) / 2 + 5 words; a score pack or a fit pack has no such D)"""
    if not torch.is_tensor(pack) or pack.dim() != 2 or pack.shape[0] < 1:
        raise L.VmpError('pack must be a (K, words) tensor from impute_pack_niw / impute_pack_t')
    for D in range(1, L.MAX_D + 1):
        if 2 * D + D * (D + 1) // 2 + 5 == pack.shape[1]:
            return D
    raise L.VmpError('pack has shape %s: %d words per component is no impute pack (impute_pack_niw / impute_pack_t; a score pack or a '
                     'fit pack does not do)' % (tuple(pack.shape), pack.shape[1]))


def _sample_launch(x, mask, pack, N, D, K, seed, draws, row0, want_z):
    x_out = torch.empty(draws, N, D, dtype=torch.float32, device=pack.device)
    z = torch.empty(draws, N, dtype=torch.int32, device=pack.device) if want_z else None
    L.check(L.lib().vmp_mixture_sample(L.ptr(x), L.ptr(mask), N, D, K, L.ptr(pack), seed, row0, draws, L.ptr(x_out), L.ptr(z),
                                       L.stream()), 'vmp_mixture_sample')
    return x_out, z


def mixture_sample(x, miss, pack, seed, draws=1, row0=0, want_z=False):
    """`draws` seeded draws of the missing entries of every row of x (N,D) - miss (N,D), nonzero / True = missing - from
    p(x_missing | x_observed) under an impute pack, in one streaming pass (vmp_mixture_sample): (x_draws (draws,N,D), z (draws,N)
    int32 or None) - multiple imputation.  Observed entries are copied bit for bit; z is the component each draw came from (-1 in a
    row whose every weight is -inf, whose missing entries are 0).  The random stream is a function of (seed, row0 + n, draw) only:
    rows [a, b) drawn with row0 = a are rows a .. b of the whole call, and two calls with the same arguments return the same bits.
    What a missing slot of x holds is never read into arithmetic.  Everything stays on the device: no host synchronisation."""
    seed, draws, row0 = _draw_counts(seed, draws, row0)
    D = _impute_pack_dim(pack)
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != D:
        raise L.VmpError('x has shape %s, expected (N,%d) for this pack' % (tuple(x.shape) if torch.is_tensor(x) else type(x), D))
    x, mask, pack, N, D, K = _masked_operands(x, miss, pack, 'vmp_mixture_impute_pack_words', 'impute_pack_niw / impute_pack_t')
    return _sample_launch(x, mask, pack, N, D, K, seed, draws, row0, want_z)


def mixture_draw(n, pack, seed, row0=0, want_z=False):
    """n seeded rows from the mixture of an impute pack itself (vmp_mixture_sample without x and mask: every entry missing):
    (x (n,D), z (n,) int32 or None).  Row i is a function of (seed, row0 + i) only.  No host synchronisation."""
    seed, _, row0 = _draw_counts(seed, 1, row0)
    n = int(n)
    if n < 1:
        raise L.VmpError('n must be >= 1 (got %d)' % n)
    D = _impute_pack_dim(pack)
    K = pack.shape[0]
    if not 1 <= K <= L.MAX_K:
        raise L.VmpError('K=%d outside compiled range 1..%d' % (K, L.MAX_K))
    pack = L.dev_f32(pack, 'pack')
    x_out, z = _sample_launch(None, None, pack, n, D, K, seed, 1, row0, want_z)
    return x_out[0], (z[0] if want_z else None)


_mask_u8 = L.mask_u8


def fit_pack(alpha_k, beta_k, m_k, C_k, v_k):
    """Fit pack of the NIW posterior (vmp_mixture_fit_pack): [m | v C^-1 packed lower | E log pi + 1/2 E log|Lambda| - D / (2 beta)]
    per component - what mixture_fit_pass evaluates the E-step on partly observed rows from."""
    return _k_pack('vmp_mixture_fit_pack', 'vmp_mixture_fit_pack_words', (alpha_k, beta_k, m_k, C_k, v_k), _NIW[0], _NIW[1](*m_k.shape),
                   m_k.device)


def mixture_fit_pass(x, miss, pack, want_logr=False, want_fill=False, want_stats=True):
    """One streaming pass (vmp_mixture_fit_pass) over the rows of x (N,D) and their mask miss (N,D; nonzero = missing) under a fit
    pack: (r (N,K), logr (N,K), x_fill (N,D), stats (K, 2+D+D*D) fp64); outputs that are not wanted are None.  r is the E-step with
    the missing entries integrated out; x_fill is x with its missing entries replaced by sum_k r_nk E_q[x_m | k]; stats are the raw
    moments [Nk | Wk | sx | sxx] of the completed rows, the conditional covariances included - the input of finalize().  What a
    missing slot of x holds is never read into arithmetic.  No host synchronisation."""
    x, mask, pack, N, D, K = _masked_operands(x, miss, pack, 'vmp_mixture_fit_pack_words', 'fit_pack')
    dev = x.device
    f32 = dict(dtype=torch.float32, device=dev)
    r = torch.empty(N, K, **f32)
    logr = torch.empty(N, K, **f32) if want_logr else None
    x_fill = torch.empty(N, D, **f32) if want_fill else None
    stats = torch.empty((K, L.lib().vmp_mix_stats_words(D)), dtype=torch.float64, device=dev) if want_stats else None
    nb = L.lib().vmp_mixture_fit_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_fit_pass(L.ptr(x), L.ptr(mask), N, D, K, L.ptr(pack), L.ptr(r), L.ptr(logr), L.ptr(x_fill),
                                         L.ptr(stats), L.ptr(ws), nb, L.stream()), 'vmp_mixture_fit_pass')
    return r, logr, x_fill, stats


def _bound_dims(x, miss, pack_or_m, what, pack=False):
    """(N, D, K) of a lower-bound call, refused BEFORE the library or a device is touched: x (N >= 1, D), an optional mask (N,D) on
    x's device and either the component locations (K,D) or a fit pack (K, D + D(D+1)/2 + 1) - a score or impute pack is wider and
    would make the kernel read past its end"""
    if pack:
        if not torch.is_tensor(x) or x.dim() != 2:
            raise L.VmpError('%s: x must be (N,D)' % what)
        if not torch.is_tensor(pack_or_m) or pack_or_m.dim() != 2:
            raise L.VmpError('%s: pack must be a (K, words) tensor from fit_pack' % what)
        K = pack_or_m.shape[0]
        N, D = _dims(x, K)
        words = D + D * (D + 1) // 2 + 1
        if pack_or_m.shape[1] != words:
            raise L.VmpError('%s: pack has shape %s, expected (%d,%d): %d words per component is no fit pack for D=%d (fit_pack; a score '
                             'pack or an impute pack does not do)' % (what, tuple(pack_or_m.shape), K, words, pack_or_m.shape[1], D))
        if N < 1:
            raise L.VmpError('%s: x has no rows' % what)
    else:
        N, D, K = _score_dims(x, pack_or_m, what)
    if miss is not None:
        if not torch.is_tensor(miss) or tuple(miss.shape) != (N, D):
            raise L.VmpError('%s: the missing-data mask has shape %s, expected %s'
                             % (what, tuple(miss.shape) if torch.is_tensor(miss) else type(miss), (N, D)))
        if miss.device != x.device:
            raise L.VmpError('%s: the missing-data mask is on %s, x on %s' % (what, miss.device, x.device))
    return N, D, K


def mixture_bound(x, miss, pack, want_rows=False):
    """The data term of the variational lower bound in one streaming pass (vmp_mixture_bound_pass) over the rows of x (N,D) under a
    fit pack: (data 0-dim fp64 on the device, lse (N,) fp32 or None), data = sum_n [logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi] and
    lse_n the log-sum-exp alone.  miss (N,D), nonzero = missing, on x's device: the missing entries are integrated out as in
    mixture_fit_pass and what their slots of x hold is never read into arithmetic; miss=None: every entry observed, nothing is
    factored.  The sum is deterministic: the same bits from run to run and with or without want_rows.  No host synchronisation."""
    N, D, K = _bound_dims(x, miss, pack, 'mixture_bound', pack=True)
    x = L.dev_f32(x, 'x')
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, L.lib().vmp_mixture_fit_pack_words(D)))
    if pack.device != dev:
        raise L.VmpError('pack is on %s, x on %s' % (pack.device, dev))
    mask = None if miss is None else _mask_u8(miss)
    data = torch.empty((), dtype=torch.float64, device=dev)
    lse = torch.empty(N, dtype=torch.float32, device=dev) if want_rows else None
    nb = L.lib().vmp_mixture_bound_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_bound_pass(L.ptr(x), L.ptr(mask), N, D, K, L.ptr(pack), L.ptr(lse), L.ptr(data), L.ptr(ws), nb,
                                           L.stream()), 'vmp_mixture_bound_pass')
    return data, lse


def _niw_shapes(ops, names, K, D):
    return [_kd(t, n, shp) for t, n, shp in zip(ops, names, _NIW[1](K, D))]


def bound_terms(prior, theta):
    """The K-sized terms of the variational lower bound (vmp_mixture_bound_terms): a (2+K,) fp64 device tensor
    [KL(q(pi) || p(pi)) | sum_k KL(q(mu, Lambda)_k || p) | the K terms of that sum] from prior = (alpha_0, beta_0, m_0, C_0, v_0) and
    theta = (alpha_k, beta_k, m_k, C_k, v_k); fp64 inside, the sums in k order.  One launch, no host synchronisation."""
    if len(prior) != 5 or len(theta) != 5:
        raise L.VmpError('bound_terms: prior and theta are (alpha, beta, m, C, v)')
    m_k = theta[2]
    if not torch.is_tensor(m_k) or m_k.dim() != 2:
        raise L.VmpError('bound_terms: m_k must be (K,D)')
    K, D = m_k.shape
    theta = _niw_shapes(theta, _NIW[0], K, D)
    a0, b0, m0, C0, v0 = prior
    if torch.is_tensor(b0) and b0.numel() == K:
        b0 = b0.reshape(K)
    prior = _niw_shapes((a0, b0, m0, C0, v0), ('alpha_0', 'beta_0', 'm_0', 'C_0', 'v_0'), K, D)
    if not (1 <= D <= L.MAX_D):
        raise L.VmpError('D=%d outside the compiled range 1..%d' % (D, L.MAX_D))
    if not (1 <= K <= L.MAX_K):
        raise L.VmpError('K=%d outside the compiled range 1..%d' % (K, L.MAX_K))
    dev = m_k.device
    theta = [L.dev_f32(t.detach().to(torch.float32), n) for t, n in zip(theta, _NIW[0])]
    prior = _prior(prior, K, D, dev)
    out = torch.empty(2 + K, dtype=torch.float64, device=dev)
    L.check(L.lib().vmp_mixture_bound_terms(D, K, *[L.ptr(t) for t in prior], *[L.ptr(t) for t in theta], L.ptr(out), L.stream()),
            'vmp_mixture_bound_terms')
    return out


def lower_bound(x, theta, prior=None, miss=None, weights=None):
    """The variational lower bound (free energy) of the Gaussian-mixture posterior theta = (alpha_k, beta_k, m_k, C_k, v_k) on the rows
    of x (N,D): a 0-dim fp64 device tensor, data - KL(q(pi) || p(pi)) - sum_k KL(q(mu, Lambda)_k || p) (include/vmp_hip.h "Variational
    lower bound") with q(z) - and, under a mask, q(x_m | z) - at their optimum for theta: the free energy of a loop after step().
    miss (N,D), nonzero = missing, on x's device; prior=None: default_prior.  fit_pack, mixture_bound, bound_terms and one
    subtraction, all on the device: no host synchronisation.  weights (N,) fp32 >= 0 on x's device: row n counts w_n times in the
    data term and a row of weight 0 not at all (the bound-only form of mixture_wfit_pass; include/vmp_hip.h "Mixture fitting on
    weighted rows"); weights=None is the unweighted pass, unchanged."""
    if len(theta) != 5:
        raise L.VmpError('lower_bound: theta is (alpha_k, beta_k, m_k, C_k, v_k)')
    N, D, K = _bound_dims(x, miss, theta[2], 'lower_bound')
    if weights is not None:
        _weights_dims(x, weights, 'lower_bound')
    theta = _niw_shapes(theta, _NIW[0], K, D)
    prior = default_prior(K, D, x.device) if prior is None else prior
    terms = bound_terms(prior, theta)
    if weights is not None:
        data = mixture_wfit_pass(x, weights, fit_pack(*theta), miss=miss, want_r=False, want_stats=False, want_bound=True)[4]
    else:
        data, _ = mixture_bound(x, miss, fit_pack(*theta))
    return data - (terms[0] + terms[1])


def _weights_dims(x, weights, what):
    """shape and device of the (N,) row weights, refused BEFORE the library or a device is touched"""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise L.VmpError('%s: x must be (N,D)' % what)
    if not torch.is_tensor(weights) or tuple(weights.shape) != (x.shape[0],):
        raise L.VmpError('%s: the weights have shape %s, expected %s'
                         % (what, tuple(weights.shape) if torch.is_tensor(weights) else type(weights), (x.shape[0],)))
    if weights.device != x.device:
        raise L.VmpError('%s: the weights are on %s, x on %s' % (what, weights.device, x.device))
    if weights.dtype != torch.float32:
        raise L.VmpError('%s: the weights must be float32 (got %s)' % (what, weights.dtype))


def check_weights(x, weights):
    """The row weights of a weighted fit, checked once (the loop's constructor calls this; a pass never does): shape (N,), fp32, on
    x's device, and - one read-back of three flags - finite, >= 0 and not all zero.  Returns the weights."""
    _weights_dims(x, weights, 'weights')
    flags = torch.stack([torch.isfinite(weights).all(), (weights >= 0).all(), (weights > 0).any()]).tolist()
    if not flags[0]:
        raise L.VmpError('weights: every weight must be finite (found NaN or Inf)')
    if not flags[1]:
        raise L.VmpError('weights: every weight must be >= 0 (found a negative weight)')
    if not flags[2]:
        raise L.VmpError('weights: every weight is zero - nothing to fit')
    return weights


def mixture_wfit_pass(x, weights, pack, miss=None, want_r=True, want_logr=False, want_fill=False, want_stats=True, want_bound=False):
    """One streaming pass (vmp_mixture_wfit_pass) over the rows of x (N,D), their weights (N,) fp32 >= 0 and, if given, their mask
    miss (N,D; nonzero = missing) under a fit pack: (r (N,K), logr (N,K), x_fill (N,D), stats (K, 2+D+D*D) fp64, bound 0-dim fp64);
    outputs that are not wanted are None.  r is the E-step of mixture_fit_pass - a weight does not enter a row's own
    responsibilities; stats are the raw moments [Nk | Wk | sx | sxx] with every row counted w_n times; bound is the data term
    sum_n w_n (logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi) of the lower bound.  A row of weight 0 reaches neither stats nor bound,
    whatever its x holds; its r is that of a held-out row.  miss=None: complete rows, nothing is factored.  want_logr and want_stats
    need want_r, want_fill needs a mask; want_r=False with want_bound is the bound-only form.  The weights are taken as they are
    (check_weights is the loop's business).  stats and bound are the same bits from run to run and for every set of outputs.  No host
    synchronisation."""
    what = 'mixture_wfit_pass'
    N, D, K = _bound_dims(x, miss, pack, what, pack=True)
    _weights_dims(x, weights, what)
    if not (want_r or want_logr or want_fill or want_stats or want_bound):
        raise L.VmpError('%s: no output requested' % what)
    if (want_stats or want_logr) and not want_r:
        raise L.VmpError('%s: want_stats and want_logr need want_r (the moments are those of the r the pass writes)' % what)
    if want_fill and miss is None:
        raise L.VmpError('%s: want_fill needs a mask (a complete row has nothing to fill)' % what)
    x = L.dev_f32(x, 'x')
    dev = x.device
    pack = L.dev_f32(pack, 'pack', (K, L.lib().vmp_mixture_fit_pack_words(D)))
    if pack.device != dev:
        raise L.VmpError('pack is on %s, x on %s' % (pack.device, dev))
    w = L.dev_f32(weights, 'weights', (N,))
    mask = None if miss is None else _mask_u8(miss)
    f32 = dict(dtype=torch.float32, device=dev)
    r = torch.empty(N, K, **f32) if want_r else None
    logr = torch.empty(N, K, **f32) if want_logr else None
    x_fill = torch.empty(N, D, **f32) if want_fill else None
    stats = torch.empty((K, L.lib().vmp_mix_stats_words(D)), dtype=torch.float64, device=dev) if want_stats else None
    bound = torch.empty((), dtype=torch.float64, device=dev) if want_bound else None
    nb = L.lib().vmp_mixture_wfit_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_wfit_pass(L.ptr(x), L.ptr(w), L.ptr(mask), N, D, K, L.ptr(pack), L.ptr(r), L.ptr(logr), L.ptr(x_fill),
                                          L.ptr(stats), L.ptr(bound), L.ptr(ws), nb, L.stream()), 'vmp_mixture_wfit_pass')
    return r, logr, x_fill, stats, bound


def weighted_mean_filled(x, mask, w):
    """The copy of x a weighted loop takes the moments of r_init from: a missing entry (mask (N,D) or None) holds its column's
    weighted mean over the observed entries of the rows that count (sum_n w_n x_nd / sum_n w_n; 0 for a column with none) - with
    integer weights the fill mean_filled gives on the replicated rows - and a row of weight 0 is all zeros, so that what it holds
    (NaN included) cannot reach 0 * x."""
    drop = (w == 0)[:, None]
    gone = drop.expand_as(x) if mask is None else ((mask != 0) | drop)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    if mask is None:
        return torch.where(gone, zero, x).contiguous()
    wd = torch.where(gone, torch.zeros((), dtype=torch.float64, device=x.device), w.double()[:, None].expand_as(x))
    num = (torch.where(gone, zero, x).double() * wd).sum(0)
    den = wd.sum(0)
    mean = torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num)).to(x.dtype)
    out = torch.where(mask != 0, mean[None, :].expand_as(x), x)
    return torch.where(drop, zero, out).contiguous()


def mean_filled(x, mask):
    """x with every missing entry replaced by its column's mean over the observed entries (0 for a column with none): the copy the
    masked loop takes the moments of r_init from."""
    gone = mask != 0
    mean = _observed_mean(x, gone)
    return torch.where(gone, mean[None, :].expand_as(x), x).contiguous()


def _observed_mean(x, gone):
    """(D,) column means of x over the entries that `gone` (N,D) bool does not flag (0 for a column with none), in x's dtype"""
    xz = torch.where(gone, torch.zeros((), dtype=x.dtype, device=x.device), x)
    cnt = (~gone).sum(0)
    return (xz.double().sum(0) / cnt.clamp_min(1).double()).to(x.dtype)


def _seed_operands(x, miss, K, what):
    """(x fp32 on the device, uint8 mask or None) of a seeding call: shapes and devices are refused BEFORE the library or a device is
    touched, CPU tensors by the operand check"""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1:
        raise L.VmpError('%s: x must be (N >= 1, D), got %s' % (what, tuple(x.shape) if torch.is_tensor(x) else type(x)))
    if miss is not None:
        if not torch.is_tensor(miss) or tuple(miss.shape) != tuple(x.shape):
            raise L.VmpError('%s: the missing-data mask has shape %s, expected %s'
                             % (what, tuple(miss.shape) if torch.is_tensor(miss) else type(miss), tuple(x.shape)))
        if miss.device != x.device:
            raise L.VmpError('%s: the missing-data mask is on %s, x on %s' % (what, miss.device, x.device))
    _dims(x, K)
    x = L.dev_f32(x, 'x')
    return x, (None if miss is None else _mask_u8(miss))


def seed_centers(x, K, seed, miss=None, want_index=False, want_mind2=False):
    """K seeded k-means++ centres (D^2-seeding) from the rows of x (N,D) on the device (vmp_mixture_seed_centers; include/vmp_hip.h
    "Mixture initialisation"): (centers (K,D), index (K,) int64 or None, mind2 (N,) or None) - the chosen rows and every row's squared
    distance to its nearest centre.  A pure function of (seed, row index, round): the same bits from run to run.  miss (N,D),
    nonzero = missing, on x's device: distances run over the observed coordinates (scaled by D / D_o), a row with none is never
    chosen, and a centre takes its column's mean over the observed entries - the fill of mean_filled - where its row has a gap.
    K + 1 launches enqueued by one call, no host synchronisation."""
    K, seed = int(K), int(seed)
    if not 0 <= seed < 1 << 64:
        raise L.VmpError('seed must be in 0 .. 2^64 - 1 (got %d)' % seed)
    x, mask = _seed_operands(x, miss, K, 'seed_centers')
    N, D = x.shape
    dev = x.device
    fill = None if mask is None else _observed_mean(x, mask != 0).contiguous()
    centers = torch.empty(K, D, dtype=torch.float32, device=dev)
    index = torch.empty(K, dtype=torch.int64, device=dev) if want_index else None
    mind2 = torch.empty(N, dtype=torch.float32, device=dev) if want_mind2 else None
    nb = L.lib().vmp_mixture_seed_workspace_bytes(N, D, K)
    ws = L.workspace(dev, nb)
    L.check(L.lib().vmp_mixture_seed_centers(L.ptr(x), L.ptr(mask), L.ptr(fill), N, D, K, seed, L.ptr(centers), L.ptr(index),
                                             L.ptr(mind2), L.ptr(ws), nb, L.stream()), 'vmp_mixture_seed_centers')
    return centers, index, mind2


def seed_assign(x, centers, miss=None, smooth=0.0, want_z=False):
    """Responsibilities of the nearest centre (vmp_mixture_seed_assign): (r (N,K), z (N,) int32 or None) with z_n the nearest of
    centers (K,D) by the distance of seed_centers (ties to the lowest k) and r_nk = (1 - smooth) [k = z_n] + smooth / K,
    0 <= smooth < 1; a row without an observed entry gets z = -1 and r = 1 / K.  One streaming launch, no host synchronisation."""
    smooth = float(smooth)
    if not 0.0 <= smooth < 1.0:
        raise L.VmpError('smooth must be in [0, 1) (got %r)' % smooth)
    if not torch.is_tensor(x) or x.dim() != 2:
        raise L.VmpError('seed_assign: x must be (N,D)')
    if not torch.is_tensor(centers) or centers.dim() != 2 or centers.shape[1] != x.shape[1]:
        raise L.VmpError('seed_assign: centers has shape %s, expected (K,%d)'
                         % (tuple(centers.shape) if torch.is_tensor(centers) else type(centers), x.shape[1]))
    if centers.device != x.device:
        raise L.VmpError('seed_assign: centers is on %s, x on %s' % (centers.device, x.device))
    K = centers.shape[0]
    x, mask = _seed_operands(x, miss, K, 'seed_assign')
    N, D = x.shape
    centers = L.dev_f32(centers, 'centers', (K, D))
    r = torch.empty(N, K, dtype=torch.float32, device=x.device)
    z = torch.empty(N, dtype=torch.int32, device=x.device) if want_z else None
    L.check(L.lib().vmp_mixture_seed_assign(L.ptr(x), L.ptr(mask), N, D, K, L.ptr(centers), smooth, L.ptr(r), L.ptr(z), L.stream()),
            'vmp_mixture_seed_assign')
    return r, z


INITS = ('random', 'kmeans++')


def check_init(init):
    """the `init` keyword of gmm.inference / gmm.inference_missing / smm.inference, refused on the host"""
    if init not in INITS:
        raise L.VmpError('init=%r: expected one of %s' % (init, ', '.join(repr(i) for i in INITS)))
    return init


def seeded_r_init(x, K, seed, miss=None, smooth=0.0):
    """r_init (N,K) of init='kmeans++': seed_centers, then seed_assign - on the device, no host synchronisation"""
    centers, _, _ = seed_centers(x, K, seed, miss=miss)
    return seed_assign(x, centers, miss=miss, smooth=smooth)[0]


def default_prior(K, D, device):
    """The prior gmm.inference / smm.inference hard-code (reference gmm.py:252-256): init_mm_params(K, D,
    alpha_scale=0.05/K, beta_scale=0.5, m_scale=0, C_scale=D+0.5, v_init=D+0.5), in standard form."""
    f32 = dict(dtype=torch.float32, device=device)
    alpha_0 = torch.full((K,), 0.05 / K, **f32)
    beta_0 = torch.full((K,), 0.5, **f32)
    m_0 = torch.zeros(K, D, **f32)
    C_0 = (D + 0.5) * torch.eye(D, **f32).expand(K, D, D).contiguous()
    v_0 = torch.full((K,), float(D + D + 0.5), **f32)
    return alpha_0, beta_0, m_0, C_0, v_0


class VMPLoop(object):
    """The iteration `sess.run(step)` drives in the reference (gmm.py:258-263 / smm.py:232-238):
    M-step from the current (r, u) -> E-step -> assign.  One iteration is TWO launches:
      vmp_mix_finalize_ws  (K blocks)   reduce the per-block fp64 partial moments + posterior + E-step pack
      vmp_mix_estep_fused  (streaming)  E-pass that also accumulates the raw moments of ITS OWN output,
    which are exactly the M-pass input of the next iteration; only the very first iteration needs a
    stand-alone M-pass (vmp_mix_stats_ws).
    Nothing inside an iteration reads r or u: the finalize launch takes the partial moments, the next pass forms r again from x and
    the new pack.  stream_phase() and all but the last iteration of a run() therefore go through vmp_mixture_estep_fused_nostore / vmp_mixture_iterate_nostore, whose
    kernel writes the partials alone (where the fused pass has the XDL form, K <= 16; elsewhere, and for accurate=, miss=, weights=
    and a log r request, the storing calls as before), and `r` / `u` are properties: read after such a pass, they first run ONE
    E-only pass (vmp_mix_estep: the bits the fused pass would have stored) from the current pack into the loop's own two buffers -
    the same tensors on every read, nothing launched on a second read.  That is the r of the last pass as long as no finalize has
    moved the pack on since: read between finalize_phase() and stream_phase(), it is the r of the NEW pack, while `stats` and the
    workspace still describe the last pass.  step() hands r back on every call, so it keeps the storing pass, and the LAST iteration of
    a run() is the storing pass as well: r is current when either returns, and neither ever costs more launches than before.
    accurate=True (round 6, opt-in): the E-part runs entirely in fp64 from an fp64 copy of the pack (vmp_mix_finalize_ws64 +
    vmp_mix_estep_accurate) and the moments of its output come from a separate fp64 M-pass (vmp_mix_stats_ws_accurate): three launches
    per iteration instead of one.  It is what meets the stated 1e-5 on the SMM's responsibilities at C5 (whose log rho is linear in
    the Mahalanobis distance with a factor (D + kappa) / 2 and reaches 1e2..1e3: beyond fp32); the default stays the fused pass.
    (A one-launch form of the iteration - posterior in the heads of the streaming launch - was built and measured in round 5:
    bit-identical and no faster; removed in round 6.)
    miss=mask (GMM only; (N,D) on x's device, nonzero = missing): the fit on partly observed rows, the missing entries being latent
    variables of the posterior (include/vmp_hip.h "Mixture fitting on partly observed rows").  An iteration is vmp_mix_finalize on
    the (K, stats words) moments of the completed rows, vmp_mixture_fit_pack, and the streaming vmp_mixture_fit_pass with its
    fixed-order reduction; run() enqueues them through vmp_mixture_fit_iterate.  filled() returns x with its gaps filled.  miss=None
    is the loop described above, unchanged.
    weights=w (GMM only; (N,) fp32 on x's device, finite, >= 0, not all zero - check_weights, one read-back, here and nowhere else):
    row n counts as w_n identical rows (include/vmp_hip.h "Mixture fitting on weighted rows") - counts of binned data, coresets,
    importance weights, and 0/1 folds over the same resident x.  A row of weight 0 is held out: it reaches nothing the fit adds up,
    whatever it holds, and its r is what the E-step gives.  An iteration is vmp_mix_finalize -> vmp_mixture_fit_pack ->
    vmp_mixture_wfit_pass, with or without miss=; run() goes through vmp_mixture_wfit_iterate; the pass leaves the data term of the
    lower bound behind, so lower_bound() costs one K-sized launch and no further pass over x.  weights=None is today's code path."""

    def __init__(self, x, r_init, flavour, kappa=None, u_init=None, prior=None, accurate=False, miss=None, weights=None):
        self.miss = None
        self.w = None
        if weights is not None:
            self._check_weighted(x, weights, flavour, accurate)        # before the device is touched
        if miss is not None:
            self._check_miss(x, miss, flavour, accurate)               # before the device is touched
        self.x = L.dev_f32(x, 'x')
        self.N, self.D = self.x.shape
        self.K = K = r_init.shape[1]
        _dims(self.x, K)
        dev = self.x.device
        self.flavour = flavour
        self.kappa = None if kappa is None else L.dev_f32(kappa.to(dev, torch.float32), 'kappa', (K,))
        prior = prior if prior is not None else default_prior(K, self.D, dev)
        self.prior = _prior(prior, K, self.D, dev)
        self._r = L.dev_f32(r_init, 'r_nk', (self.N, K)).clone()
        self._u = None
        if flavour == L.VMP_SMM:
            self._u = (torch.ones_like(self._r) if u_init is None else L.dev_f32(u_init, 'u_nk', (self.N, K)).clone())
        D = self.D
        self.post = _post_buffers(K, D, dev)
        self.logr = None
        self.accurate = bool(accurate)
        self.iterations = 0
        self.pack64 = None
        self._stale = False              # self._r / self._u are behind the pack: a no-store pass ran since they were written
        self._nostore = False            # stream_phase() / run() go through the pass that stores no r / u
        if weights is not None:
            self._init_weighted(weights, miss)
            return
        if miss is not None:
            self._init_masked(miss)
            return
        self.nb = L.lib().vmp_mix_workspace_bytes(self.N, D, K)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=dev)      # private: partials live across calls
        self.pivot = pivot_of(self.x)                                     # once per dataset
        seed_fn = L.lib().vmp_mix_stats_ws_accurate if self.accurate else L.lib().vmp_mix_stats_ws
        L.check(seed_fn(L.ptr(self.x), L.ptr(self._r), L.ptr(self._u), L.ptr(self.pivot), self.N, D, K,
                        L.ptr(self.ws), self.nb, L.stream()), 'vmp_mix_stats_ws')
        self.pack64 = torch.empty(K, L.lib().vmp_mix_pack_words(D), dtype=torch.float64, device=dev) if self.accurate else None
        self._nostore = not self.accurate and self._has_nostore()

    def _has_nostore(self):
        """the fused pass of this loop has an instance without r / u stores: the XDL form (a host query, vmp_mix_pass_plan), in a
        library that has the entry point (an older build selected with VMP_LIB_PATH for an A/B measurement may not)"""
        import ctypes
        if not hasattr(L.lib(), 'vmp_mixture_estep_fused_nostore'):
            return False
        plan = (ctypes.c_int64 * 8)()
        L.check(L.lib().vmp_mix_pass_plan(self.N, self.D, self.K, self.flavour, 1, 1, 0, plan), 'vmp_mix_pass_plan')
        return plan[0] == 2

    def _fresh(self):
        """self._r / self._u hold the r / u of the current pack: after a pass that stored none, one E-only pass (with the loop's
        pivot: the pivot enters the rounding of the E-part) into the same buffers"""
        if self._stale:
            L.check(L.lib().vmp_mix_estep(L.ptr(self.x), self.N, self.D, self.K, self.flavour, L.ptr(self.post['pack']), None,
                                          L.ptr(self._r), L.ptr(self._u), None, L.ptr(self.pivot), None, None, 0, L.stream()),
                    'vmp_mix_estep')
            self._stale = False

    @property
    def r(self):
        self._fresh()
        return self._r

    @property
    def u(self):
        self._fresh()
        return self._u

    @classmethod
    def from_seed(cls, x, K, flavour, seed, kappa=None, prior=None, accurate=False, miss=None, smooth=0.0):
        """The loop started from the data: r_init = seed_assign on the K centres of seed_centers(x, K, seed) - k-means++ on the
        device, a pure function of (x, miss, K, seed) - instead of responsibilities the caller has to invent.  The refusals of the
        constructor come first."""
        if miss is not None:
            cls._check_miss(x, miss, flavour, accurate)
        r0 = seeded_r_init(x, K, seed, miss=miss, smooth=smooth)
        return cls(x, r0, flavour, kappa=kappa, prior=prior, accurate=accurate, miss=miss)

    @classmethod
    def from_seed_weighted(cls, x, weights, K, flavour, seed, prior=None, accurate=False, miss=None, smooth=0.0):
        """from_seed() for a weighted loop (its signature is pinned by the seeding tests, hence a method of its own).  The weights go
        to the loop only: the k-means++ seeding itself is unweighted in this version - every row of x, those of weight 0 included, can
        become a centre with the probability its distance gives it - so x must be finite in its observed slots throughout.  The
        refusals of the constructor come first, the value check of the weights included: nothing is seeded from weights that the
        constructor would refuse (it checks them again: two scalar read-backs on this path)."""
        cls._check_weighted(x, weights, flavour, accurate)
        if miss is not None:
            cls._check_miss(x, miss, flavour, accurate)
        r0 = seeded_r_init(x, K, seed, miss=miss, smooth=smooth)
        return cls(x, r0, flavour, prior=prior, accurate=accurate, miss=miss, weights=weights)

    @staticmethod
    def _check_miss(x, miss, flavour, accurate):
        """the refusals of a masked loop, on the host: nothing here looks at a device"""
        if flavour != L.VMP_GMM:
            raise L.VmpError('miss= is for the Gaussian mixture (VMP_GMM): the Student-t mixture on partly observed rows needs the joint '
                             'q(u, x_m | k) and is not implemented')
        if accurate:
            raise L.VmpError('miss= and accurate=True do not combine: the masked pass has no fp64 form')
        if not torch.is_tensor(x) or x.dim() != 2:
            raise L.VmpError('x must be (N,D)')
        if not torch.is_tensor(miss) or tuple(miss.shape) != tuple(x.shape):
            raise L.VmpError('the missing-data mask has shape %s, expected %s' % (tuple(miss.shape) if torch.is_tensor(miss) else type(miss),
                                                                                 tuple(x.shape)))
        if miss.device != x.device:
            raise L.VmpError('the missing-data mask is on %s, x on %s' % (miss.device, x.device))

    @staticmethod
    def _check_weighted(x, weights, flavour, accurate, values=True):
        """the refusals of a weighted loop, on the host; the value check of the weights is the one read-back (check_weights);
        values=False: shape, dtype and device only"""
        if flavour != L.VMP_GMM:
            raise L.VmpError('weights= is for the Gaussian mixture (VMP_GMM): the Student-t mixture has no weighted pass')
        if accurate:
            raise L.VmpError('weights= and accurate=True do not combine: the weighted pass has no fp64 form')
        if values:
            check_weights(x, weights)
        else:
            _weights_dims(x, weights, 'weights')

    def _init_weighted(self, weights, miss):
        """State of the loop on weighted rows, like the masked one: the moments live in self._stats (K, stats words) fp64 - seeded
        here by vmp_mix_stats from r_init * w (the moments are linear in r) on weighted_mean_filled(x, miss, w) - and every iteration is
        vmp_mix_finalize -> vmp_mixture_fit_pack -> vmp_mixture_wfit_pass (csrc/vmp_wfit.hip), which also leaves the data term of the
        lower bound in self._data."""
        dev, N, D, K = self.x.device, self.N, self.D, self.K
        self.w = L.dev_f32(weights, 'weights', (N,))
        self.miss = None if miss is None else _mask_u8(miss)
        keep = (self.w != 0)[:, None]
        rw = torch.where(keep, self._r * self.w[:, None], torch.zeros((), dtype=torch.float32, device=dev))
        self._stats = raw_stats(weighted_mean_filled(self.x, self.miss, self.w), rw)
        self.fpack = torch.empty(K, L.lib().vmp_mixture_fit_pack_words(D), dtype=torch.float32, device=dev)
        self.x_fill = None if miss is None else torch.empty_like(self.x)
        self._data = torch.empty((), dtype=torch.float64, device=dev)
        self.nb = L.lib().vmp_mixture_wfit_workspace_bytes(N, D, K)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=dev)
        self.pivot = None

    def _init_masked(self, miss):
        """State of the loop on partly observed rows: the moments live in self._stats (K, stats words) fp64 - seeded here from r_init
        on a copy of x whose missing entries hold their column's observed mean, no covariance term - and every iteration is
        vmp_mix_finalize -> vmp_mixture_fit_pack -> vmp_mixture_fit_pass (csrc/vmp_missfit.hip)."""
        dev, N, D, K = self.x.device, self.N, self.D, self.K
        self.miss = _mask_u8(miss)
        self._stats = raw_stats(mean_filled(self.x, self.miss), self._r)
        self.fpack = torch.empty(K, L.lib().vmp_mixture_fit_pack_words(D), dtype=torch.float32, device=dev)
        self.x_fill = torch.empty_like(self.x)
        self.nb = L.lib().vmp_mixture_fit_workspace_bytes(N, D, K)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=dev)
        self.pivot = None

    def _fin_ptrs(self, post=True):
        """(ws, pivot, N, D, K, flavour, prior x 5, kappa, posterior x 9): the leading arguments of vmp_mix_finalize_ws / _ws64 /
        _exchange; post=False: no posterior output (the reduction-only form).  [3:] is what vmp_mix_finalize takes behind its stats."""
        return [L.ptr(self.ws), L.ptr(self.pivot), self.N] + _fin_tail(self.D, self.K, self.flavour, self.prior, self.kappa,
                                                                      self.post if post else None)

    def finalize(self, stats_out=None):
        if self.miss is not None or self.w is not None:
            L.check(L.lib().vmp_mix_finalize(L.ptr(self._stats), *_fin_tail(self.D, self.K, self.flavour, self.prior, None, self.post),
                                             L.stream()), 'vmp_mix_finalize')
            p = self.post
            L.check(L.lib().vmp_mixture_fit_pack(self.D, self.K, L.ptr(p['alpha']), L.ptr(p['beta']), L.ptr(p['m']), L.ptr(p['C']),
                                                 L.ptr(p['v']), L.ptr(self.fpack), L.stream()), 'vmp_mixture_fit_pack')
            return
        if self.accurate:
            L.check(L.lib().vmp_mix_finalize_ws64(*self._fin_ptrs(), L.ptr(self.pack64), L.ptr(stats_out), L.stream()), 'vmp_mix_finalize_ws64')
            return
        L.check(L.lib().vmp_mix_finalize_ws(*self._fin_ptrs(), L.ptr(stats_out), L.stream()), 'vmp_mix_finalize_ws')

    def finalize_phase(self):
        """everything of an iteration that is not the streaming launch (bench.py brackets that launch with events): the finalize launch"""
        self.finalize()

    def estep(self, want_logr=False):
        """E-pass with fused moments on the current pack (the second launch of an iteration)"""
        if want_logr and self.logr is None:
            self.logr = torch.empty_like(self._r)
        if self.w is not None:
            L.check(L.lib().vmp_mixture_wfit_pass(L.ptr(self.x), L.ptr(self.w), L.ptr(self.miss), self.N, self.D, self.K, L.ptr(self.fpack),
                                                  L.ptr(self._r), L.ptr(self.logr if want_logr else None), L.ptr(self.x_fill),
                                                  L.ptr(self._stats), L.ptr(self._data), L.ptr(self.ws), self.nb, L.stream()),
                    'vmp_mixture_wfit_pass')
            return
        if self.miss is not None:
            L.check(L.lib().vmp_mixture_fit_pass(L.ptr(self.x), L.ptr(self.miss), self.N, self.D, self.K, L.ptr(self.fpack), L.ptr(self._r),
                                                 L.ptr(self.logr if want_logr else None), L.ptr(self.x_fill), L.ptr(self._stats),
                                                 L.ptr(self.ws), self.nb, L.stream()), 'vmp_mixture_fit_pass')
            return
        if self.accurate:
            L.check(L.lib().vmp_mix_estep_accurate(L.ptr(self.x), self.N, self.D, self.K, self.flavour, L.ptr(self.pack64), L.ptr(self._r),
                                                   L.ptr(self._u), L.ptr(self.logr if want_logr else None), L.stream()), 'vmp_mix_estep_accurate')
            L.check(L.lib().vmp_mix_stats_ws_accurate(L.ptr(self.x), L.ptr(self._r), L.ptr(self._u), L.ptr(self.pivot), self.N, self.D,
                                                      self.K, L.ptr(self.ws), self.nb, L.stream()), 'vmp_mix_stats_ws_accurate')
            return
        L.check(L.lib().vmp_mix_estep_fused(L.ptr(self.x), self.N, self.D, self.K, self.flavour, L.ptr(self.post['pack']),
                                            L.ptr(self._r), L.ptr(self._u), L.ptr(self.logr if want_logr else None),
                                            L.ptr(self.pivot), L.ptr(self.ws), self.nb, L.stream()), 'vmp_mix_estep_fused')
        self._stale = False

    def stream_phase(self, want_logr=False):
        """the streaming launch of an iteration: the E-pass with the moments of its own output - which it does not write out where a
        kernel without the r / u stores exists and no log r is asked for (`r` / `u` catch up when they are read)"""
        if want_logr or not self._nostore:
            self.estep(want_logr)
            return
        L.check(L.lib().vmp_mixture_estep_fused_nostore(L.ptr(self.x), self.N, self.D, self.K, self.flavour, L.ptr(self.post['pack']),
                                                        L.ptr(self.pivot), L.ptr(self.ws), self.nb, L.stream()),
                'vmp_mixture_estep_fused_nostore')
        self._stale = True

    def step(self, want_logr=False):
        """one iteration; returns its r - which is why the pass here is the storing one"""
        self.finalize_phase()
        self.estep(want_logr)
        self.iterations += 1
        return self._r

    def run(self, iterations):
        """`iterations` VMP iterations enqueued without host work between the launches (vmp_mix_iterate; where the pass has an instance
        without r / u stores, vmp_mixture_iterate_nostore for all but the last of them).  Returns r."""
        if self.accurate:
            for _ in range(int(iterations)):
                self.step()
            return self._r
        if self.w is not None:
            p = self.post
            L.check(L.lib().vmp_mixture_wfit_iterate(L.ptr(self.x), L.ptr(self.w), L.ptr(self.miss), self.N, self.D, self.K,
                                                     *[L.ptr(t) for t in self.prior], L.ptr(self._r), None, L.ptr(self.x_fill),
                                                     *[L.ptr(p[k]) for k in _POST[:8]], L.ptr(self.fpack), L.ptr(self._stats),
                                                     L.ptr(self._data), L.ptr(self.ws), self.nb, int(iterations), L.stream()),
                    'vmp_mixture_wfit_iterate')
            self.iterations += int(iterations)
            return self._r
        if self.miss is not None:
            p = self.post
            L.check(L.lib().vmp_mixture_fit_iterate(L.ptr(self.x), L.ptr(self.miss), self.N, self.D, self.K, *[L.ptr(t) for t in self.prior],
                                                    L.ptr(self._r), None, L.ptr(self.x_fill), *[L.ptr(p[k]) for k in _POST[:8]],
                                                    L.ptr(self.fpack), L.ptr(self._stats), L.ptr(self.ws), self.nb, int(iterations),
                                                    L.stream()), 'vmp_mixture_fit_iterate')
            self.iterations += int(iterations)
            return self._r
        ws, pivot, *f = self._fin_ptrs()                       # f = N, D, K, flavour, prior x 5, kappa | posterior x 9
        n = int(iterations)
        if self._nostore and n > 1:
            # all but the last iteration without the r / u stores; the last one stores them, so that r is current when the call
            # returns and no E-only pass is ever launched for it (run_until* call run() every few iterations)
            L.check(L.lib().vmp_mixture_iterate_nostore(L.ptr(self.x), *f[:10], pivot, *f[10:], ws, self.nb, n - 1, L.stream()),
                    'vmp_mixture_iterate_nostore')
            self.iterations += n - 1
            n = 1
        L.check(L.lib().vmp_mix_iterate(L.ptr(self.x), *f[:10], pivot, L.ptr(self._r), L.ptr(self._u), *f[10:], ws, self.nb, n, L.stream()),
                'vmp_mix_iterate')
        self.iterations += n
        if n > 0:
            self._stale = False
        return self.r

    def score_pack(self):
        """Score pack of the CURRENT posterior (self.post: needs one iteration).  GMM: the posterior predictive (score_pack_niw); SMM: the plug-in Student-t mixture with mu = m_k,
        sigma = C_k / v_k, nu = kappa, log_w = log(alpha_k / sum alpha) (score_pack_t; see smm.heldout_logprob)."""
        if self.iterations == 0:
            raise L.VmpError('no posterior to score yet: run at least one iteration')
        al, be, m, C, v = self.theta()
        if self.flavour == L.VMP_SMM:
            return score_pack_t(torch.log(al / al.sum()), m, C / v[:, None, None], self.kappa)
        return score_pack_niw(al, be, m, C, v)

    def score(self, x_val):
        """Mean log score (nats per row) of the rows of x_val (M,D) under the current posterior: the GMM's log posterior
        predictive density, the SMM's plug-in log density.  One streaming launch over x_val, one scalar read-back."""
        x_val = L.dev_f32(x_val, 'x_val')
        if x_val.dim() != 2 or x_val.shape[1] != self.D or x_val.shape[0] < 1:
            raise L.VmpError('x_val has shape %s, expected (M >= 1, %d)' % (tuple(x_val.shape), self.D))
        _, _, total = mixture_score(x_val, self.score_pack(), want_logp=False)
        return total.item() / x_val.shape[0]

    def impute_pack(self):
        """Impute pack of the CURRENT posterior: the mixture score_pack() scores (GMM: impute_pack_niw; SMM: impute_pack_t)."""
        if self.iterations == 0:
            raise L.VmpError('no posterior to impute from yet: run at least one iteration')
        al, be, m, C, v = self.theta()
        if self.flavour == L.VMP_SMM:
            return impute_pack_t(torch.log(al / al.sum()), m, C / v[:, None, None], self.kappa)
        return impute_pack_niw(al, be, m, C, v)

    def impute(self, x_new, miss):
        """(x_filled (M,D), logp (M,)) of the partly observed rows x_new (M,D) with mask miss (M,D; nonzero = missing) under the current
        posterior - gmm.predictive_impute / smm.heldout_impute on theta().  One streaming launch, no host synchronisation."""
        if self.iterations == 0:
            raise L.VmpError('no posterior to impute from yet: run at least one iteration')
        if not torch.is_tensor(x_new) or x_new.dim() != 2 or x_new.shape[1] != self.D or x_new.shape[0] < 1:
            raise L.VmpError('x_new has shape %s, expected (M >= 1, %d)' % (tuple(x_new.shape) if torch.is_tensor(x_new) else type(x_new), self.D))
        _impute_dims(x_new, miss, self.post['m'], 'impute')
        x_out, logp, _, _ = mixture_impute(x_new, miss, self.impute_pack())
        return x_out, logp

    def sample(self, n, seed, want_z=False):
        """n seeded rows (n,D) from the mixture impute() fills from - the GMM's posterior predictive, the SMM's plug-in mixture - of the
        current posterior (mixture_draw on impute_pack()); with want_z also the component of each row.  One streaming launch, no host
        synchronisation."""
        x, z = mixture_draw(n, self.impute_pack(), seed, want_z=want_z)
        return (x, z) if want_z else x

    def impute_draws(self, x_new, miss, draws, seed, want_z=False):
        """`draws` completed copies (draws,M,D) of the partly observed rows x_new (M,D) with mask miss (M,D; nonzero = missing), their
        missing entries drawn from p(x_missing | x_observed) under the current posterior (mixture_sample on impute_pack()) - multiple
        imputation, where impute() returns the conditional mean; with want_z also the (draws,M) components.  One streaming launch,
        no host synchronisation."""
        if self.iterations == 0:
            raise L.VmpError('no posterior to impute from yet: run at least one iteration')
        if not torch.is_tensor(x_new) or x_new.dim() != 2 or x_new.shape[1] != self.D or x_new.shape[0] < 1:
            raise L.VmpError('x_new has shape %s, expected (M >= 1, %d)' % (tuple(x_new.shape) if torch.is_tensor(x_new) else type(x_new), self.D))
        _impute_dims(x_new, miss, self.post['m'], 'impute_draws')
        x, z = mixture_sample(x_new, miss, self.impute_pack(), seed, draws=draws, want_z=want_z)
        return (x, z) if want_z else x

    def run_until(self, x_val, tol, check_every=5, max_iterations=1000):
        """run(check_every) and score(x_val) in turn until the score improves by less than `tol` (absolute, nats per row) over
        the previous check, or `max_iterations` iterations of this call are done.  Returns [(iterations, score), ...] with
        `iterations` the loop's running count.  A plain host loop: one scalar read-back per check."""
        return L.check_until(self, lambda: self.score(x_val), lambda v, prev: v - prev < tol, check_every, max_iterations)

    def _check_bound(self, need_posterior):
        """the refusals of lower_bound() / run_until_bound(), on the host: nothing here looks at a device"""
        if self.flavour != L.VMP_GMM:
            raise L.VmpError('the lower bound is for the Gaussian mixture (VMP_GMM): the Student-t E-step of the reference is not the '
                             'E-step of a bound')
        if need_posterior and self.iterations == 0:
            raise L.VmpError('no posterior to bound yet: run at least one iteration')

    def lower_bound(self):
        """The variational lower bound (free energy, nats) of the current posterior on the loop's own x, mask and prior - the state
        step() leaves: theta from the M-step, r from the E-step at that theta (lower_bound() above).  Plain, masked and accurate=True
        Gaussian loops; the pass is the fp32 one in all three.  Two K-sized launches, one streaming launch over x with its one-wave
        sum, one scalar read-back.  A weighted loop: the weighted data term its own pass wrote, minus the same two KL terms."""
        self._check_bound(True)
        if self.w is not None:          # the pass of the last iteration left its data term: one K-sized launch, no pass over x
            terms = bound_terms(self.prior, self.theta())
            return (self._data - (terms[0] + terms[1])).item()
        return lower_bound(self.x, self.theta(), prior=self.prior, miss=self.miss).item()

    def run_until_bound(self, tol, check_every=5, max_iterations=1000):
        """run(check_every) and lower_bound() in turn until the bound improves by less than tol * max(1, |bound|) over the previous
        check, or `max_iterations` iterations of this call are done - convergence on the quantity the loop optimises, without
        held-out rows.  Returns [(iterations, bound), ...] with `iterations` the loop's running count, as run_until does.  A plain
        host loop: one scalar read-back per check."""
        self._check_bound(False)
        return L.check_until(self, self.lower_bound, lambda v, prev: v - prev < tol * max(1.0, abs(v)), check_every, max_iterations)

    @property
    def stats(self):
        """Raw moments of the current r (reduces the partials the last pass left in the workspace; a masked loop keeps them
        reduced: the moments of the completed rows, conditional covariances included)."""
        if self.miss is not None or self.w is not None:
            return self._stats.clone()
        st = torch.empty((self.K, L.lib().vmp_mix_stats_words(self.D)), dtype=torch.float64, device=self.x.device)
        keep = {k: v.clone() for k, v in self.post.items()}
        self.finalize(stats_out=st)
        for k, v in keep.items():
            self.post[k].copy_(v)
        return st

    def filled(self):
        """x with its missing entries replaced by sum_k r_nk E_q[x_m | k] under the factor of the last iteration (observed entries
        carry the bits of x).  Masked loops only; needs one iteration."""
        if self.miss is None:
            raise L.VmpError('filled() is for a loop built with miss=')
        if self.iterations == 0:
            raise L.VmpError('nothing filled in yet: run at least one iteration')
        return self.x_fill

    def theta(self):
        p = self.post
        return p['alpha'], p['beta'], p['m'], p['C'], p['v']

    def aux(self):
        p = self.post
        return p['xbar'], p['S'], p['pi']


# the diagonal-covariance mixture on wide rows (D up to 64) lives in models/_diag.py; its entry points are reachable from here as well
from ._diag import (DiagFitLoop, DiagLoop, default_diag_prior, diag_bound_terms, diag_finalize, diag_lower_bound,  # noqa: E402,F401
                    diag_mfit_pack, diag_pack, diag_predictive_impute, diag_predictive_logprob, diag_score_pack, diag_seed_assign,
                    diag_seed_centers, mixture_diag_mfit_pass, mixture_diag_pass, mixture_diag_score, nearest_center_r,
                    observed_column_means)
