"""Multivariate Student-t log-density - mirror of reference distributions/student_t.py."""


def log_probability_per_samp(y, mu, sigma, v, name='student_t_logprob_per_samp'):
    """reference student_t.py:7-39,59-61: y (N,K,S,D), mu (K,D), sigma (K,D,D), v (K) -> (N,K,S).
    HIP kernel: vmp_student_t_logprob (K distinct scale matrices are factorised once, not N*K*S times)."""
    from ..models import _svae_ops
    return _svae_ops.student_t_logprob(y, mu, sigma, v)


def _logprob_full_scale(y, mu, sigma, v, name='student_t_logprob'):
    """reference student_t.py:7-39 (the function log_probability_per_samp forwards to)."""
    return log_probability_per_samp(y, mu, sigma, v, name)


def logprob_smm_mixture(y, mu, sigma, v, log_pi, name='student_t_logprob'):
    """reference student_t.py:42-56: y (N,D) -> (N,K) log S(y_n | mu_k, sigma_k, v_k) + log pi_k."""
    N, D = y.shape
    K = mu.shape[0]
    yk = y[:, None, None, :].expand(N, K, 1, D).contiguous()
    return log_probability_per_samp(yk, mu, sigma, v).reshape(N, K) + log_pi[None, :]


def mixture_logprob(y, mu, sigma, v, log_pi, return_resp=False):
    """log sum_k pi_k S(y_n | mu_k, sigma_k, v_k): y (N,D) -> (N,), equal to logsumexp(logprob_smm_mixture(...), dim=1)
    (reference student_t.py:42-56 followed by the log-sum-exp its caller takes) without the (N,K,1,D) expansion or the (N,K)
    intermediate: one streaming HIP pass over y (vmp_mix_score_pack_t + vmp_mix_score).  return_resp=True also returns the
    (N,K) responsibilities exp(term_nk - logp_n)."""
    from ..models import _mix
    _mix._score_dims(y, mu, 'mixture_logprob')
    pack = _mix.score_pack_t(log_pi, mu, sigma, v)
    logp, resp, _ = _mix.mixture_score(y, pack, want_resp=return_resp, want_sum=False)
    return (logp, resp) if return_resp else logp


def mixture_impute(y, miss, mu, sigma, v, log_pi, return_resp=False):
    """Conditional means of the missing entries of y (N,D) - miss (N,D), nonzero = missing - under the mixture
    sum_k pi_k S(. | mu_k, sigma_k, v_k): (y_filled (N,D), logp (N,)) with logp the marginal log density of each row's observed
    entries, plus the (N,K) responsibilities exp(term_nk - logp_n) with return_resp=True.  For v_k <= 1 a Student-t has no mean; the
    component's conditional location mu_m + sigma_mo sigma_oo^-1 (y_o - mu_o) is used either way.  One streaming HIP pass
    (vmp_mixture_impute_pack_t + vmp_mixture_impute)."""
    from ..models import _mix
    _mix._impute_dims(y, miss, mu, 'mixture_impute')
    pack = _mix.impute_pack_t(log_pi, mu, sigma, v)
    y_out, logp, resp, _ = _mix.mixture_impute(y, miss, pack, want_resp=return_resp)
    return (y_out, logp, resp) if return_resp else (y_out, logp)


def mixture_sample(n, seed, mu, sigma, v, log_pi, want_z=False):
    """n seeded rows (n,D) from the mixture sum_k pi_k S(. | mu_k, sigma_k, v_k) in one streaming HIP pass
    (vmp_mixture_impute_pack_t + vmp_mixture_sample); with want_z also the (n,) int32 components.  Row i is a function of
    (seed, i) only; conditional draws of partly observed rows are models._mix.mixture_sample on the same pack."""
    from ..models import _mix
    pack = _mix.impute_pack_t(log_pi, mu, sigma, v)
    y, z = _mix.mixture_draw(n, pack, seed, want_z=want_z)
    return (y, z) if want_z else y
