"""fp64 truth of the diagonal mixture's scoring pass (include/vmp_hip.h "Diagonal-covariance mixture: scoring and filling wide rows")
for tests/test_mix_diagscore_*.py, in numpy; G_k = lgamma(a + 1/2) - lgamma(a) - 1/2 log pi comes from mpmath at 30 digits (the
difference of two fp64 lgamma loses 1e-7 at a = 5e7).

  pack()            [m | g | h | log w | a + 1/2 | c] in fp64, NaN rows by the kernel's rule
  score()           l_nk, logp, resp, the sum and x with its missing entries filled, masked or not; dtype=np.float32 is the fp32
                    restatement: the pack rounded once to fp32 (as the kernel's), the row arithmetic in fp32 with a true log1p
                    (np.log1p on float32), the sum of the rows' logp in fp64; plain_log=True replaces log1p(t) by log(1 + t)
  errors(), bars()  bar = max(1e-5, 3 x the error of the fp32 restatement against fp64 on the same inputs) per quantity: absolute for
                    resp, relative to max(1, |value|) for logp, the sum and the filled entries
  explicit_theta()  a = 1 + N_k / 2, b = 1 + N_k s^2 / 2, beta = 0.5 + N_k, alpha = 0.05 / K + N_k for given counts N_k, and rows
                    drawn near the components
  quad_log_st()     log of the Normal-Gamma integral by mpmath quadrature"""
import math

import mpmath
import numpy as np

HALF_LOG_PI = 0.5 * math.log(math.pi)
NAMES = ('alpha', 'beta', 'm', 'a', 'b')


def gamma_term(a):
    """G = lgamma(a + 1/2) - lgamma(a) - 1/2 log pi, elementwise, NaN where a is not positive and finite"""
    out = np.full(np.shape(a), np.nan)
    with mpmath.workdps(30):
        for i, v in np.ndenumerate(np.asarray(a, np.float64)):
            if v > 0 and np.isfinite(v):
                out[i] = float(mpmath.loggamma(mpmath.mpf(v) + 0.5) - mpmath.loggamma(mpmath.mpf(v)) - mpmath.log(mpmath.pi) / 2)
    return out


def pack(theta):
    """dict(m, g, h (K,D), logw, ah, c (K)) in fp64 from theta (any float dtype; read as fp64)"""
    alpha, beta, m, a, b = [np.asarray(t, np.float64) for t in theta]
    with np.errstate(all='ignore'):
        g = beta[:, None] / (2.0 * b * (1.0 + beta[:, None]))
        h = gamma_term(a)[:, None] + 0.5 * np.log(g)
        logw = np.log(alpha / alpha.sum())
    bad = ~((alpha > 0) & (beta > 0) & (a > 0) & (b > 0).all(1))
    out = dict(m=m.copy(), g=g, h=h, logw=logw, ah=a + 0.5, c=logw + h.sum(1))
    for v in out.values():
        v[bad] = np.nan
    return out


def pack_array(p):
    """the (K, 3 D + 3) layout of the C ABI"""
    return np.concatenate([p['m'], p['g'], p['h'], p['logw'][:, None], p['ah'][:, None], p['c'][:, None]], 1)


def score(x, theta, miss=None, dtype=np.float64, plain_log=False, chunk=256, pk=None):
    """dict(l (N,K), logp (N), resp (N,K), total, filled (N,D) or None) in `dtype`"""
    p = {k: v.astype(dtype) for k, v in (pack(theta) if pk is None else pk).items()}
    x = np.asarray(x, dtype)
    N, D = x.shape
    obs = None if miss is None else (np.asarray(miss) == 0)
    ls = []
    with np.errstate(all='ignore'):
        for i in range(0, N, chunk):
            xc = x[i:i + chunk]
            if obs is not None:
                xc = np.where(obs[i:i + chunk], xc, dtype(0))               # what a missing slot holds never enters arithmetic
            dev = xc[:, None, :] - p['m'][None]
            t = p['g'][None] * dev * dev
            lt = np.log(dtype(1) + t) if plain_log else np.log1p(t)
            # a complete row: c_k and the D log1p terms; a masked row: log w_k, the h_kd and the log1p terms of its observed coordinates
            if obs is None:
                l = p['c'][None] - p['ah'][None] * lt.sum(2, dtype=dtype)
            else:
                o = obs[i:i + chunk, None, :]
                l = (p['logw'][None] + np.where(o, p['h'][None], dtype(0)).sum(2, dtype=dtype)) \
                    - p['ah'][None] * np.where(o, lt, dtype(0)).sum(2, dtype=dtype)
                l = np.where(np.isnan(p['c'])[None], dtype(np.nan), l)       # a NaN row stays NaN for a row with nothing observed
            ls.append(l.astype(dtype))
        l = np.concatenate(ls)
        ml = l.max(1)
        shift = np.where(np.isfinite(ml), ml, dtype(0))
        e = np.exp(l - shift[:, None])
        s = e.sum(1, dtype=dtype)
        logp = (shift + np.log(s)).astype(dtype)
        resp = np.where(s[:, None] > 0, e / np.where(s > 0, s, dtype(1))[:, None], dtype(0)).astype(dtype)
        filled = None
        if obs is not None:
            filled = np.where(obs, x, (resp @ np.nan_to_num(p['m'])).astype(dtype)) if not np.isnan(p['c']).any() else None
    return dict(l=l, logp=logp, resp=resp, total=float(logp.astype(np.float64).sum()), filled=filled)


def abs_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def errors(got, truth, miss=None):
    """errors of dict(logp, resp, total, filled) (missing keys / None skipped) against the truth"""
    errs = {}
    if got.get('logp') is not None:
        errs['logp'] = rel_err(got['logp'], truth['logp'])
    if got.get('resp') is not None:
        errs['resp'] = abs_err(got['resp'], truth['resp'])
    if got.get('total') is not None:
        errs['total'] = rel_err(got['total'], truth['total'])
    if got.get('filled') is not None and truth.get('filled') is not None:
        sel = np.asarray(miss) != 0
        errs['filled'] = rel_err(np.asarray(got['filled'])[sel], truth['filled'][sel])
    return errs


def bars(x, theta, miss=None):
    """the fp64 truth with e_* = the error of the fp32 restatement on the same inputs and bar_* = max(1e-5, 3 e_*)"""
    pk = pack(theta)
    t64 = score(x, theta, miss, np.float64, pk=pk)
    t32 = score(x, theta, miss, np.float32, pk=pk)
    out = dict(t64)
    for k, e in errors(t32, t64, miss).items():
        out['e_' + k] = e
        out['bar_' + k] = max(1e-5, 3 * e)
    return out


def explicit_theta(counts, D, seed):
    """theta (fp32 arrays, as a device holds them) for per-component counts N_k, and the per-coordinate sd s (K,D) it was made from"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Nk = np.asarray(counts, np.float64)
    K = len(Nk)
    m = rng.standard_normal((K, D)) * 3.0
    s = rng.uniform(0.5, 1.5, (K, D))
    theta = (0.05 / K + Nk, 0.5 + Nk, m, 1.0 + Nk / 2, 1.0 + Nk[:, None] * s * s / 2)
    return tuple(np.asarray(t, np.float32) for t in theta), s


def rows_near(theta, s, M, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.asarray(theta[2], np.float64)
    z = rng.integers(0, m.shape[0], M)
    return (m[z] + s[z] * rng.standard_normal((M, m.shape[1]))).astype(np.float32)


def quad_log_st(x, m, a, b, beta, dps=30):
    """log int_0^inf Gamma(lam; a, rate b) N(x; m, (1 + beta) / (beta lam)) d lam by quadrature"""
    with mpmath.workdps(dps):
        x, m, a, b, beta = [mpmath.mpf(v) for v in (x, m, a, b, beta)]
        prec = beta / (1 + beta)

        def f(lam):
            return mpmath.exp(a * mpmath.log(b) - mpmath.loggamma(a) + (a - 1) * mpmath.log(lam) - b * lam
                              + mpmath.log(prec * lam / (2 * mpmath.pi)) / 2 - prec * lam * (x - m) ** 2 / 2)
        mode = max(a / b, mpmath.mpf(1e-3))
        return float(mpmath.log(mpmath.quad(f, [0, mode / 4, mode, 4 * mode, 64 * mode, mpmath.inf])))
