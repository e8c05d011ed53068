"""fp64 truth of the diagonal-covariance Gaussian mixture fit (include/vmp_hip.h "Diagonal-covariance mixture fitting on wide rows") for
tests/test_mix_diag_*.py, in torch (torch.special.digamma, torch.lgamma).

  make_data()     centres N(0, 3^2), per-coordinate sd uniform in [0.5, 1.5], a Dirichlet r0, x rounded to fp32
  planted_clusters()  unit-variance clusters far apart, for responsibilities that underflow to exact zeros
  default_prior() alpha_0 = 0.05 / K, beta_0 = 0.5, m_0 = column means (rounded to fp32, as the product hands them to the kernels),
                  a_0 = 1, b_0 = 1
  moments()       two-pass centred moments, as oracle/mixtures.py forms them: Nk, xbar, NS = sum_n r_nk (x_n - xbar_k)^2
  m_step(), e_step(), kl_terms(), iterate()
  log_marginal()  closed-form log marginal likelihood of D independent Normal-Gamma models (K = 1)
  bars()          truth, the error of the same functions run in fp32, and bar = max(1e-5, 3 x that error) per quantity
  aux()           the finalize's other outputs: xbar, S = NS / Nk (0 where Nk = 0), pi = exp(psi(alpha_k) - psi(sum alpha))
  geometry()      the launch geometry of the pass for (N, D, K): blocks, waves, rows per wave, waves without rows
  pass_truth()    one E-step and its raw moments over the rows in chunks (never an (N, K, D) array), with the fp32 restatement
  int_case(), int_stats(), int_model()   integer x and a one-hot r whose moments the kernel must give exactly; the numpy fp32 model
                  of the kernel's arithmetic that says why
  mp_finalize(), mp_pack(), mp_terms()   the K-sized kernels in mpmath at 50 digits

dtype = torch.float32 runs every function in fp32 from the fp32 inputs; only the sum of the rows' log-sum-exp is taken in fp64, as
the kernel takes it."""
import math

import numpy as np
import torch

LOG_2PI = math.log(2.0 * math.pi)
NAMES = ('alpha', 'beta', 'm', 'a', 'b')
SHAPES = [(300, 1, 2), (257, 17, 3), (513, 64, 16), (65, 5, 64), (1031, 33, 33)]     # the last one also with offset +1000


def make_data(N, D, K, seed, offset=0.0, r_rows=None):
    """r_rows: r0 for the first r_rows rows only (a start for a large x)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((K, D)) * 3.0
    sd = rng.uniform(0.5, 1.5, (K, D))
    z = rng.integers(0, K, N)
    x = (c[z] + sd[z] * rng.standard_normal((N, D)) + offset).astype(np.float32)
    r0 = rng.dirichlet(np.ones(K), N if r_rows is None else r_rows).astype(np.float32)
    return x, r0


def planted_clusters(N, D, K, sep, seed):
    """K unit-variance clusters with centres pairwise `sep` standard deviations apart (centre k on axis k): (x fp32, centres fp64, labels)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = np.zeros((K, D))
    centres[np.arange(K), np.arange(K)] = sep / math.sqrt(2.0)
    z = rng.integers(0, K, N)
    return (centres[z] + rng.standard_normal((N, D))).astype(np.float32), centres, z


def default_prior(x, K):
    x = np.asarray(x)
    D = x.shape[1]
    mean = x.astype(np.float64).mean(0).astype(np.float32)
    return (np.full(K, 0.05 / K, np.float32), np.full(K, 0.5, np.float32), np.tile(mean[None, :], (K, 1)),
            np.ones(K, np.float32), np.ones((K, D), np.float32))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def moments(x, r, dtype):
    x, r = _t(x, dtype), _t(r, dtype)
    Nk = r.sum(0)
    some = Nk > 0
    xbar = torch.where(some[:, None], (r.t() @ x) / Nk.clamp_min(1e-300 if dtype == torch.float64 else 1e-30)[:, None], torch.zeros((), dtype=dtype))
    dev = x[:, None, :] - xbar[None, :, :]
    NS = (r[:, :, None] * dev * dev).sum(0)
    return Nk, xbar, NS


def raw_stats(Nk, xbar, NS):
    """(K, 1 + 2 D) fp64 [Nk | sx | sxx] from the centred moments"""
    Nk, xbar, NS = Nk.double(), xbar.double(), NS.double()
    return torch.cat([Nk[:, None], Nk[:, None] * xbar, NS + Nk[:, None] * xbar * xbar], 1)


def m_step(Nk, xbar, NS, prior, dtype):
    a0, b0, m0, g0, h0 = [_t(p, dtype) for p in prior]            # alpha_0, beta_0, m_0, a_0, b_0
    alpha, beta, a = a0 + Nk, b0 + Nk, g0 + Nk / 2
    m = (b0[:, None] * m0 + Nk[:, None] * xbar) / beta[:, None]
    b = h0 + 0.5 * (NS + (b0 * Nk / beta)[:, None] * (xbar - m0) ** 2)
    return alpha, beta, m, a, b


def aux(Nk, xbar, NS, alpha):
    """(xbar, S, pi) as the finalize hands them out, in the dtype of its arguments"""
    some = Nk > 0
    S = torch.where(some[:, None], NS / torch.where(some, Nk, torch.ones_like(Nk))[:, None], torch.zeros_like(NS))
    dg = torch.special.digamma
    return xbar, S, torch.exp(dg(alpha) - dg(alpha.sum()))


def e_step(x, theta, dtype):
    alpha, beta, m, a, b = [t.to(dtype) for t in theta]
    x = _t(x, dtype)
    D = x.shape[1]
    dg = torch.special.digamma
    c = dg(alpha) - dg(alpha.sum()) + 0.5 * (dg(a)[:, None] - torch.log(b)).sum(1) - D / (2 * beta)
    lbar = a[:, None] / b
    dev = x[:, None, :] - m[None, :, :]
    logrho = c[None, :] - 0.5 * (lbar[None, :, :] * dev * dev).sum(2)
    lse = torch.logsumexp(logrho, 1)
    logr = logrho - lse[:, None]
    data = lse.double().sum().item() - 0.5 * x.shape[0] * D * LOG_2PI
    return torch.exp(logr), logr, data


def kl_terms(theta, prior):
    """(kl_pi, kl_ng (K,D)) in fp64"""
    alpha, beta, m, a, b = [torch.as_tensor(t).double() for t in theta]
    a0, b0, m0, g0, h0 = [_t(p, torch.float64) for p in prior]
    dg, lg = torch.special.digamma, torch.lgamma
    kl_pi = (lg(alpha.sum()) - lg(alpha).sum() - lg(a0.sum()) + lg(a0).sum() + ((alpha - a0) * (dg(alpha) - dg(alpha.sum()))).sum()).item()
    lbar = a[:, None] / b
    kl_ng = ((0.5 * torch.log(beta / b0) - 0.5 + 0.5 * b0 / beta)[:, None] + 0.5 * b0[:, None] * lbar * (m - m0) ** 2
             + ((a - g0) * dg(a) - lg(a) + lg(g0))[:, None] + g0[:, None] * (torch.log(b) - torch.log(h0)) + a[:, None] * (h0 - b) / b)
    return kl_pi, kl_ng


def iterate(x, r0, prior, iterations, dtype=torch.float64):
    """the state after `iterations` iterations from r0: dict(r, logr, stats, theta, xbar, S, pi, data, bound, bounds, kl_pi, kl_ng,
    kl_k = kl_ng.sum(1), kl_sum = kl_ng.sum())"""
    r = _t(r0, dtype)
    bounds, out = [], None
    for _ in range(iterations):
        mom = moments(x, r, dtype)
        theta = m_step(*mom, prior, dtype)
        xbar, S, pi = aux(*mom, theta[0])
        r, logr, data = e_step(x, theta, dtype)
        kl_pi, kl_ng = kl_terms(theta, prior)
        bounds.append(data - kl_pi - kl_ng.sum().item())
        out = dict(r=r, logr=logr, theta=theta, xbar=xbar, S=S, pi=pi, data=data, bound=bounds[-1], kl_pi=kl_pi, kl_ng=kl_ng,
                   kl_k=kl_ng.sum(1), kl_sum=kl_ng.sum().item())
    out['stats'] = raw_stats(*moments(x, r, dtype))
    out['bounds'] = bounds
    return out


def log_marginal(x, prior):
    """log p(x) of D independent Normal-Gamma models with the prior's component 0 (the K = 1 mixture), fp64"""
    _, b0, m0, g0, h0 = [_t(p, torch.float64) for p in prior]
    x = _t(x, torch.float64)
    N = x.shape[0]
    xbar = x.mean(0)
    NS = ((x - xbar) ** 2).sum(0)
    bN, aN = b0[0] + N, g0[0] + N / 2
    hN = h0[0] + 0.5 * (NS + b0[0] * N / bN * (xbar - m0[0]) ** 2)
    lg = torch.lgamma
    return (-0.5 * N * LOG_2PI + 0.5 * torch.log(b0[0] / bN) + g0[0] * torch.log(h0[0]) - aN * torch.log(hN) + lg(aN) - lg(g0[0])).sum().item()


def _f64(a):
    """fp64 on the host; a Python float keeps its 53 bits (torch.as_tensor alone would round it to fp32)"""
    return a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def abs_err(a, b):
    return (_f64(a) - _f64(b)).abs().max().item()


def rel_err(a, b):
    a, b = _f64(a), _f64(b)
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()


def errors(got, truth):
    """errors of a state dict against the truth: absolute for r, relative to max(1, |value|) for everything else"""
    errs = {}
    if got.get('r') is not None:
        errs['r'] = abs_err(got['r'], truth['r'])
    for name in ('logr', 'stats', 'xbar', 'S', 'pi', 'kl_k'):
        if got.get(name) is not None:
            errs[name] = rel_err(got[name], truth[name])
    if got.get('theta') is not None:
        for name, a, b in zip(NAMES, got['theta'], truth['theta']):
            errs[name] = rel_err(a, b)
    for name in ('data', 'bound', 'kl_pi', 'kl_sum'):
        if got.get(name) is not None:
            errs[name] = rel_err(float(got[name]), float(truth[name]))
    return errs


def bars(x, r0, prior, iterations):
    """the fp64 truth after `iterations` iterations, the errors e_* of the same functions run in fp32 from the same inputs, and
    bar_* = max(1e-5, 3 x e_*)"""
    t64 = iterate(x, r0, prior, iterations, torch.float64)
    t32 = iterate(x, r0, prior, iterations, torch.float32)
    out = dict(t64)
    for k, e in errors(t32, t64).items():
        out['e_' + k] = e
        out['bar_' + k] = max(1e-5, 3 * e)
    return out


# ---- the launch geometry of the pass (csrc/vmp_diagfit.hip: diag_blocks, rows_per_wave) ----

def geometry(N, D, K):
    """dict(cap, blocks, waves, rpw, empty): blocks = min(cap, ceil(N / 2048)) with cap = 512 while K (1 + 2 D) <= 2048 and 256 beyond,
    4 waves per block, rows per wave = ceil(N / waves) rounded up to a multiple of 64, and the number of waves left without rows"""
    cap = 512 if K * (1 + 2 * D) <= 2048 else 256
    blocks = min(cap, max(1, -(-N // 2048)))
    waves = 4 * blocks
    rpw = -(-(-(-N // waves)) // 64) * 64
    return dict(cap=cap, blocks=blocks, waves=waves, rpw=rpw, empty=waves - (-(-N // rpw)))


def workspace_blocks(nbytes, D, K):
    """the block count behind vmp_mixture_diag_workspace_bytes: blocks x (4 waves x K (1 + 2 D) + 1) fp64 words and a 64-word fp32 pivot"""
    blocks, rest = divmod(nbytes - 256, 8 * (4 * K * (1 + 2 * D) + 1))
    assert rest == 0 and blocks >= 1, (nbytes, D, K)
    return blocks


# ---- one pass over many rows, in chunks ----

def _chunked_moments(x, r_chunks, dtype, chunk):
    """moments() over the chunks of x: Nk and r^T x first, then NS about xbar; every sum and every accumulation in `dtype`"""
    K, D = r_chunks[0].shape[1], x.shape[1]
    Nk, sx = torch.zeros(K, dtype=dtype), torch.zeros(K, D, dtype=dtype)
    for i, r in enumerate(r_chunks):
        xc = _t(x[i * chunk:(i + 1) * chunk], dtype)
        Nk += r.sum(0)
        sx += r.t() @ xc
    some = Nk > 0
    xbar = torch.where(some[:, None], sx / Nk.clamp_min(1e-300 if dtype == torch.float64 else 1e-30)[:, None], torch.zeros((), dtype=dtype))
    NS = torch.zeros(K, D, dtype=dtype)
    for i, r in enumerate(r_chunks):
        dev = _t(x[i * chunk:(i + 1) * chunk], dtype)[:, None, :] - xbar[None, :, :]
        dev.mul_(dev).mul_(r[:, :, None])
        NS += dev.sum(0)
    return Nk, xbar, NS


def pass_truth(x, theta, got_r=None, got_logr=None, chunk=65536):
    """One E-step under theta and the raw moments of its r, over the rows of x in chunks of `chunk` - never an (N, K, D) array.
    dict(stats, data) in fp64; e_r, e_logr, e_stats, e_data = the errors of the same functions run in fp32 (the log-sum-exp sum in
    fp64) and bar_* = max(1e-5, 3 x e_*); with got_r / got_logr (N,K) their errors err_r / err_logr, compared chunk by chunk."""
    x = np.asarray(x)
    N, D = x.shape
    f64, f32 = torch.float64, torch.float32
    th = {f64: [torch.as_tensor(np.asarray(t)).to(f64) for t in theta], f32: [torch.as_tensor(np.asarray(t)).to(f32) for t in theta]}
    rs, data = {f64: [], f32: []}, {f64: 0.0, f32: 0.0}
    out = dict(e_r=0.0, e_logr=0.0)
    if got_r is not None:
        out['err_r'] = 0.0
    if got_logr is not None:
        out['err_logr'] = 0.0
    for c0 in range(0, N, chunk):
        xc = x[c0:c0 + chunk]
        r64, l64, d64 = e_step(xc, th[f64], f64)
        r32, l32, d32 = e_step(xc, th[f32], f32)
        data[f64] += d64
        data[f32] += d32
        out['e_r'] = max(out['e_r'], abs_err(r32, r64))
        out['e_logr'] = max(out['e_logr'], rel_err(l32, l64))
        if got_r is not None:
            out['err_r'] = max(out['err_r'], abs_err(got_r[c0:c0 + chunk], r64))
        if got_logr is not None:
            out['err_logr'] = max(out['err_logr'], rel_err(got_logr[c0:c0 + chunk], l64))
        rs[f64].append(r64)
        rs[f32].append(r32)
    out['stats'] = raw_stats(*_chunked_moments(x, rs[f64], f64, chunk))
    out['stats32'] = raw_stats(*_chunked_moments(x, rs[f32], f32, chunk))
    out['data'], out['data32'] = data[f64], data[f32]
    out['e_stats'] = rel_err(out['stats32'], out['stats'])
    out['e_data'] = rel_err(data[f32], data[f64])
    for name in ('r', 'logr', 'stats', 'data'):
        out['bar_' + name] = max(1e-5, 3 * out['e_' + name])
    return out


# ---- integer data whose moments are exact in the kernel's arithmetic ----

def int_case(N, D, K):
    """x (N,D) int64 with values in {0, 1, 2, 3} and a component z (N) int64 per row, both fixed functions of the row index"""
    n = np.arange(N, dtype=np.int64)
    xi = (n[:, None] * (np.arange(D, dtype=np.int64) + 1)[None, :] + (n // 5)[:, None]) % 4
    z = (7 * n + n // 3) % K
    return xi, z


def one_hot(z, K):
    r = np.zeros((len(z), K), np.float32)
    r[np.arange(len(z)), z] = 1.0
    return r


def int_stats(xi, z, K):
    """(K, 1 + 2 D) int64 [Nk | sx | sxx] of the one-hot r of z: counts of (component, value) pairs, int64 throughout"""
    N, D = xi.shape
    out = np.zeros((K, 1 + 2 * D), np.int64)
    out[:, 0] = np.bincount(z, minlength=K)
    v = np.arange(4, dtype=np.int64)
    for d in range(D):
        cnt = np.bincount(4 * z + xi[:, d], minlength=4 * K).reshape(K, 4).astype(np.int64)
        out[:, 1 + d] = (cnt * v).sum(1)
        out[:, 1 + D + d] = (cnt * v * v).sum(1)
    return out


def pivot_model(x):
    """the kernel's pivot in numpy fp32: the column means of min(N, 64) rows with stride N // that count, added in row order"""
    x = np.asarray(x, np.float32)
    N = x.shape[0]
    cnt = min(N, 64)
    s = np.zeros(x.shape[1], np.float32)
    for j in range(cnt):
        s = s + x[j * (N // cnt)]
    return s / np.float32(cnt)


def int_model(xi, z, K):
    """The kernel's arithmetic on int_case() data in numpy: fp32 pivot, fp32 x - pivot and its square, fp32 sums over the 128 rows
    between two flushes (added row by row), fp64 from there on, the un-shift in the kernel's own order.  Asserts on the way what makes
    the result exact: the pivot is a multiple of 1/64, the differences and squares are exact and multiples of 2^-6 and 2^-12, and a
    128-row sum stays below 2^11, so that every partial sum in ANY order of addition fits the 24 bits of an fp32.  Returns the
    (K, 1 + 2 D) fp64 stats."""
    N, D = xi.shape
    assert N >= 64                                                  # below, the pivot divides by N and is no multiple of 1/64
    x = xi.astype(np.float32)
    p = pivot_model(x)
    assert (p.astype(np.float64) * 64 == np.round(p.astype(np.float64) * 64)).all()
    y = x - p[None, :]
    assert y.dtype == np.float32 and (y.astype(np.float64) == xi.astype(np.float64) - p.astype(np.float64)[None, :]).all()
    y2 = y * y
    assert y2.dtype == np.float32 and (y2.astype(np.float64) == y.astype(np.float64) ** 2).all()
    assert (y.astype(np.float64) * 2 ** 6 % 1 == 0).all() and (y2.astype(np.float64) * 2 ** 12 % 1 == 0).all()
    assert 128 * np.abs(y).max() < 2 ** 11 and 128 * y2.max() < 2 ** 11          # < 2^11 with 12 fractional bits: 23 bits
    G = -(-N // 128)
    r = np.zeros((G * 128, K), np.float32)
    r[:N] = one_hot(z, K)
    s = []
    for v in (np.ones((G * 128, 1), np.float32), np.concatenate([y, np.zeros((G * 128 - N, D), np.float32)]),
              np.concatenate([y2, np.zeros((G * 128 - N, D), np.float32)])):
        t = (r[:, :, None] * v[:, None, :]).reshape(G, 128, K, v.shape[1])
        c32 = np.cumsum(t, axis=1, dtype=np.float32)
        assert (c32.astype(np.float64) == np.cumsum(t, axis=1, dtype=np.float64)).all()       # every partial sum, not the last alone
        s.append(c32[:, -1].astype(np.float64).sum(0))
    t0, t1, t2 = s[0], s[1], s[2]                                   # (K,1), (K,D), (K,D)
    pd = p.astype(np.float64)[None, :]
    return np.concatenate([t0, t1 + t0 * pd, t2 + 2.0 * pd * t1 + t0 * pd * pd], 1)


# ---- the K-sized kernels (finalize, pack, bound terms) in mpmath at 50 digits ----

MP_DIGITS = 50


def _mp(a):
    """object array of mpf from a float array: every fp32 / fp64 value is taken exactly"""
    import mpmath
    a = np.asarray(a)
    return np.array([mpmath.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def _mpf(fn):
    return np.frompyfunc(fn, 1, 1)


def mp_finalize(stats, prior):
    """dict(alpha, beta, m, a, b, xbar, S, pi) of mpf arrays from fp64 stats (K, 1 + 2 D) and the fp32 prior"""
    import mpmath
    with mpmath.workdps(MP_DIGITS):
        stats = _mp(np.asarray(stats, np.float64))
        K, D = stats.shape[0], (stats.shape[1] - 1) // 2
        a0, b0, m0, g0, h0 = [_mp(np.asarray(p, np.float32)) for p in prior]
        zero, one = mpmath.mpf(0), mpmath.mpf(1)
        Nk, sx, sxx = stats[:, 0], stats[:, 1:1 + D], stats[:, 1 + D:]
        some = np.array([v > 0 for v in Nk])
        safe = np.where(some, Nk, one)
        xbar = np.where(some[:, None], sx / safe[:, None], zero)
        NS = np.where(some[:, None], sxx - sx * sx / safe[:, None], zero)
        NS = np.where(NS < 0, zero, NS)
        alpha, beta, a = a0 + Nk, b0 + Nk, g0 + Nk / 2
        m = (b0[:, None] * m0 + sx) / beta[:, None]
        b = h0 + (NS + (b0 * Nk / beta)[:, None] * (xbar - m0) ** 2) / 2
        pi = _mpf(mpmath.exp)(_mpf(mpmath.digamma)(alpha) - mpmath.digamma(alpha.sum()))
        return dict(alpha=alpha, beta=beta, m=m, a=a, b=b, xbar=xbar, S=np.where(some[:, None], NS / safe[:, None], zero), pi=pi)


def mp_pack(theta):
    """(K, 2 D + 1) mpf pack [ m | a / b | c ] of an fp32 posterior"""
    import mpmath
    with mpmath.workdps(MP_DIGITS):
        alpha, beta, m, a, b = [_mp(np.asarray(t, np.float32)) for t in theta]
        D = m.shape[1]
        dg = _mpf(mpmath.digamma)
        c = dg(alpha) - mpmath.digamma(alpha.sum()) + (D * dg(a) - _mpf(mpmath.log)(b).sum(1)) / 2 - D / (2 * beta)
        return np.concatenate([m, a[:, None] / b, c[:, None]], 1)


def mp_terms(theta, prior):
    """(kl_pi, kl_ng (K,D)) as kl_terms(), in mpf, from an fp32 posterior and prior"""
    import mpmath
    with mpmath.workdps(MP_DIGITS):
        alpha, beta, m, a, b = [_mp(np.asarray(t, np.float32)) for t in theta]
        a0, b0, m0, g0, h0 = [_mp(np.asarray(p, np.float32)) for p in prior]
        dg, lg, log = _mpf(mpmath.digamma), _mpf(mpmath.loggamma), _mpf(mpmath.log)
        asum, a0sum = alpha.sum(), a0.sum()
        kl_pi = (mpmath.loggamma(asum) - lg(alpha).sum() - mpmath.loggamma(a0sum) + lg(a0).sum()
                 + ((alpha - a0) * (dg(alpha) - mpmath.digamma(asum))).sum())
        kl_ng = ((log(beta / b0) / 2 - mpmath.mpf(1) / 2 + b0 / beta / 2)[:, None] + b0[:, None] * (a[:, None] / b) * (m - m0) ** 2 / 2
                 + ((a - g0) * dg(a) - lg(a) + lg(g0))[:, None] + g0[:, None] * (log(b) - log(h0)) + a[:, None] * (h0 - b) / b)
        return kl_pi, kl_ng


def mp_err(got, ref, floor):
    """max |got - ref| / max(|ref|, floor) over the elements, the difference taken in mpf: got holds floats, ref mpf"""
    import mpmath
    with mpmath.workdps(MP_DIGITS):
        got = _mp(torch.as_tensor(got).detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64))
        ref = np.asarray(ref, dtype=object).reshape(got.shape)
        worst = mpmath.mpf(0)
        for g, r in zip(got.ravel(), ref.ravel()):
            e = abs(g - r) / max(abs(r), mpmath.mpf(floor))
            worst = e if not (e <= worst) else worst
        return float(worst)
