"""fp64 truth of the variational lower bound of the Gaussian-mixture fit (include/vmp_hip.h "Variational lower bound") for
tests/test_mix_bound_*.py, in its three parts.  The definition is tests/mix_missfit_truth.lower_bound, imported unchanged: parts()
restates its K-sized terms one by one so that each can be compared on its own, and tests/test_mix_bound_truth.py holds the sum of
the parts to that function.

  parts()     (data, kl_pi, kl_nw (K)) in fp64, and the per-row log-sum-exp (without the 2 pi term)
  data32()    the fp32 restatement of the data term: e_step(dtype=float32, with_const=True)['lse'], each row rounded to fp32, summed in fp64
  case()      everything a test compares against for one posterior, with its bars
  sequence()  the bound after each of `iterations` iterations from r_init, truth and fp32 restatement, with the bar of each

The bar, as everywhere in this project: max(1e-5, 3 x the error of the fp32 restatement against the fp64 truth), relative to
max(1, |value|) - for the data term, the whole bound and the per-row log-sum-exp.  The K-sized parts are fp64 in the kernel: they
are compared with the truth on the same fp32-rounded theta at the project's floor, 1e-5 relative to max(1, |value|)."""
import math

import numpy as np
import torch

import mix_missfit_truth as T

FLOOR = 1e-5

# the inputs of the loop tests, CPU and GPU: (N, D, K, frac) of make_data(seed=7); frac = 0: the complete-data case (plain loop)
LOOP_INPUTS = [(300, 3, 4, 0.25), (300, 8, 16, 0.25), (64, 1, 3, 0.3), (300, 5, 20, 0.0)]


def rel(got, want):
    """|got - want| / max(1, |want|) of two scalars"""
    return abs(float(got) - float(want)) / max(1.0, abs(float(want)))


def loop_input(N, D, K, frac):
    """(x, r_init, miss or None): make_data(seed=7); frac = 0 gives complete rows and no mask (row 0, which make_data blanks,
    becomes a row of zeros, as in tests/test_mix_missfit_truth.py)"""
    x, r0, miss = T.make_data(N, D, K, seed=7, frac=frac)
    if frac > 0:
        return x, r0, miss
    return np.nan_to_num(x), r0, None


def _mask(x, miss):
    return np.zeros(np.asarray(x).shape, np.uint8) if miss is None else miss


def parts(x, miss, theta, prior=None):
    """dict(data, kl_pi, kl_nw (K), lse (N)) in fp64: the terms of T.lower_bound, each on its own"""
    alpha, beta, m, C, v = T._f64(theta)
    K, D = m.shape
    a0, b0, m0, C0, v0 = T._f64(T.default_prior(K, D) if prior is None else prior)
    b0 = b0.reshape(K)
    miss = _mask(x, miss)
    e = T.e_step(x, miss, theta, torch.float64, with_const=True)
    n_obs = torch.as_tensor((np.asarray(miss) == 0).sum(1)).double()
    _, Lbar, _, elp, eld = T.expectations(theta)
    lg = torch.lgamma
    kl_pi = lg(alpha.sum()) - lg(alpha).sum() - lg(a0.sum()) + lg(a0).sum() + ((alpha - a0) * elp).sum()
    dm = m - m0
    ldC, ldC0 = torch.linalg.slogdet(C)[1], torch.linalg.slogdet(C0)[1]
    kl_nw = (0.5 * D * torch.log(beta / b0) - 0.5 * D + 0.5 * D * b0 / beta + 0.5 * b0 * torch.einsum('kd,kde,ke->k', dm, Lbar, dm)
             + T._log_B(-ldC, v, D) - T._log_B(-ldC0, v0, D) + 0.5 * (v - v0) * eld - 0.5 * v * D
             + 0.5 * torch.einsum('kde,ked->k', C0, Lbar))
    return dict(data=e['lse'].sum().item(), kl_pi=kl_pi.item(), kl_nw=kl_nw, lse=e['lse'] + 0.5 * n_obs * T.LOG_2PI)


def data32(x, miss, theta):
    """(data, lse (N) without the 2 pi term) of the fp32 restatement: every row's log-sum-exp computed in fp32 and rounded to fp32,
    the rows added in fp64"""
    miss = _mask(x, miss)
    lse = T.e_step(x, miss, theta, torch.float32, with_const=True)['lse'].float()
    n_obs = torch.as_tensor((np.asarray(miss) == 0).sum(1)).float()
    return lse.double().sum().item(), (lse + 0.5 * n_obs * np.float32(T.LOG_2PI)).double()


def bar_of(err):
    return max(FLOOR, 3.0 * err)


def case(x, miss, theta, prior=None):
    """the truth of one posterior and the bars of what the kernel computes in fp32: dict(data, kl_pi, kl_nw, lse, bound, e_data,
    bar_data, e_bound, bar_bound, e_lse, bar_lse)"""
    p = parts(x, miss, theta, prior)
    d32, lse32 = data32(x, miss, theta)
    p['bound'] = p['data'] - p['kl_pi'] - p['kl_nw'].sum().item()
    b32 = d32 - p['kl_pi'] - p['kl_nw'].sum().item()
    p['e_data'], p['e_bound'], p['e_lse'] = rel(d32, p['data']), rel(b32, p['bound']), T.rel_err(lse32, p['lse'])
    for k in ('data', 'bound', 'lse'):
        p['bar_' + k] = bar_of(p['e_' + k])
    return p


def theta_after(x, miss, r_init, iterations, prior=None, dtype=torch.float64):
    return T.iterate(x, _mask(x, miss), r_init, iterations, prior, dtype)['theta']


def sequence(x, miss, r_init, iterations, prior=None):
    """[dict(bound, e, bar)] after iterations 1 .. `iterations` from r_init.  bound: T.lower_bound at the theta of the fp64
    iteration.  The restatement runs the whole iteration in fp32 (T.iterate(dtype=float32): what a loop on the device does to
    theta) and takes its bound as the kernels do - the data term of data32(), the K-sized terms in fp64 - at the theta it arrived at."""
    m = _mask(x, miss)
    K, D = np.asarray(r_init).shape[1], np.asarray(x).shape[1]
    prior = T.default_prior(K, D) if prior is None else prior
    out = []
    st64, st32 = T.seed_stats(x, m, r_init, torch.float64), T.seed_stats(x, m, r_init, torch.float32)
    for _ in range(iterations):
        it64 = T.one_iteration(x, m, st64, prior, torch.float64)
        it32 = T.one_iteration(x, m, st32, prior, torch.float32)
        st64, st32 = it64['stats'], it32['stats']
        b64 = T.lower_bound(x, m, it64['theta'], prior)
        p32 = parts(x, m, it32['theta'], prior)
        b32 = data32(x, m, it32['theta'])[0] - p32['kl_pi'] - p32['kl_nw'].sum().item()
        e = rel(b32, b64)
        out.append(dict(bound=b64, e=e, bar=bar_of(e)))
    return out
