"""fp64 truth of mixture sampling (include/vmp_hip.h "Mixture sampling"; csrc/vmp_sample.hip) for tests/test_mix_sample_*.py, CPU only.

From (x, miss, parameters, seed, row0, draws) draw() regenerates the uniforms and normals of the documented counter layout with
oracle/philox.py - counter = (row low, row high, s, SAMPLE_TAG + b), key = seed; b = 0: u_z, u_b; b = 1: eps; b = 16 + t: attempt t of
the gamma draw - and evaluates the draw: the responsibilities are those of tests/mix_impute_truth.py (evaluate), the chosen
component's cell is restated here index by index in the kernel's order.  dtype = float64 is the truth; dtype = float32 rounds every
operand once and keeps every intermediate in fp32 - the restatement (up to the fused multiply-adds and the order of the in-row prefix
sum, which numpy cannot express).  Besides the draw it reports the DECISION MARGINS of every (draw, row): the distance of u_z from
the nearest boundary of the cdf, and for every gamma attempt that was looked at the distance of the accept inequality from equality
in log units.  measure() compares the two runs: the largest margin at which the restatement takes another decision than the truth
sets tau, its worst error on the rows that tau leaves decidable sets the bar (profiles/NOTES_mix_stream_shared.md section 6)."""
import numpy as np
import torch

import mix_impute_truth as T
from mix_score_truth import make_case  # noqa: F401  (re-exported for the tests)
from oracle import philox

SAMPLE_TAG = 0x6d78a500
B_Z, B_EPS, B_GAMMA = 0, 1, 16
ATTEMPTS = 8
FLT_MIN = 1.17549435e-38

# tau and the bar of tests/test_mix_sample_gpu.py, from measure() over the sweep below (profiles/NOTES_mix_sample.md): the restatement
# flips a decision at margins up to 2.2e-7 and is off by up to 4.6204e-6 on the decidable rows (N = 532 481, pack_niw); 4 x each, floored at 1e-5
TAU = 1e-5
BAR = 4 * 4.6204e-6

# the shape sweep of tests/test_mix_sample_gpu.py: (N, D, K); LONG_N makes a wave of the capped grid (2048 blocks of 4 waves) walk
# 64 rows - one row per lane - plus a ragged group of 4, and leaves the last waves without rows (rows per wave 68, 7831 of 8192 used)
SWEEP = [(1, 1, 17), (63, 5, 33), (64, 8, 1), (65, 3, 17), (257, 8, 3), (4099, 8, 16), (4099, 3, 64), (65, 8, 64)]
LONG_N = (532481, 2, 3)
# draw seeds are chosen so that the TRUTH leaves at most 1 % of a case's rows undecidable (in a case of fewer than 100 rows: none)
SEED_SALT = {(65, 3, 17): 1}


def _words(seed, rows, draws, block):
    """(draws, N, 4) uint32: Philox block `block` of every (draw, absolute row)"""
    rows = np.asarray(rows, dtype=np.uint64)
    ctr = np.zeros((draws, rows.size, 4), dtype=np.uint32)
    ctr[..., 0] = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32)[None, :]
    ctr[..., 1] = (rows >> np.uint64(32)).astype(np.uint32)[None, :]
    ctr[..., 2] = np.arange(draws, dtype=np.uint32)[:, None]
    ctr[..., 3] = np.uint32(SAMPLE_TAG + block)
    key = np.zeros((draws, rows.size, 2), dtype=np.uint32)
    key[..., 0] = np.uint32(seed & 0xFFFFFFFF)
    key[..., 1] = np.uint32((seed >> 32) & 0xFFFFFFFF)
    return philox.philox4x32(ctr, key)


def uniform(w, dtype):
    """(top 24 bits + 1/2) 2^-24, rounded once to dtype and kept at most 1 - 2^-24 (fp32 would round the largest to 1.0)"""
    return np.minimum((((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(dtype), dtype(1 - 2.0 ** -24))


def _normal_pair(w, dtype):
    """oracle.philox.box_muller8 with every intermediate in dtype (it is box_muller8 itself for float64)"""
    a = (((w >> np.uint32(12)).astype(np.float64) + 0.5) * 2.0 ** -20).astype(dtype)
    th = ((w & np.uint32(0xFFF)).astype(np.float64) * 2.0 ** -12).astype(dtype) * dtype(2 * np.pi)
    r = np.sqrt(dtype(-2.0) * np.log(a))
    return r * np.cos(th), r * np.sin(th)


def normals(seed, rows, draws, D, dtype=np.float64):
    """eps (draws, N, D) of block 1: word t -> (eps_2t, eps_2t+1)"""
    c, s = _normal_pair(_words(seed, rows, draws, B_EPS), dtype)
    return np.stack([c, s], axis=-1).reshape(draws, len(rows), 8)[..., :D]


def _cell(x, miss, mu, P, dtype):
    """the chosen component's cell, vectorised over the leading axes: x, miss, mu (..., D), P (..., D, D) -> q, xh (list of D), A, rd
    in the order of sample_cell (csrc/vmp_sample.hip)"""
    D = x.shape[-1]
    zero, one = dtype(0), dtype(1)
    mk = [miss[..., d] for d in range(D)]
    dt = [np.where(mk[d], zero, x[..., d] - mu[..., d]) for d in range(D)]
    lam = lambda i, j: P[..., max(i, j), min(i, j)]
    v, qo = [], np.zeros(x.shape[:-1], dtype)
    for i in range(D):
        s = lam(i, 0) * dt[0]
        for j in range(1, D):
            s = s + lam(i, j) * dt[j]
        v.append(np.where(mk[i], s, zero))
        qo = qo + dt[i] * s
    A = [[np.where(mk[i] & mk[j], lam(i, j), one if i == j else zero) for j in range(i + 1)] for i in range(D)]
    rd = []
    for j in range(D):
        s = A[j][j]
        for q in range(j):
            s = s - A[j][q] * A[j][q]
        rd.append(one / np.sqrt(s))
        for i in range(j + 1, D):
            t = A[i][j]
            for q in range(j):
                t = t - A[i][q] * A[j][q]
            A[i][j] = t * rd[j]
    yy = np.zeros(x.shape[:-1], dtype)
    for i in range(D):
        s = v[i]
        for q in range(i):
            s = s - A[i][q] * v[q]
        v[i] = s * rd[i]
        yy = yy + v[i] * v[i]
    for i in range(D - 1, -1, -1):
        s = v[i]
        for q in range(i + 1, D):
            s = s - A[q][i] * v[q]
        v[i] = s * rd[i]
    xh = [mu[..., d] - v[d] for d in range(D)]
    q = qo - yy
    return np.where(q < 0, zero, q), xh, A, rd


def draw(x, miss, pk, seed, row0=0, draws=1, dtype=np.float64, N=None):
    """The draws of rows row0 .. row0 + N - 1 under the fp64 pack pk (mix_impute_truth.pack_t / pack_niw), every operation in dtype.
    x = miss = None (then N is given): every entry missing.  Returns a dict: x (draws,N,D), z (draws,N) int64, resp (N,K),
    margin_z, margin_g (draws,N) - the smallest decision margins of the draw -, attempts (draws,N) - gamma attempts looked at -,
    exhausted (draws,N) bool."""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    D, K = pk[0].shape[1], pk[0].shape[0]
    if x is None:
        x, miss = np.zeros((N, D), np.float32), np.ones((N, D), np.uint8)
    x, miss = np.asarray(x), np.asarray(miss) != 0
    N = x.shape[0]
    xs = np.where(miss, 0, x)                                      # what a missing slot holds never enters
    _, _, resp, _ = T.evaluate(xs, miss, pk, tdt)
    resp = resp.numpy()
    mu, P, _, nu = (t.to(tdt).numpy() for t in pk[:4])
    n_obs = (~miss).sum(1)
    rows = np.arange(N, dtype=np.uint64) + np.uint64(row0)

    # component
    wz = _words(seed, rows, draws, B_Z)
    u_z, u_b = uniform(wz[..., 0], dtype), uniform(wz[..., 1], dtype)
    cdf = np.cumsum(resp, axis=1, dtype=dtype)
    with np.errstate(invalid='ignore'):
        hit = cdf[None, :, :] > u_z[..., None]                     # (draws, N, K)
        pos = resp > 0
    first = hit.argmax(-1)
    last = np.where(pos.any(1), K - 1 - pos[:, ::-1].argmax(1), -1)
    z = np.where(hit.any(-1), first, last[None, :])
    margin_z = np.abs(cdf[None, :, :].astype(np.float64) - u_z[..., None].astype(np.float64)).min(-1)
    bad = np.isnan(resp).any(1)
    zc = np.maximum(z, 0)

    # the chosen component's cell
    xb = np.broadcast_to(xs.astype(dtype), (draws, N, D))
    mb = np.broadcast_to(miss, (draws, N, D))
    q, xh, A, rd = _cell(xb, mb, mu[zc], P[zc], dtype)
    nuz = nu[zc]

    # scale
    a = dtype(0.5) * (nuz + n_obs[None, :].astype(dtype))
    small = a < 1
    ap = np.where(small, a + dtype(1), a)
    d = ap - dtype(np.float32(0.333333343))
    c = dtype(1) / np.sqrt(dtype(9) * d)
    gam, done = d.copy(), np.zeros(a.shape, bool)
    margin_g = np.full(a.shape, np.inf)
    attempts = np.zeros(a.shape, np.int64)
    for t in range(ATTEMPTS):
        wg = _words(seed, rows, draws, B_GAMMA + t)
        n_t, _ = _normal_pair(wg[..., 0], dtype)
        lu = np.log(uniform(wg[..., 1], dtype))
        w = dtype(1) + c * n_t
        v = w * w * w
        with np.errstate(invalid='ignore', divide='ignore'):
            rhs = dtype(0.5) * n_t * n_t + d - d * v + d * np.log(np.where(w > 0, v, dtype(1)))
            ok = (w > 0) & (lu < rhs)
            m = np.where(w > 0, np.abs(lu.astype(np.float64) - rhs.astype(np.float64)), np.inf)
        margin_g = np.where(done, margin_g, np.minimum(margin_g, m))
        attempts += ~done
        gam = np.where(~done & ok, d * v, gam)
        done |= ok
    g = dtype(2) * gam
    with np.errstate(divide='ignore', invalid='ignore'):
        g = np.where(small, g * np.exp(np.log(u_b) / np.where(small, a, dtype(1))), g)
        g = np.where(g < dtype(FLT_MIN), dtype(FLT_MIN), g)
        scale = np.sqrt((nuz + q) / g)

    # entries
    eps = normals(seed, rows, draws, D, dtype)
    w = [np.where(mb[..., i], eps[..., i], dtype(0)) for i in range(D)]
    for i in range(D - 1, -1, -1):
        s = w[i]
        for j in range(i + 1, D):
            s = s - A[j][i] * w[j]
        w[i] = s * rd[i]
    with np.errstate(invalid='ignore'):
        xm = np.stack([xh[i] + scale * w[i] for i in range(D)], axis=-1)
    none = (z < 0)[..., None]
    xm = np.where(none, np.where(bad[None, :, None], dtype(np.nan), dtype(0)), xm)
    out = np.where(mb, xm, np.broadcast_to(x.astype(dtype), (draws, N, D)))
    return dict(x=out, z=z.astype(np.int64), resp=resp, margin_z=margin_z, margin_g=margin_g, attempts=attempts, exhausted=~done & (z >= 0))


def make_mask(N, D, seed, p=0.25):
    """(N,D) uint8, 1 = missing: seeded Bernoulli(p) per entry; where N allows, row 0 all missing and row 1 all observed"""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = (rng.random((N, D)) < p).astype(np.uint8)
    m[0] = 1
    if N > 1:
        m[1] = 0
    return m


def case_inputs(N, D, K):
    """(x, miss, t, q, seed) of a sweep case: data and both parameter sets of mix_score_truth.make_case, the mask, the draw seed"""
    cs = 1000 * D + 10 * K + N % 7
    x, t, q = make_case(N, D, K, seed=cs)
    return x, make_mask(N, D, cs + 1), t, q, 0x9E3779B97F4A7C15 ^ (cs + (SEED_SALT.get((N, D, K), 0) << 20))


def undecidable(tr, tau):
    """(N,) bool: rows with a decision margin of any draw below tau"""
    return (np.minimum(tr['margin_z'], tr['margin_g']) < tau).any(0)


def rel_err(got, want, keep):
    """max |got - want| / (1 + |want|) over the kept rows ((draws,N,D) arrays, keep (N,))"""
    got, want = np.asarray(got, np.float64)[:, keep], np.asarray(want, np.float64)[:, keep]
    if got.size == 0:
        return 0.0
    return float(np.nanmax(np.abs(got - want) / (1.0 + np.abs(want))))


def measure(x, miss, pk, seed, draws, row0=0, N=None):
    """(truth, flip, err): the fp64 run, the largest margin of a (draw, row) at which the fp32 restatement decides otherwise than the
    truth (another z or another number of gamma attempts; 0.0 if none), and err(tau) -> the restatement's worst relative error on the
    rows tau leaves decidable"""
    t64 = draw(x, miss, pk, seed, row0, draws, np.float64, N)
    t32 = draw(x, miss, pk, seed, row0, draws, np.float32, N)
    fz = t64['z'] != t32['z']
    fg = ~fz & (t64['attempts'] != t32['attempts'])                # behind another z the gamma draw is another draw altogether
    flip = max([0.0] + [float(t64[k][f].max()) for k, f in (('margin_z', fz), ('margin_g', fg)) if f.any()])
    return t64, flip, lambda tau: rel_err(t32['x'], t64['x'], ~undecidable(t64, tau))
