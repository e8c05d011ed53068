"""fp64 truth of mixture initialisation (include/vmp_hip.h "Mixture initialisation"; csrc/vmp_seed.hip) for tests/test_mix_seed_*.py,
CPU only: the section's definitions restated with numpy and oracle.philox.philox4x32 - nothing is shared with the kernel.

centers() runs the K rounds of the exponential race and reports, next to the chosen rows, the centres and the final w, the RELATIVE
MARGIN (s_second - s_first) / s_first of every round: a kernel whose fp32 s differs from the truth's by far less than the margin
must pick the same row.  assign() reports every row's relative margin between its nearest centre and the nearest centre that differs
from it in a coordinate the row observes: centres that agree bit for bit where the row looks (N < K repeats centres; two centres
with a gap in the same coordinate both hold `fill` there) give identical distances in any arithmetic, so the tie rule - the lowest
k - decides alike everywhere and such pairs carry no margin.  dtype = float32 rounds every operand once and keeps every
intermediate in fp32: the restatement whose error against the truth sets the bar of mind2_out (restatement_error)."""
import numpy as np

from mix_missfit_truth import make_data  # noqa: F401  (re-exported: row 0 fully missing, row 1 fully observed, NaN in the gaps)
from oracle import philox

SEED_TAG = 0x6b6d2b00


def words(seeds, rows, j):
    """(..., len(rows), 4) uint32: the Philox block of every (seed, row) in round j - counter (n low, n high, j, SEED_TAG), key = seed;
    `seeds` is one integer or an array of them (a leading axis)"""
    seeds = np.asarray(seeds, dtype=np.uint64)
    rows = np.asarray(rows, dtype=np.uint64)
    shape = seeds.shape + rows.shape
    ctr = np.zeros(shape + (4,), dtype=np.uint32)
    ctr[..., 0] = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[..., 1] = (rows >> np.uint64(32)).astype(np.uint32)
    ctr[..., 2] = np.uint32(j)
    ctr[..., 3] = np.uint32(SEED_TAG)
    key = np.zeros(shape + (2,), dtype=np.uint32)
    key[..., 0] = (seeds & np.uint64(0xFFFFFFFF)).astype(np.uint32)[..., None]
    key[..., 1] = (seeds >> np.uint64(32)).astype(np.uint32)[..., None]
    return philox.philox4x32(ctr, key)


def uniform(w, dtype=np.float64):
    """(top 24 bits + 1/2) 2^-24, rounded once to dtype and kept at most 1 - 2^-24"""
    w = np.asarray(w, dtype=np.uint32)
    return np.minimum((((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(dtype), dtype(1 - 2.0 ** -24))


def exponentials(seeds, N, j, dtype=np.float64):
    """E_nj = -log u(seed, n, j) for n = 0 .. N-1: (..., N)"""
    return -np.log(uniform(words(seeds, np.arange(N), j)[..., 0], dtype))


def race(E, w):
    """(s, winner, relative margin) of one round: s = E / w (+inf where w = 0), the winner the lowest n among the smallest s; the
    margin is (s_second - s_first) / s_first, +inf when there is no finite second or when every s is +inf (the tie rule alone
    decides: row 0)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(w > 0, E / w, np.inf)
    i = int(np.argmin(s))                               # numpy returns the first of equal minima
    rest = np.delete(s, i)
    if not np.isfinite(s[i]) or rest.size == 0 or not np.isfinite(rest.min()):
        return s, i, np.inf
    return s, i, float((rest.min() - s[i]) / s[i])


def observed(x, miss):
    """(bool mask of missing entries, x with 0 in them) - miss=None: every entry observed"""
    x = np.asarray(x)
    gone = np.zeros(x.shape, bool) if miss is None else np.asarray(miss) != 0
    return gone, np.where(gone, 0, x)


def fill_of(x, miss):
    """(D,) fp32 column means over the observed entries (0 for a column with none): the fill of models/_mix.py mean_filled"""
    gone, xz = observed(x, miss)
    return (xz.astype(np.float64).sum(0) / np.maximum((~gone).sum(0), 1)).astype(np.float32)


def filled(x, miss, fill):
    """x~: fp32 rows with `fill` in their missing slots"""
    gone, xz = observed(x, miss)
    return np.where(gone, np.asarray(fill, np.float32)[None, :], xz).astype(np.float32)


def dist2(x, miss, c, dtype=np.float64):
    """(N,) partial-distance rule: (D / D_o) sum over the observed coordinates of (x - c)^2, 0 when D_o = 0.  float32: every operand
    rounded once, the sum taken coordinate by coordinate in fp32"""
    gone, xz = observed(x, miss)
    D = xz.shape[1]
    xz, c = xz.astype(dtype), np.asarray(c).astype(dtype)
    s = np.zeros(xz.shape[0], dtype)
    for d in range(D):
        t = np.where(gone[:, d], dtype(0), xz[:, d] - c[d])
        s = s + t * t
    n_obs = (~gone).sum(1)
    return np.where(n_obs > 0, s * (dtype(D) / np.maximum(n_obs, 1).astype(dtype)), dtype(0)).astype(dtype)


def centers(x, miss, fill, K, seed, dtype=np.float64):
    """dict(index (K,) int64, centers (K,D) fp32 = the bits of x~ at those rows, w (N,) after the last round, margin (K,))"""
    gone, _ = observed(x, miss)
    N, D = gone.shape
    xt = filled(x, miss, np.zeros(D, np.float32) if fill is None else fill)
    w = ((~gone).sum(1) > 0).astype(dtype)
    index, margin = np.zeros(K, np.int64), np.zeros(K)
    for j in range(K):
        _, index[j], margin[j] = race(exponentials(seed, N, j, dtype), w)
        d2 = dist2(x, miss, xt[index[j]], dtype)
        w = d2 if j == 0 else np.minimum(w, d2)
    return dict(index=index, centers=xt[index], w=w, margin=margin)


def assign(x, miss, cen, smooth=0.0, dtype=np.float64):
    """dict(z (N,) int32, r (N,K) fp32, margin (N,)): z the nearest centre, ties to the lowest k, -1 for a row that observes nothing;
    r = (1 - smooth) onehot + smooth / K formed in fp32, 1 / K in a row with z = -1; margin as the module docstring has it"""
    gone, _ = observed(x, miss)
    cen = np.asarray(cen, np.float32)
    N, K = gone.shape[0], cen.shape[0]
    d = np.stack([dist2(x, miss, cen[k], dtype) for k in range(K)], axis=1)           # N,K
    z = np.argmin(d, axis=1).astype(np.int32)
    first = d[np.arange(N), z]
    same = np.all(gone[:, None, :] | (cen[None, :, :] == cen[z][:, None, :]), axis=2)   # N,K: equal to the nearest where n observes
    other = np.where(same, np.inf, d)
    second = other.min(1) if K > 1 else np.full(N, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        margin = np.where(second > first, (second - first) / first, 0.0)
    margin = np.where(np.isinf(second), np.inf, margin)
    nothing = (~gone).sum(1) == 0
    z[nothing] = -1
    margin[nothing] = np.inf
    s = np.float32(smooth)
    lo = s / np.float32(K)
    hi = (np.float32(1) - s) + lo
    r = np.full((N, K), lo, np.float32)
    r[np.arange(N), np.maximum(z, 0)] = hi
    r[nothing] = np.float32(1) / np.float32(K)
    return dict(z=z, r=r, margin=margin)


def restatement_error(x, miss, fill, K, seed, t64=None):
    """max |w32 - w64| / max(1, |w64|) of the final w, fp32 restatement against the truth (both must have chosen the same rows)"""
    t64 = centers(x, miss, fill, K, seed, np.float64) if t64 is None else t64
    t32 = centers(x, miss, fill, K, seed, np.float32)
    assert np.array_equal(t64['index'], t32['index'])
    return float(np.max(np.abs(t32['w'].astype(np.float64) - t64['w']) / np.maximum(1.0, np.abs(t64['w']))))


def four_clusters(seed, N=2048, M=512, frac=0.0):
    """(x (N,3), x_val (M,3), miss (N,3) uint8): four unit-variance clusters at the corners of a regular tetrahedron of edge 8 - eight
    standard deviations apart -, M held-out rows and a mask with about `frac` missing (the rows of x are returned complete)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float) * (8 / (2 * np.sqrt(2)))
    x = (c[rng.integers(0, 4, N + M)] + rng.standard_normal((N + M, 3))).astype(np.float32)
    miss = (rng.random((N, 3)) < frac).astype(np.uint8)
    return x[:N], x[N:], miss


# ---- the fixtures of tests/test_mix_seed_gpu.py ------------------------------------------------------------------------------
# (N, D, K): every N, D and K of the sweep occurs.  The geometry of csrc/vmp_seed.hip is one block of four waves per 1024 rows and
# 64 rows per wave step: 1025 needs two blocks; at 129 the rows per wave are 64, wave 2 holds one row and wave 3 none (at 1, 2, 3, 63
# and 64 waves 1 .. 3 hold none).  N < K: (3, 3, 5), (3, 8, 64), (63, 5, 64); the only row of (1, 1, 1) observes nothing under a mask.
SWEEP = [(1, 1, 1), (2, 2, 2), (3, 3, 5), (3, 8, 64), (63, 5, 64), (64, 8, 17), (65, 1, 16), (129, 2, 5), (257, 8, 16), (1000, 3, 17),
         (1025, 5, 2), (4099, 8, 64), (4099, 2, 16)]
UNALIGNED = [(257, 8, 16), (129, 2, 5)]
DRAW_SEED = 0x5eed00000001          # above 2^32: both key words are in use
# data seeds are base + salt with the salt chosen HERE, on the CPU, so that the truth alone has a margin >= 1e-3 in every round
# (find_salt); cases that are not listed use salt 0
SALT = {}
MARGIN = 1e-3
Z_MARGIN = 1e-4


def case(N, D, K, masked):
    """(x fp32 with NaN in its missing slots, miss uint8 or None, fill or None) of a sweep case"""
    salt = SALT.get((N, D, K, masked), 0)
    x, _, miss = make_data(N, D, max(K, 2), 1000 * N + 10 * D + K + 100000 * salt, frac=0.3)
    if not masked:
        rng = np.random.Generator(np.random.PCG64(7 + N + salt))
        x = np.where(np.isnan(x), rng.standard_normal(x.shape).astype(np.float32), x).astype(np.float32)
        return x, None, None
    return x, miss, fill_of(x, miss)


def find_salt(N, D, K, masked, tries=50):
    """the first salt whose case meets the fixture conditions under the truth alone (run by hand when the sweep changes)"""
    for salt in range(tries):
        SALT[(N, D, K, masked)] = salt
        x, miss, fill = case(N, D, K, masked)
        c = centers(x, miss, fill, K, DRAW_SEED)
        a = assign(x, miss, c['centers'])
        undecided = int((a['margin'] <= Z_MARGIN).sum())
        if c['margin'].min() >= MARGIN and undecided <= min(0.005 * N, 4 if N < 800 else N):
            return salt
    raise AssertionError((N, D, K, masked))
