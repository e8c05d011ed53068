"""The fp64 truth of mixture initialisation (tests/mix_seed_truth.py; include/vmp_hip.h "Mixture initialisation") checked on its own,
on the CPU: the bit layout of the uniforms, the exponential race as exact D^2-sampling, the rows that observe nothing, N < K and the
masked distance against the unmasked one."""
import numpy as np

import mix_seed_truth as T
from oracle import philox


def test_uniforms_have_the_stated_bit_layout():
    w = np.array([0x00000000, 0x000000FF, 0x00000100, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.uint32)
    top = np.array([0, 0, 1, 1 << 23, (1 << 24) - 2, (1 << 24) - 1], dtype=np.float64)
    u64 = T.uniform(w, np.float64)
    assert np.array_equal(u64[:5], (top[:5] + 0.5) * 2.0 ** -24)                # exact in fp64; the low 8 bits never enter
    assert u64[5] == 1 - 2.0 ** -24                                             # (2^24 - 1/2) 2^-24 is kept at most 1 - 2^-24
    u32 = T.uniform(w, np.float32)
    assert u32.dtype == np.float32
    assert u32[0] == np.float32(2.0 ** -25) and u32[2] == np.float32(1.5 * 2.0 ** -24) and u32[3] == np.float32(0.5 + 2.0 ** -25)
    assert u32[4] == np.float32(1 - 2.0 ** -23)          # 16777214.5 needs 25 bits: rounded once, ties to even
    assert u32[5] == np.float32(1 - 2.0 ** -24)          # would round to 1.0: kept at the largest fp32 below 1
    assert np.all((u32 > 0) & (u32 < 1))


def test_counter_and_key_layout():
    seed, rows, j = 0x0123456789abcdef, np.array([0, 5, (1 << 32) + 7], dtype=np.uint64), 3
    got = T.words(seed, rows, j)
    for i, n in enumerate(rows.tolist()):
        ctr = np.array([n & 0xFFFFFFFF, n >> 32, j, 0x6b6d2b00], dtype=np.uint32)
        key = np.array([0x89abcdef, 0x01234567], dtype=np.uint32)
        assert np.array_equal(got[i], philox.philox4x32(ctr, key)), n
    assert not np.array_equal(got[1], T.words(seed, rows, j + 1)[1])            # the round enters
    many = T.words(np.array([1, 2], dtype=np.uint64), np.arange(4), 0)          # a leading axis of seeds
    assert many.shape == (2, 4, 4) and np.array_equal(many[1], T.words(2, np.arange(4), 0))


def test_the_race_is_exact_d2_sampling():
    """12 rows with given w; the round-1 pick over 20 000 seeds follows w / sum w.  Chi-square with 11 degrees of freedom; the bar is
    its 1 - 1e-6 quantile, 52.4 - no tuning: the truth is exact sampling."""
    w = np.array([0.1, 0.5, 1.0, 2.0, 4.0, 0.25, 3.0, 1.5, 0.05, 6.0, 0.75, 5.0])
    S = 20000
    E = T.exponentials(np.arange(S, dtype=np.uint64) + 12345, 12, 1)            # (S, 12)
    pick = np.argmin(E / w, axis=1)
    counts = np.bincount(pick, minlength=12)
    p = w / w.sum()
    chi2 = float(((counts - S * p) ** 2 / (S * p)).sum())
    print('chi2 = %.2f' % chi2)
    assert chi2 < 52.4
    w0 = w.copy()
    w0[[0, 8]] = 0.0                                                            # a weight of 0 is never chosen
    with np.errstate(divide='ignore'):
        assert not np.isin(np.argmin(np.where(w0 > 0, E / w0, np.inf), axis=1), [0, 8]).any()
    for i, (sv, wi, mg) in enumerate(T.race(E[k], w) for k in range(50)):       # race() agrees with the vectorised pick
        assert wi == pick[i] and mg >= 0


def test_rows_that_observe_nothing_are_never_picked_and_get_no_component():
    for seed in range(8):
        x, _, miss = T.make_data(40, 3, 4, seed, frac=0.4)
        gone = miss != 0
        nothing = np.flatnonzero((~gone).sum(1) == 0)
        assert 0 in nothing
        c = T.centers(x, miss, T.fill_of(x, miss), 6, 99 + seed)
        assert not np.isin(c['index'], nothing).any()
        assert np.all(c['w'][nothing] == 0) and np.all(np.isfinite(c['w']))
        assert np.all(np.isfinite(c['centers']))                                # NaN in a missing slot never surfaces: fill stands there
        a = T.assign(x, miss, c['centers'], smooth=0.1)
        assert np.all(a['z'][nothing] == -1) and np.all(a['z'][np.setdiff1d(np.arange(40), nothing)] >= 0)
        assert np.all(a['r'][nothing] == np.float32(1) / np.float32(6))
        assert np.allclose(a['r'].sum(1), 1, atol=1e-6)


def test_fewer_rows_than_centres_repeats_them():
    x, _, _ = T.make_data(3, 2, 2, 5, frac=0.0)
    x = np.nan_to_num(x)                                                        # make_data empties row 0
    c = T.centers(x, None, None, 5, 11)
    assert sorted(set(c['index'][:3].tolist())) == [0, 1, 2]                    # three rounds take the three rows ...
    assert np.all(c['index'][3:] == 0) and np.all(np.isinf(c['margin'][3:]))    # ... then every w is 0: the tie rule, row 0
    assert np.all(c['w'] == 0)
    assert np.array_equal(c['centers'], x[c['index']])
    a = T.assign(x, None, c['centers'])
    assert np.array_equal(a['z'], [int(np.flatnonzero(c['index'] == n)[0]) for n in range(3)])   # the lowest k of equal centres
    assert np.all(np.isinf(a['margin']) | (a['margin'] > 0))


def test_an_all_zero_mask_is_no_mask():
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.standard_normal((50, 5)).astype(np.float32)
    zero = np.zeros((50, 5), np.uint8)
    for dt in (np.float64, np.float32):
        assert np.array_equal(T.dist2(x, zero, x[7], dt), T.dist2(x, None, x[7], dt))
    a, b = T.centers(x, zero, np.zeros(5, np.float32), 4, 21), T.centers(x, None, None, 4, 21)
    assert np.array_equal(a['index'], b['index']) and np.array_equal(a['w'], b['w'])
    d = T.dist2(x, None, x[7])
    assert d[7] == 0 and np.allclose(d, ((x.astype(np.float64) - x[7].astype(np.float64)) ** 2).sum(1), rtol=1e-14)


def test_the_sweep_fixtures_meet_their_conditions_under_the_truth_alone():
    """what tests/test_mix_seed_gpu.py asserts of its fixtures, here for the cheap half of the sweep (the GPU test asserts all of it)"""
    for (N, D, K) in T.SWEEP:
        if N * K > 20000:
            continue
        for masked in (False, True):
            x, miss, fill = T.case(N, D, K, masked)
            c = T.centers(x, miss, fill, K, T.DRAW_SEED)
            assert c['margin'].min() >= T.MARGIN, (N, D, K, masked, c['margin'].min())
