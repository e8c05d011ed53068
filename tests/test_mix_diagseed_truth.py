"""The fixtures of the wide-row seeding sweep (tests/mix_diagseed_truth.py) under the fp64 truth of tests/mix_seed_truth.py, CPU only:
every case has a race margin >= MARGIN in every round and at most the allowed number of rows with an assignment margin <= Z_MARGIN,
and the fp32 restatement - the arithmetic a kernel may use - picks the same rows as fp64 on each."""
import functools

import numpy as np
import pytest

import mix_diagseed_truth as S
import mix_seed_truth as T

CASES = S.SWEEP + [S.CAPPED]


@functools.lru_cache(maxsize=None)
def _truth(N, D, K):
    return S.truth(N, D, K)


@pytest.mark.parametrize('N,D,K', CASES)
def test_the_fixture_meets_the_margin_conditions(N, D, K):
    t = _truth(N, D, K)
    assert t['x'].shape == (N, D) and t['x'].dtype == np.float32 and np.isfinite(t['x']).all()
    assert t['c']['margin'].min() >= S.MARGIN, t['c']['margin'].min()
    undecided = int((t['a']['margin'] <= S.Z_MARGIN).sum())
    assert undecided <= S.allowed_undecided(N), undecided
    assert S.fixture_ok(t)


@pytest.mark.parametrize('N,D,K', CASES)
def test_the_fp32_restatement_picks_the_same_rows(N, D, K):
    t = _truth(N, D, K)
    c32 = T.centers(t['x'], None, None, K, S.DRAW_SEED, np.float32)
    assert np.array_equal(c32['index'], t['c']['index'])
    assert np.array_equal(c32['centers'].view(np.uint32), t['c']['centers'].view(np.uint32))
    ok = t['a']['margin'] > S.Z_MARGIN
    a32 = T.assign(t['x'], None, t['c']['centers'], dtype=np.float32)
    assert np.array_equal(a32['z'][ok], t['a']['z'][ok])


def test_fewer_rows_than_centres_repeat_centres():
    for N, D, K in ((3, 64, 5), (63, 17, 64)):
        idx = _truth(N, D, K)['c']['index']
        assert len(set(idx.tolist())) <= N < K and idx.min() >= 0 and idx.max() < N


def test_the_sweep_covers_the_issue_and_the_geometry():
    issue = [(1, 9, 1), (3, 64, 5), (63, 17, 64), (64, 33, 17), (65, 16, 16), (129, 49, 5), (257, 64, 16), (1025, 24, 2),
             (2049, 64, 64), (4099, 9, 33), (257, 8, 16), (129, 2, 5)]
    assert S.SWEEP[:len(issue)] == issue
    ns = {n for n, _, _ in S.SWEEP}
    for edge in (64, 128, 192, 256, 1024):                 # a wave, a tile, a block fills up: one N on either side
        assert edge in ns and edge + 1 in ns, edge
    assert S.CAPPED[1] > 32 and -(-S.CAPPED[0] // 1024) > 512


def test_the_end_to_end_fixture_has_four_separated_clusters():
    x = S.four_clusters_wide()
    assert x.shape == (S.E2E['N'], S.E2E['D']) and x.dtype == np.float32
    r0 = S.dirichlet_r_init(S.E2E['N'], S.E2E['K'], S.E2E['seed'])
    assert r0.shape == (S.E2E['N'], S.E2E['K']) and np.allclose(r0.sum(1), 1, atol=1e-5)
