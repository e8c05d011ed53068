"""Fixtures of the seeded start of the diagonal-covariance mixture on wide rows (csrc/vmp_diagseed.hip; include/vmp_hip.h
"Diagonal-covariance mixture: seeded start on wide rows") for tests/test_mix_diagseed_*.py, CPU only.  The fp64 truth is
tests/mix_seed_truth.py (numpy, generic in D) with miss = None; here are the sweep, its data and the salts.

mix_seed_truth.case builds on mix_missfit_truth.make_data, which is generic in D but plants NaN and a fully missing row 0 for the
masked kernels; the complete rows of this sweep come from mix_diag_truth.make_data (clusters of per-coordinate spread 0.5 .. 1.5
around centres drawn at 3 standard deviations per coordinate), which reaches D = 64 as it is.

Geometry of csrc/vmp_diagseed.hip: one block of four waves per 1024 rows (at most 1024 blocks, 512 above D = 32), wave g owns
rows_per_wave = ceil(ceil(N / (4 blocks)) / 64) 64 rows and walks them in tiles of 64.  With one block: N <= 64 wave 0 alone, 65 puts
one row in wave 1, 129 one in wave 2, 193 one in wave 3, 257 starts a second tile in wave 0; 1025 needs two blocks; 525313 rows at
D = 33 would be 513 blocks and are capped at 512 (320 rows per wave, five tiles, the last waves empty).  Instantiation is per D."""
import numpy as np

import mix_diag_truth as DT
import mix_seed_truth as T

MARGIN = T.MARGIN                   # 1e-3: the race margin every round of every case must have under the fp64 truth alone
Z_MARGIN = T.Z_MARGIN               # 1e-4: rows with a smaller assignment margin are left out of the z / r comparison
DRAW_SEED = T.DRAW_SEED

# the sweep of the issue, then one N on either side of every wave / tile / block boundary that the sweep does not already have
SWEEP = [(1, 9, 1), (3, 64, 5), (63, 17, 64), (64, 33, 17), (65, 16, 16), (129, 49, 5), (257, 64, 16), (1025, 24, 2), (2049, 64, 64),
         (4099, 9, 33), (257, 8, 16), (129, 2, 5),
         (128, 10, 3), (192, 31, 4), (193, 32, 4), (256, 63, 7), (1024, 40, 8)]
CAPPED = (525313, 33, 2)            # the block cap above D = 32
SAME_AS_SEED_KERNELS = [(257, 8, 16), (129, 2, 5)]
UNALIGNED = [(257, 64, 16), (129, 49, 5), (65, 16, 16)]

# data seeds are base + 100000 salt with the salt chosen HERE, on the CPU, so that the truth alone meets the fixture conditions
# (find_salt; run `python tests/mix_diagseed_truth.py` when the sweep changes); cases that are not listed use salt 0
SALT = {}


def case(N, D, K):
    """x (N,D) fp32, complete rows, clustered"""
    salt = SALT.get((N, D, K), 0)
    return DT.make_data(N, D, max(K, 2), 1000 * N + 10 * D + K + 100000 * salt, r_rows=1)[0]


def allowed_undecided(N):
    return min(0.005 * N, 4) if N < 800 else 0.005 * N


def truth(N, D, K):
    """dict(x, c = mix_seed_truth.centers, a = mix_seed_truth.assign on those centres) under fp64"""
    x = case(N, D, K)
    c = T.centers(x, None, None, K, DRAW_SEED)
    return dict(x=x, c=c, a=T.assign(x, None, c['centers']))


def fixture_ok(t):
    """the conditions the tests assert on a fixture before they compare anything"""
    N = t['x'].shape[0]
    undecided = int((t['a']['margin'] <= Z_MARGIN).sum())
    return t['c']['margin'].min() >= MARGIN and undecided <= allowed_undecided(N)


def find_salt(N, D, K, tries=50):
    """the first salt whose case meets the fixture conditions under the truth alone"""
    for salt in range(tries):
        SALT[(N, D, K)] = salt
        if fixture_ok(truth(N, D, K)):
            return salt
    raise AssertionError((N, D, K))


# ---- the end-to-end fixture: four clusters eight standard deviations apart in D = 24 -------------------------------------------------
# data seed 0; draw seed 1 for both starts, chosen HERE under the fp64 truth alone (mix_diag_truth.iterate, ten iterations, default prior):
# draw seeds 0 .. 3 give bound gaps 0.172, 1366.661, 1601.615, 0.001 nats - with seeds 0 and 3 the Dirichlet start happens to
# separate the four clusters within ten iterations as well, and the gap is below what an fp32 data term resolves at |bound| = 7e4
E2E = dict(N=2048, D=24, K=4, sep=8.0, data_seed=0, seed=1, iterations=10)


def four_clusters_wide():
    """x (2048, 24) fp32: mix_diag_truth.planted_clusters - unit-variance clusters, centre k on axis k, pairwise 8 sd apart"""
    return DT.planted_clusters(E2E['N'], E2E['D'], E2E['K'], E2E['sep'], E2E['data_seed'])[0]


def dirichlet_r_init(N, K, seed):
    """the start of gmm.inference_diag(init='random') (models/gmm.py _dirichlet_init): Dirichlet(1) rows from normalised
    exponentials of torch's host generator, fp32"""
    import torch
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    e = -torch.log(torch.rand(N, K, generator=g).clamp_min(1e-30))
    return (e / e.sum(1, keepdim=True)).numpy()


if __name__ == '__main__':
    for shape in SWEEP + [CAPPED]:
        print(shape, find_salt(*shape))
