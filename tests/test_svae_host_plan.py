"""The SVAE E-step's host decisions, pinned: the pure host queries of include/vmp_hip.h (no launch, no device needed) answer, over a
grid of shapes, what the library answered at the commit before the launch plans (FwdPlan / BwdPlan, csrc/vmp_svae.hip) replaced the
per-entry-point copies of the launch geometry.  tests/golden/svae_host_plan.npz holds that recording; every row is replayed.

Re-recording (only ever against a library whose answers are the reference):
    VMP_LIB_PATH=/path/to/libvmp_hip.so python tests/test_svae_host_plan.py tests/golden/svae_host_plan.npz
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'svae_host_plan.npz')

KS = (0, 1, 5, 7, 8, 9, 10, 12, 15, 16, 17, 32, 64, 65)
LS = tuple(range(1, 10))
SS = (1, 2, 4, 7, 10, 16, 17, 100)
NS = (0, 1, 64, 512, 1024, 1025, 4096, 10 ** 5, 10 ** 6)
COLUMNS = ('K', 'L', 'S', 'N', 'rng_in_kernel', 'fwd_mom_blocks', 'bwd_blocks', 'bwd_blocks_for', 'bwd_blocks_for_student',
           'bwd_tail_applies', 'bwd_tail_applies_t')
NO_ANSWER = -1        # vmp_svae_bwd_blocks at K outside 1..64: the recorded library divided by zero there, so it was not asked


def _answers(lib, K, L, S, N, ask_blocks):
    return (K, L, S, N, lib.vmp_svae_rng_in_kernel(K, L, S), lib.vmp_svae_fwd_mom_blocks(N, K, L, S),
            lib.vmp_svae_bwd_blocks(N, K) if ask_blocks else NO_ANSWER,
            lib.vmp_svae_bwd_blocks_for(N, K, L, S, 0), lib.vmp_svae_bwd_blocks_for(N, K, L, S, 1),
            lib.vmp_svae_bwd_tail_applies(N, K, L, S), lib.vmp_svae_bwd_tail_applies_t(N, K, L, S))


def _lib():
    sys.path.insert(0, ROOT)
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_host_queries_answer_as_recorded():
    lib = _lib()
    with np.load(FIXTURE) as f:
        table = f['table']
        assert tuple(str(c) for c in f['columns']) == COLUMNS
    grid = list(itertools.product(KS, LS, SS, NS))
    assert table.shape == (len(grid), len(COLUMNS)) and len(grid) == 14 * 9 * 8 * 9
    assert [tuple(r) for r in table[:, :4].tolist()] == grid                    # the issue's grid, whole and in order
    bad = []
    for row in table.tolist():
        K, L, S, N = row[:4]
        got = list(_answers(lib, K, L, S, N, True))
        want = list(row)
        if want[6] == NO_ANSWER:
            assert not 1 <= K <= 64
            want[6] = 0                                                         # no tiles of K-lane rows: no blocks
        if got != want:
            bad.append((want, got))
    assert not bad, '%d of %d rows differ, first: %s' % (len(bad), len(table), bad[:3])
    # the recording is not trivially constant: every decision is taken both ways somewhere on the grid
    for c in ('rng_in_kernel', 'bwd_tail_applies', 'bwd_tail_applies_t'):
        assert set(table[:, COLUMNS.index(c)].tolist()) == {0, 1}, c
    assert table[:, COLUMNS.index('fwd_mom_blocks')].max() == 256
    assert (table[:, COLUMNS.index('bwd_blocks_for')] != table[:, COLUMNS.index('bwd_blocks_for_student')]).any()


if __name__ == '__main__':
    lib_ = _lib()
    rows = [_answers(lib_, K, L, S, N, 1 <= K <= 64) for K, L, S, N in itertools.product(KS, LS, SS, NS)]
    np.savez_compressed(sys.argv[1], table=np.asarray(rows, dtype=np.int32), columns=np.asarray(COLUMNS))
    print('%d rows -> %s' % (len(rows), sys.argv[1]))
