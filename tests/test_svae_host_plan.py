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


def _plan(lib, direction, N, K, L, S, f0, f1, f2, f3):
    import ctypes
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    return lib.vmp_svae_launch_plan(direction, N, K, L, S, f0, f1, f2, f3, out), list(out)


def test_launch_plan_agrees_with_the_recorded_queries():
    """vmp_svae_launch_plan (which form a shape takes: fwd_plan / bwd_plan as they stand) against the older queries on every row of the
    golden: vmp_svae_rng_in_kernel, vmp_svae_fwd_mom_blocks, vmp_svae_bwd_blocks_for, vmp_svae_bwd_tail_applies[_t].  Shapes the
    entry points refuse are refused (out zeroed); vmp_svae_rng_in_kernel, _fwd_mom_blocks and _bwd_tail_applies[_t] answer 0 there."""
    lib = _lib()
    with np.load(FIXTURE) as f:
        table = f['table'].tolist()
    bad, forms_f, forms_b = [], set(), set()
    for K, L, S, N, rng_in, mom_blocks, blocks, blocks_for, blocks_for_t, tail, tail_t in table:
        valid = N >= 1 and 1 <= K <= 64 and 1 <= L <= 8
        rc, at = _plan(lib, 0, max(N, 1), K, L, S, 1, 1, 0, 0)                     # the streaming in-kernel-noise form, whatever N
        rcf, fwd = _plan(lib, 0, N, K, L, S, 1, 1, 0, 1)
        rcm, mom = _plan(lib, 0, N, K, L, S, 1, 1, 1, 1)
        rcb, bwd = _plan(lib, 1, N, K, L, S, 0, 1, 0, 0)
        rct, bwd_t = _plan(lib, 1, N, K, L, S, 1, 1, 0, 0)
        if not valid:
            # refused, out zeroed (vmp_svae_rng_in_kernel has no N: the plan is asked at N = 1)
            assert rcf != 0 and rcm != 0 and rcb != 0 and rct != 0 and fwd == mom == bwd == bwd_t == [0] * 8, (K, L, S, N)
            kl_ok = 1 <= K <= 64 and 1 <= L <= 8
            assert (rc == 0) == kl_ok
            # (vmp_svae_bwd_blocks_for does not look at L: it is not compared on these rows)
            got = (int(kl_ok and at[0] != 0), 0, 0, 0)
            want = (rng_in, mom_blocks, tail, tail_t)
        else:
            assert rc == rcf == rcm == rcb == rct == 0
            got = (int(at[0] != 0), mom[2], bwd[1], bwd_t[1], bwd[2], bwd_t[2])
            want = (rng_in, mom_blocks, blocks_for, blocks_for_t, tail, tail_t)
            forms_f.add(fwd[0])
            forms_b.update((bwd[0], bwd_t[0]))
            # the plan is whole: a form has waves and blocks, no form has none; the minibatch form is one block per tile
            assert (fwd[0] == 0) == (fwd[1] == 0 and fwd[2] == 0) and all(v == 0 for v in fwd[5:] + bwd[3:])
            if fwd[0] == 1:
                assert fwd[2] == -(-N // (64 // K)) and fwd[1] == (S + 1) // 2 and fwd[3] == 0
            if bwd[0] == 1:
                assert bwd[1] == -(-N // (64 // K)) and bwd[2] == 1
            # the partial rows of vmp_svae_estep_bwd (vmp_svae_bwd_blocks) are a plan too; any other count is none
            rcn, bwd_n = _plan(lib, 1, N, K, L, S, 0, 1, blocks, 0)
            assert rcn == 0 and bwd_n[0] != 0 and bwd_n[1] == blocks, (K, L, S, N, bwd_n)
            rcn, bwd_n = _plan(lib, 1, N, K, L, S, 0, 1, blocks + blocks_for + 1, 0)
            assert rcn == 0 and bwd_n[0] == 0 and bwd_n[1] == 0
        if tuple(got) != tuple(want):
            bad.append(((K, L, S, N), got, want))
    assert not bad, '%d of %d rows differ, first: %s' % (len(bad), len(table), bad[:3])
    assert forms_f == {0, 1, 2, 3, 4} and forms_b == {1, 2, 3, 4}, (forms_f, forms_b)     # every in-kernel-noise / backward form is on the grid
    # the noise-tensor forms: tile, chunked (a cell's noise block beyond the LDS tile), fwd3 (L S no multiple of 4, or misaligned)
    assert [_plan(lib, 0, 100, 10, 6, 10, 0, al, 0, 1)[1][0] for al in (1, 0)] == [2, 6]
    assert _plan(lib, 0, 21, 10, 2, 100, 0, 1, 0, 1)[1][0] == 5 and _plan(lib, 0, 5, 3, 2, 3, 0, 1, 0, 1)[1][0] == 6


def test_launch_plan_refuses_bad_arguments():
    lib = _lib()
    E_BADARG, E_DIM = -1, -2
    ok = (0, 100, 16, 8, 10, 1, 1, 0, 1)
    assert _plan(lib, *ok)[0] == 0
    assert lib.vmp_svae_launch_plan(*ok, None) == E_BADARG
    for i, v, code in ((0, 2, E_BADARG), (0, -1, E_BADARG), (1, 0, E_BADARG), (1, -5, E_BADARG), (2, 0, E_DIM), (2, 65, E_DIM),
                       (3, 0, E_DIM), (3, 9, E_DIM), (4, 0, E_BADARG), (4, (1 << 16) + 1, E_DIM), (5, 2, E_BADARG), (6, -1, E_BADARG),
                       (7, 2, E_BADARG), (8, 3, E_BADARG)):
        a = list(ok)
        a[i] = v
        rc, out = _plan(lib, *a)
        assert rc == code and out == [0] * 8, (i, v, rc, out)
    okb = (1, 100, 16, 8, 10, 0, 1, 0, 0)
    assert _plan(lib, *okb)[0] == 0
    for i, v in ((5, 2), (6, -1), (7, -1), (8, 1)):
        a = list(okb)
        a[i] = v
        rc, out = _plan(lib, *a)
        assert rc == E_BADARG and out == [0] * 8, (i, v, rc, out)


if __name__ == '__main__':
    lib_ = _lib()
    rows = [_answers(lib_, K, L, S, N, 1 <= K <= 64) for K, L, S, N in itertools.product(KS, LS, SS, NS)]
    np.savez_compressed(sys.argv[1], table=np.asarray(rows, dtype=np.int32), columns=np.asarray(COLUMNS))
    print('%d rows -> %s' % (len(rows), sys.argv[1]))
