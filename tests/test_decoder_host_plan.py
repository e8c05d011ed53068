"""The decoder / encoder MLP launch layer's host decisions, pinned: vmp_decoder_launch_plan (include/vmp_hip.h; pure host, no launch, no
device needed) answers, over a grid of launch kinds and shapes, what the library decided at the commit before dec_plan
(csrc/vmp_decoder.hip) replaced dec_fwd_blocks, dec_bwd_blocks, the split / red_one / BT expressions of dec_bwd_launch and the seven
dispatch macros.  tests/golden/decoder_host_plan.npz holds that recording - made with the same export added to the old code, calling
the old functions and expressions untouched; every row is replayed.

Re-recording (only ever against a library whose answers are the reference):
    VMP_LIB_PATH=/path/to/libvmp_hip.so python tests/test_decoder_host_plan.py tests/golden/decoder_host_plan.npz
"""
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'decoder_host_plan.npz')

FWD, EVAL, PREP, BWD, BWD_GIN = range(5)                            # the `kind` of vmp_decoder_launch_plan
KINDS = (FWD, EVAL, PREP, BWD, BWD_GIN)
LS = tuple(range(10))
DYS = (0, 1, 2, 5, 8, 9)
US = (0, 1, 15, 16, 17, 32, 33, 48, 49, 50, 64, 65)
# both sides of: the few-tile / eight-wave switch of the backward grid (1024 tiles), its full grid (2048 tiles), the forward grid's
# cap (4096 blocks of 4 tiles), the BT = 2 threshold, the 2^31 refusal
ROWS = (0, 1, 16, 17, 4096, 4097, 16384, 16385, 32768, 32769, 262144, 262145, 2 ** 19 - 1, 2 ** 19, 10 ** 6, 42 * 10 ** 6, 2 ** 31 - 1, 2 ** 31)
KEYS = ('kind', 'rows', 'L', 'Dy', 'U', 'K')
COLUMNS = KEYS + ('rc', 'UT', 'FS', 'BT', 'split', 'red_one', 'blocks', 'threads', 'lds_bytes')
E_DIM = -2


def _ks(kind):
    return (16, 1, 64) if kind == PREP else (16,)


def _grid():
    return [(kind, rows, L, Dy, U, K) for kind in KINDS for rows, L, Dy, U in itertools.product(ROWS, LS, DYS, US) for K in _ks(kind)]


def _answer(lib, kind, rows, L, Dy, U, K):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    rc = lib.vmp_decoder_launch_plan(kind, rows, L, Dy, U, K, out)
    return (kind, rows, L, Dy, U, K, rc) + tuple(out)


def _lib():
    sys.path.insert(0, ROOT)
    import vmp_for_svae_amd as V
    return V._lib.lib()


def _table():
    with np.load(FIXTURE) as f:
        assert tuple(str(c) for c in f['columns']) == COLUMNS
        return f['table']


def _col(t, c):
    return t[:, COLUMNS.index(c)]


def test_launch_plan_answers_as_recorded():
    lib = _lib()
    table = _table()
    grid = _grid()
    assert table.shape == (len(grid), len(COLUMNS)) and len(grid) == (4 + 3) * 18 * 10 * 6 * 12
    assert [tuple(r) for r in table[:, :len(KEYS)].tolist()] == grid               # the whole grid, in order
    bad = []
    for row in table.tolist():
        got = _answer(lib, *row[:len(KEYS)])
        if list(got) != row:
            bad.append((row, got))
    assert not bad, '%d of %d rows differ, first: %s' % (len(bad), len(table), bad[:3])


def test_recording_is_not_trivial():
    t = _table()
    ok = _col(t, 'rc') == 0
    assert ok.any() and (~ok).any()
    assert set(_col(t, 'rc')[~ok].tolist()) == {E_DIM}
    assert not t[~ok][:, len(KEYS) + 1:].any()                                       # a refused plan is all zeros
    bwd = ok & (_col(t, 'kind') >= BWD)
    assert set(_col(t, 'UT')[ok].tolist()) == {1, 2, 3, 4} == set(_col(t, 'UT')[bwd].tolist())
    assert set(_col(t, 'FS')[bwd].tolist()) == {0, 1}
    assert set(_col(t, 'BT')[bwd].tolist()) == {2, 3}
    assert set(_col(t, 'red_one')[bwd].tolist()) == {0, 1}
    assert set(_col(t, 'split')[bwd].tolist()) == {54, 58}
    assert (_col(t, 'lds_bytes')[ok] > 65536).any()
    assert set(_col(t, 'threads')[bwd].tolist()) == {512} and set(_col(t, 'threads')[ok & ~bwd].tolist()) == {256}
    assert not t[ok & ~bwd][:, COLUMNS.index('FS'):COLUMNS.index('red_one') + 1].any()     # the forward kinds have no FS, BT, split, red_one
    # the 8 slabs of the epilogue fit the LDS at PW = 3896 (8, 8, 50) and not at PW = 5856 (8, 8, 64)
    lib = _lib()
    assert lib.vmp_decoder_param_words(8, 50, 8) == 3896 and lib.vmp_decoder_param_words(8, 64, 8) == 5856
    at = lambda U: bwd & (_col(t, 'L') == 8) & (_col(t, 'Dy') == 8) & (_col(t, 'U') == U)
    assert set(_col(t, 'red_one')[at(50)].tolist()) == {1} and set(_col(t, 'red_one')[at(64)].tolist()) == {0}
    # accepted: exactly what dec_check accepts, and for the prep kind at least one row
    for row in t.tolist():
        kind, rows, L, Dy, U, K, rc = row[:7]
        want = 1 <= L <= 8 and 1 <= Dy <= 8 and 1 <= U <= 64 and 0 <= rows < 2 ** 31 and (kind != PREP or rows >= 1)
        assert (rc == 0) == want, row
    # the prep kind: 2 K blocks behind the forward's
    fwd = {tuple(r[1:5]): r[COLUMNS.index('blocks')] for r in t[ok & (_col(t, 'kind') == FWD)].tolist()}
    for r in t[ok & (_col(t, 'kind') == PREP)].tolist():
        assert r[COLUMNS.index('blocks')] == fwd[tuple(r[1:5])] + 2 * r[5], r


def test_workspace_query_is_the_plans_blocks_times_the_parameter_words():
    lib = _lib()
    t = _table()
    t = t[(_col(t, 'rc') == 0) & (_col(t, 'kind') >= BWD)]
    assert len(t) == 2 * 17 * 8 * 4 * 10
    for kind, rows, L, Dy, U, K, rc, UT, FS, BT, split, red_one, blocks, threads, lds in t.tolist():
        assert lib.vmp_decoder_workspace_bytes(rows, 1, 1, L, U, Dy) == blocks * lib.vmp_decoder_param_words(L, U, Dy) * 4, (kind, rows, L, Dy, U)


def test_partial_row_query_is_the_plans_blocks():
    """vmp_decoder_bwd_blocks(rows) == blocks at every row count a launch happens at.  At rows = 0 nothing is launched and the query
    answers 0, while the plan (and vmp_decoder_workspace_bytes, test above) counts the one block a grid cannot go below: the old code's
    answers, kept."""
    lib = _lib()
    t = _table()
    t = t[(_col(t, 'rc') == 0) & (_col(t, 'kind') >= BWD)]
    seen = set()
    for row in t.tolist():
        rows, blocks = row[1], row[COLUMNS.index('blocks')]
        assert lib.vmp_decoder_bwd_blocks(rows) == (blocks if rows > 0 else 0), row
        assert blocks >= 1
        seen.add((rows, blocks))
    assert len(seen) == 17                                                           # the grid depends on the rows alone
    assert lib.vmp_decoder_bwd_blocks(0) == 0


if __name__ == '__main__':
    lib_ = _lib()
    rows_ = [_answer(lib_, *g) for g in _grid()]
    np.savez_compressed(sys.argv[1], table=np.asarray(rows_, dtype=np.int64), columns=np.asarray(COLUMNS))
    print('%d rows -> %s' % (len(rows_), sys.argv[1]))
