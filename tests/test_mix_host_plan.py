"""The mixture pass's host decisions, pinned: vmp_mix_pass_plan (include/vmp_hip.h; pure host, no launch, no device needed) answers,
over a grid of shapes and pass forms, what the library decided at the commit before pass_plan (csrc/vmp_mix.hip) replaced make_plan,
use_xdl and the two launch macros.  tests/golden/mix_host_plan.npz holds that recording - made with the same export added to the old
code, calling the old functions untouched; every row is replayed.  For the (estep, stats, mask) triples the old launch code could not
express, the recording holds what the old entry points answered: VMP_E_BADARG.

Re-recording (only ever against a library whose answers are the reference):
    VMP_LIB_PATH=/path/to/libvmp_hip.so python tests/test_mix_host_plan.py tests/golden/mix_host_plan.npz
"""
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'mix_host_plan.npz')

NS = (0, 1, 8, 63, 64, 65, 512, 513, 4096, 65535, 65536, 125000, 131072, 131073, 300007, 10 ** 6, 10 ** 7)
DS = tuple(range(10))
KS = (0, 1, 5, 15, 16, 17, 32, 33, 48, 49, 64, 65)
FLAVOURS = (0, 1, 2)
TRIPLES = tuple(itertools.product((0, 1), repeat=3))            # (estep, stats, mask)
KEYS = ('N', 'D', 'K', 'flavour', 'estep', 'stats', 'mask')
COLUMNS = KEYS + ('rc', 'form', 'kt_mt', 'nw', 'blocks', 'rpw', 'rpw_b', 'par_reduce', 'lds')
TILED, XDL = 1, 2


def _grid():
    return itertools.product(NS, DS, KS, FLAVOURS, TRIPLES)


def _answer(lib, N, D, K, fl, e, s, m):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    rc = lib.vmp_mix_pass_plan(N, D, K, fl, e, s, m, out)
    return (N, D, K, fl, e, s, m, rc) + tuple(out)


def _lib():
    sys.path.insert(0, ROOT)
    import vmp_for_svae_amd as V
    return V._lib.lib()


def _table():
    with np.load(FIXTURE) as f:
        assert tuple(str(c) for c in f['columns']) == COLUMNS
        return f['table']


def test_pass_plan_answers_as_recorded():
    lib = _lib()
    table = _table()
    grid = [(N, D, K, fl) + t for N, D, K, fl, t in _grid()]
    assert table.shape == (len(grid), len(COLUMNS)) and len(grid) == 17 * 10 * 12 * 3 * 8
    assert [tuple(r) for r in table[:, :len(KEYS)].tolist()] == grid               # the whole grid, in order
    bad = []
    for row in table.tolist():
        got = _answer(lib, *row[:len(KEYS)])
        if list(got) != row:
            bad.append((row, got))
    assert not bad, '%d of %d rows differ, first: %s' % (len(bad), len(table), bad[:3])


def test_recording_is_not_trivial():
    t = _table()
    col = lambda c: t[:, COLUMNS.index(c)]
    ok = col('rc') == 0
    assert ok.any() and (~ok).any()
    assert set(col('rc')[~ok].tolist()) == {-1, -2}                                  # VMP_E_BADARG, VMP_E_DIM
    assert not t[~ok][:, len(KEYS) + 1:].any()                                       # a refused plan is all zeros
    assert set(col('form')[ok].tolist()) == {TILED, XDL}
    assert set(col('kt_mt')[ok & (col('form') == XDL)].tolist()) == {2, 3}           # both MT
    assert set(col('kt_mt')[ok & (col('form') == TILED)].tolist()) == {1, 2, 4}      # every KT
    assert (col('rpw')[ok] != col('rpw_b')[ok]).any() and (col('rpw')[ok] == col('rpw_b')[ok]).any()      # split plans, and equal ones
    assert set(col('par_reduce')[ok].tolist()) == {0, 1}
    assert (col('nw')[ok] < 8).any() and (col('nw')[ok] == 8).any()
    assert (col('lds')[ok] > 65536).any()
    # legal: the M-pass, the E-pass, the fused E-pass, and the masked E-pass of the GMM
    legal = {(fl,) + tr for fl in (0, 1) for tr in ((0, 1, 0), (1, 0, 0), (1, 1, 0))} | {(0, 1, 0, 1)}
    for row in t[ok].tolist():
        assert tuple(row[3:7]) in legal, row
    in_range = (col('N') > 0) & (col('D') >= 1) & (col('D') <= 8) & (col('K') >= 1) & (col('K') <= 64)
    for row in t[in_range].tolist():
        assert (row[7] == 0) == (tuple(row[3:7]) in legal), row


def test_blocks_depend_on_N_K_and_flavour_only():
    """What finalize_kernel is told to reduce (partial_rows, csrc/vmp_mix.hip) is the M-pass plan's block count, whichever pass filled
    the workspace: every legal pass form - and every D - must give the same blocks at fixed (N, K, flavour)."""
    t = _table()
    t = t[t[:, COLUMNS.index('rc')] == 0]
    seen = {}
    for row in t.tolist():
        key = (row[0], row[2], row[3])
        seen.setdefault(key, set()).add(row[COLUMNS.index('blocks')])
    assert len(seen) == 16 * 10 * 2
    assert all(len(v) == 1 for v in seen.values()), {k: v for k, v in seen.items() if len(v) > 1}


if __name__ == '__main__':
    lib_ = _lib()
    rows = [_answer(lib_, N, D, K, fl, *tr) for N, D, K, fl, tr in _grid()]
    np.savez_compressed(sys.argv[1], table=np.asarray(rows, dtype=np.int64), columns=np.asarray(COLUMNS))
    print('%d rows -> %s' % (len(rows), sys.argv[1]))
