"""What a caller of the fit-pack and impute-pack kernels must allocate, pinned: the pack widths and workspace sizes that the pure-host
functions of csrc/vmp_missfit.hip, vmp_wfit.hip, vmp_bound.hip and vmp_impute.hip answer (no launch, no device needed), over the
block-count edges of stream_blocks for the two geometries (512 rows x 512 blocks: the fits; 256 rows x 2048 blocks: bound, impute).
tests/golden/fit_pack_sizes.npz holds what the library answered at the commit before csrc/vmp_fit_cell.h and csrc/vmp_impute_pack.h
replaced the per-file FIT_* / WF_* constants and Geo structs; every row is replayed.

Re-recording (only ever against a library whose answers are the reference):
    VMP_LIB_PATH=/path/to/libvmp_hip.so python tests/test_fit_pack_sizes.py tests/golden/fit_pack_sizes.npz
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'fit_pack_sizes.npz')

NS = (1, 4, 511, 512, 513, 262143, 262144, 262145, 524288, 524289, 10 ** 6, 10 ** 7)
DS = tuple(range(10))
KS = (0, 1, 16, 17, 64, 65)
WORDS = ('vmp_mixture_fit_pack_words', 'vmp_mixture_impute_pack_words')
BYTES = ('vmp_mixture_fit_workspace_bytes', 'vmp_mixture_wfit_workspace_bytes', 'vmp_mixture_bound_workspace_bytes',
         'vmp_mixture_impute_workspace_bytes')
WORD_COLUMNS = ('D',) + WORDS
BYTE_COLUMNS = ('N', 'D', 'K') + BYTES


def _lib():
    sys.path.insert(0, ROOT)
    import vmp_for_svae_amd as V
    return V._lib.lib()


def _words(lib):
    return [(D,) + tuple(getattr(lib, f)(D) for f in WORDS) for D in DS]


def _bytes(lib):
    return [(N, D, K) + tuple(getattr(lib, f)(N, D, K) for f in BYTES) for N, D, K in itertools.product(NS, DS, KS)]


def _tables():
    with np.load(FIXTURE) as f:
        assert tuple(str(c) for c in f['word_columns']) == WORD_COLUMNS and tuple(str(c) for c in f['byte_columns']) == BYTE_COLUMNS
        return f['words'], f['bytes']


def test_pack_words_answer_as_recorded():
    words, _ = _tables()
    assert words.shape == (len(DS), len(WORD_COLUMNS))
    assert words.tolist() == [list(r) for r in _words(_lib())]


def test_workspace_bytes_answer_as_recorded():
    _, table = _tables()
    got = _bytes(_lib())
    assert table.shape == (len(got), len(BYTE_COLUMNS)) and len(got) == 12 * 10 * 6
    assert [tuple(r) for r in table[:, :3].tolist()] == [r[:3] for r in got]            # the whole grid, in order
    bad = [(row, g) for row, g in zip(table.tolist(), got) if row != list(g)]
    assert not bad, '%d of %d rows differ, first: %s' % (len(bad), len(got), bad[:3])


def test_recording_is_not_trivial():
    words, t = _tables()
    col = lambda c: t[:, BYTE_COLUMNS.index(c)]
    in_range = (col('D') >= 1) & (col('D') <= 8) & (col('K') >= 1) & (col('K') <= 64)
    assert in_range.any() and (~in_range).any()
    for f in BYTES[:3]:                                                     # out of range: 0; in range: something to allocate
        assert not col(f)[~in_range].any() and col(f)[in_range].all()
    assert col(BYTES[3]).all()                                              # the impute workspace does not look at D or K
    # the fits: 1 .. 512 blocks of 4 waves, K * (1 + D + D (D + 1) / 2) fp64 words per wave; wfit adds one fp64 partial per block
    fit, wfit = col(BYTES[0])[in_range], col(BYTES[1])[in_range]
    per_block = 4 * col('K')[in_range] * (1 + col('D')[in_range] + col('D')[in_range] * (col('D')[in_range] + 1) // 2) * 8
    blocks = fit // per_block
    assert (fit == blocks * per_block).all() and (wfit == fit + 8 * blocks).all()
    assert set(blocks.tolist()) == {1, 2, 512}                              # N <= 512, N = 513, every N from 262 143 on
    assert set((col(BYTES[2])[in_range] // 8).tolist()) == {1, 2, 3, 1024, 1025, 2048}      # bound: blocks of 256 rows, at most 2048
    assert (col(BYTES[2])[in_range] == col(BYTES[3])[in_range]).all()
    in_d = (words[:, 0] >= 1) & (words[:, 0] <= 8)
    assert not words[~in_d][:, 1:].any() and words[in_d][:, 1:].all()
    assert words[in_d][:, 1].tolist() == [3, 6, 10, 15, 21, 28, 36, 45] and words[in_d][:, 2].tolist() == [8, 12, 17, 23, 30, 38, 47, 57]


if __name__ == '__main__':
    lib_ = _lib()
    w_, b_ = _words(lib_), _bytes(lib_)
    np.savez_compressed(sys.argv[1], words=np.asarray(w_, dtype=np.int64), word_columns=np.asarray(WORD_COLUMNS),
                        bytes=np.asarray(b_, dtype=np.int64), byte_columns=np.asarray(BYTE_COLUMNS))
    print('%d + %d rows -> %s' % (len(w_), len(b_), sys.argv[1]))
