"""Where the shape tables of tests/mix_tiled_shapes.py land in the mixture pass's host plan (vmp_mix_pass_plan: pure host, no launch,
no device needed - as tests/test_mix_host_plan.py).  tests/test_mix_tiled_pass_gpu.py runs exactly these tables against the fp64
oracle; the assertions here are conditions on its INPUTS: if a table is edited and a branch of pass_kernel / pass_epilogue is no
longer reached, this module fails on a machine without a GPU."""
import os
import sys

import mix_tiled_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    sys.path.insert(0, ROOT)
    import vmp_for_svae_amd as V
    return V._lib.lib()


def _plans(shapes, mode, flavours=S.FLAVOURS):
    lib = _lib()
    return [((N, D, K, fl), S.plan(lib, N, D, K, fl, mode)) for N, D, K in shapes for fl in flavours]


def test_every_entry_meant_for_the_tiled_form_gets_it():
    for shapes, mode, flavours in ((S.STEP_SHAPES + S.SEVERAL, S.FUSED, S.FLAVOURS), (S.STEP_SHAPES, S.E_ONLY, S.FLAVOURS),
                                   (S.STATS_SHAPES, S.M_ONLY, S.FLAVOURS), (S.MASKED, S.E_MASKED, ('gmm',)),
                                   ([S.UNALIGNED[0], S.UNALIGNED[1], S.ODD_PACK], S.FUSED, S.FLAVOURS), (S.UNALIGNED, S.M_ONLY, S.FLAVOURS)):
        for (N, D, K, fl), p in _plans(shapes, mode, flavours):
            assert p['form'] == S.TILED and p['kt_mt'] == S.kt_of(K), (N, D, K, fl, mode, p)
    assert all(K > 16 for _, _, K in S.STEP_SHAPES + S.SEVERAL)
    assert all(K <= 16 for _, _, K in S.STATS_LOW_K)
    # the masked table holds both sides of K = 16 and every KT
    assert {S.kt_of(K) for _, _, K in S.MASKED} == {1, 2, 4}
    # the two unaligned shapes with K <= 16 are there for the XDL kernel's row loads
    for N, D, K in S.UNALIGNED[2:]:
        for mode in (S.FUSED, S.E_ONLY):
            assert all(p['form'] == S.XDL for _, p in _plans([(N, D, K)], mode))


def test_the_sweep_reaches_every_D_and_KT_in_every_pass_mode():
    want = {(D, KT) for D in range(1, 9) for KT in (2, 4)}
    for mode in (S.FUSED, S.E_ONLY, S.M_ONLY):
        for fl in S.FLAVOURS:
            got = {(D, p['kt_mt']) for (N, D, K, _), p in _plans(S.SWEEP, mode, (fl,))}
            assert got == want, (mode, fl, want - got)
    # per KT: a K that fills its tiles exactly, one with a single live lane in the last tile, and (KT = 4) a last tile wholly off
    ks = {K for _, _, K in S.SWEEP}
    assert {17, 32} <= ks and {33, 48, 49, 64} <= ks
    got = {(D, S.kt_of(K)) for _, D, K in S.MASKED}
    assert {D for D, _ in got} == {1, 3, 5, 8} and all((D, KT) in got for D in (1, 3, 5, 8) for KT in (1, 2, 4))


def test_both_block_reductions_occur_for_every_KT_and_block_size():
    for mode in (S.FUSED, S.M_ONLY):
        plans = _plans(S.STATS_SHAPES if mode == S.M_ONLY else S.STEP_SHAPES, mode)
        for KT in (2, 4):
            assert {p['par_reduce'] for _, p in plans if p['kt_mt'] == KT} == {0, 1}, (mode, KT)
            # the parallel branch with fewer waves than its compile-time bound (the w < nw guard), and at D >= 5
            assert any(p['par_reduce'] == 1 and p['nw'] < 8 for _, p in plans if p['kt_mt'] == KT), (mode, KT)
            assert any(p['par_reduce'] == 1 and k[1] >= 5 for k, p in plans if p['kt_mt'] == KT), (mode, KT)
        # ... with all eight waves (KT = 2, D <= 4), and the serial branch with fewer than eight (KT = 4, D >= 5)
        assert any(p['par_reduce'] == 1 and p['nw'] == 8 for _, p in plans), mode
        assert any(p['par_reduce'] == 0 and p['nw'] < 8 for _, p in plans), mode
        assert any(p['par_reduce'] == 0 and p['nw'] == 8 for _, p in plans), mode
        assert {p['nw'] for _, p in plans} >= {1, 2, 3, 8}, mode
    # the stats-only pass below 17 components: KT = 1
    assert {p['kt_mt'] for _, p in _plans(S.STATS_LOW_K, S.M_ONLY)} == {1}


def test_a_block_with_trailing_waves_that_own_no_rows_occurs():
    lib = _lib()
    for fl in S.FLAVOURS:
        for D, K in ((1, 17), (8, 64)):
            p = S.plan(lib, S.N_SWEEP, D, K, fl, S.FUSED)
            rows = S.wave_rows(p, S.N_SWEEP)
            assert p['blocks'] == 2 and p['nw'] == 8 and sum(rows) == S.N_SWEEP
            assert rows[:8] == [S.TR] * 8 and rows[8:] == [S.TR, 1] + [0] * 6, rows      # nine whole tiles, a one-row tile, six idle waves
    for shapes, mode, flavours in ((S.MASKED, S.E_MASKED, ('gmm',)),):
        assert any(0 in S.wave_rows(p, k[0]) for k, p in _plans(shapes, mode, flavours))


def test_split_and_equal_plans_and_three_tiles_per_wave_occur():
    small = _plans(S.STEP_SHAPES, S.FUSED)
    assert all(p['rpw'] == p['rpw_b'] == S.TR for _, p in small)                        # one tile per wave: an equal plan
    large = _plans(S.SEVERAL, S.FUSED)
    assert {K for (_, _, K, _), _ in large} == {17, 33} and {p['kt_mt'] for _, p in large} == {2, 4}
    for (N, D, K, fl), p in large:
        assert p['rpw'] != p['rpw_b'] and p['nw'] == 8, (N, D, K, fl, p)                 # a split plan
        assert p['rpw'] >= 3 * S.TR and p['rpw_b'] >= 2 * S.TR, (N, D, K, fl, p)         # three whole tiles: a flush with a tile after it
        rows = S.wave_rows(p, N)
        assert sum(rows) == N and any(r % S.TR for r in rows)                           # every row once; ragged tiles among them


def test_the_odd_pack_shape_has_an_odd_pack():
    lib = _lib()
    D = S.ODD_PACK[1]
    assert lib.vmp_mix_pack_words(D) == S.pack_words(D) and S.pack_words(D) % 2 == 1
    assert [D for D in range(1, 9) if S.pack_words(D) % 4 == 0] == [5, 8]               # every other D of the sweep loads its pack word by word
