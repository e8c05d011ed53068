"""CPU checks of tests/decoder_truth.py: the chunked fp64 truth equals the one-graph truth of test_decoder_gpu.py, the 2-term
emulation with its truncation off equals the truth and with it on differs by what two bf16 terms allow, and the restated tile
ranges of dec_bwd_kernel cover every tile once and put every case of tests/test_decoder_tiles_gpu.py on the branch it is named
for (a later retuning of dec_plan's grid, split or VMP_DEC_BT2_ROWS fails here instead of silently moving a case: the launch
decisions are read from the library through vmp_decoder_launch_plan, not restated)."""
import numpy as np
import pytest
import torch

import decoder_truth as T
import parity_log

SMALL = [  # N, K, S, L, Dy, U
    (13, 3, 7, 8, 8, 50),
    (9, 4, 5, 3, 2, 16),
    (11, 2, 3, 5, 3, 33),
]


def _close(a, b, tol=1e-12):
    return T.relmax(a, b) <= tol


@pytest.mark.parametrize('dims', SMALL)
def test_truth_chunked_equals_the_one_graph_truth_decoder(dims):
    from test_decoder_gpu import truth
    N, K, S, Ld, Dy, U = dims
    x, y, r, w = T.make_inputs(N, K, S, Ld, Dy, U, seed=sum(dims))
    _, _, A_t, g_t = truth(x.astype(np.float64), y.astype(np.float64), r.astype(np.float64), [a.astype(np.float64) for a in w])
    got = T.truth_chunked(x, y, w, r=r, chunk=4 * K * S + 1)                  # 4 data rows per chunk: does not divide N
    assert N % 4 != 0
    assert _close(got['A'], A_t) and _close(got['dx'], g_t[0])
    for a, b in zip(got['grads'], g_t[1:]):
        assert a.shape == b.shape and _close(a, b)


@pytest.mark.parametrize('head', ['natparam', 'standard'])
@pytest.mark.parametrize('dims', [(101, 8, 8, 50), (57, 3, 2, 16), (77, 5, 3, 33)])
def test_truth_chunked_equals_the_one_graph_truth_gradient_input(dims, head):
    from oracle import nets
    R, Din, Dout, U = dims
    x, g1, g2, w = T.make_gin_inputs(R, Din, Dout, U, seed=R + U)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w]
    o1, o2 = nets.mlp(xt, dict(zip(T.NET_VARS, wt)), head)
    gt = torch.autograd.grad((o1 * torch.tensor(g1).double()).sum() + (o2 * torch.tensor(g2).double()).sum(), [xt] + wt)
    got = T.truth_chunked(x, None, w, gmean=g1, gvar=g2, head=head, chunk=16)
    assert R % 16 != 0
    assert _close(got['o1'], o1) and _close(got['o2'], o2) and _close(got['dx'], gt[0])
    for a, b in zip(got['grads'], gt[1:]):
        assert a.shape == b.shape and _close(a, b)


@pytest.mark.parametrize('dims', SMALL)
def test_emulation_without_truncation_is_the_truth(dims):
    N, K, S, Ld, Dy, U = dims
    x, y, r, w = T.make_inputs(N, K, S, Ld, Dy, U, seed=sum(dims))
    want = T.truth_chunked(x, y, w, r=r, chunk=5 * K * S)
    got = T.two_term_emulation(x, y, w, r=r, chunk=3 * K * S, truncate=False)
    assert _close(got['A'], want['A']) and _close(got['dx'], want['dx'])
    for a, b in zip(got['grads'], want['grads']):
        assert _close(a, b)
    for head in ('natparam', 'standard'):
        xg, g1, g2, wg = T.make_gin_inputs(N * K * S, Ld, Dy, U, seed=sum(dims) + 1)
        want = T.truth_chunked(xg, None, wg, gmean=g1, gvar=g2, head=head, chunk=50)
        got = T.two_term_emulation(xg, None, wg, gmean=g1, gvar=g2, head=head, chunk=70, truncate=False)
        for k in ('o1', 'o2', 'dx'):
            assert _close(got[k], want[k]), (head, k)
        for a, b in zip(got['grads'], want['grads']):
            assert _close(a, b), head


@pytest.mark.parametrize('net', [T.SHIPPED_NET] + list(T.EXTRA_NETS))
def test_two_term_dx_error_is_what_two_bf16_terms_allow(net):
    """hi + mid carries 16 significant bits: each operand is off by <= 2^-17 relative, each product by about 2^-16 before the
    sum over units averages it.  The emulation's dx must differ from the truth (the truncation is really on) and stay below
    2^-14 of max |dx|.  Measured here at 2 688 rows (it is what decides whether the 2-term dx bar of test_decoder_tiles_gpu.py
    stays at 1e-5 or becomes 2 x this error): dx U = 50: 8.4e-6, U = 16: 5.2e-6, U = 32: 7.6e-6, U = 33: 1.07e-5, U = 64:
    1.23e-5 (A: 1.1e-6 .. 3.3e-6) - twice these exceeds 1e-5, so the 2-term dx bar is 2 x the emulation's error, which the GPU
    test recomputes on its own inputs; the 2-term A bar stays 1e-5."""
    Ld, Dy, U = net
    N, K, S = 128, 3, 7
    x, y, r, w = T.make_inputs(N, K, S, Ld, Dy, U, seed=U)
    want = T.truth_chunked(x, y, w, r=r)
    got = T.two_term_emulation(x, y, w, r=r)
    e_dx = parity_log.record('rel', T.relmax(got['dx'], want['dx']), what='emulation dx U=%d' % U)
    e_A = parity_log.record('rel', T.relmax(got['A'], want['A']), what='emulation A U=%d' % U)
    print('two-term emulation vs truth, net %s: dx %.3e, A %.3e' % (net, e_dx, e_A))
    assert 0.0 < e_dx < 2.0 ** -14
    assert 0.0 < e_A < 2.0 ** -14


ALL_ROWS = sorted(set([1, 15, 16, 17] + [T.case_rows(n) for n in T.ROW_CASES] + list(T.GIN_ROWS) + [2051 * 28, 2046 * 28]))


@pytest.mark.parametrize('split', [58, 54])
@pytest.mark.parametrize('R', ALL_ROWS)
def test_every_tile_is_owned_by_exactly_one_wave(R, split):
    p = T.bwd_tile_plan(R, split)
    owners = np.zeros(p['ntiles'] + 1, dtype=np.int64)
    for t0, t1 in p['waves']:
        assert 0 <= t0 <= t1 <= p['ntiles']
        owners[t0] += 1
        owners[t1] -= 1
    assert (np.cumsum(owners)[:-1] == 1).all()
    assert len(p['waves']) == p['grid'] * T.BWD_WAVES


def test_plan_thresholds_come_from_the_library():
    """The few-tile grid ends where vmp_decoder_bwd_blocks says it does: the largest row count with four working waves per block
    is found by asking the library, and the two cases that straddle it sit exactly on its two sides."""
    lo, hi = 16, 1 << 20                                    # busy_waves_max(lo) == 4 < busy_waves_max(hi) == 8
    assert T.bwd_tile_plan(lo, 58)['busy_waves_max'] <= 4 and T.bwd_tile_plan(hi, 58)['busy_waves_max'] == 8
    while hi - lo > 16:
        mid = (lo + hi) // 32 * 16
        if T.bwd_tile_plan(mid, 58)['busy_waves_max'] <= 4:
            lo = mid
        else:
            hi = mid
    assert T.case_rows('few_tile_last') == lo and T.case_rows('eight_wave_first') == lo + 16
    assert T.case_rows('bt3_last') < T.DEC_BT2_ROWS <= T.case_rows('bt2_first')
    assert T.case_rows('bt2_first') - T.case_rows('bt3_last') == 3 * 7                       # one data row apart


def test_stated_constants_are_the_librarys():
    """DEC_BT2_ROWS and BWD_WAVES are stated in decoder_truth.py; the library's launch plan must agree: BT flips exactly between
    DEC_BT2_ROWS - 1 and DEC_BT2_ROWS rows in decoder mode and never in gradient-input mode, a backward block is BWD_WAVES waves, and
    the grid the tile plan is built on is the number of partial rows vmp_decoder_bwd_blocks tells the callers to reduce."""
    import vmp_for_svae_amd as V
    lib = V._lib.lib()
    rows = sorted(set(ALL_ROWS + [T.DEC_BT2_ROWS - 1, T.DEC_BT2_ROWS, T.DEC_BT2_ROWS + 1, 2 ** 31 - 1]))
    for net in [T.SHIPPED_NET, (1, 1, 1)] + list(T.EXTRA_NETS):
        for R in rows:
            dec, gin = T.bwd_plan(*net, R), T.bwd_plan(*net, R, gin=True)
            assert dec['BT'] == (2 if R >= T.DEC_BT2_ROWS else 3) and gin['BT'] == 3, (net, R)
            assert dec['threads'] // 64 == gin['threads'] // 64 == T.BWD_WAVES and dec['threads'] % 64 == 0
            assert dec['blocks'] == gin['blocks'] == lib.vmp_decoder_bwd_blocks(R), (net, R)
    assert T.bwd_plan(*T.SHIPPED_NET, T.DEC_BT2_ROWS - 1)['BT'] == 3 and T.bwd_plan(*T.SHIPPED_NET, T.DEC_BT2_ROWS)['BT'] == 2
    for R in rows:
        assert T.bwd_tile_plan(R, 58)['grid'] == lib.vmp_decoder_bwd_blocks(R)


def test_row_cases_sit_on_the_branch_they_are_named_for():
    plan = lambda name, U=50: T.bwd_tile_plan(T.case_rows(name), T.bwd_split(U))
    p = plan('few_tile_last')
    assert (p['ntiles'], p['busy_waves_max'], p['empty_blocks'], p['max_tiles_per_wave'], p['bt']) == (1024, 4, 0, 1, 3)
    assert p['grid'] == T.bwd_tile_plan(1 << 24, 58)['grid']                                 # the full grid
    p = plan('eight_wave_first')
    assert (p['ntiles'], p['busy_waves_max'], p['max_tiles_per_wave'], p['bt']) == (1025, 8, 1, 3)
    p = plan('two_tile_first')
    assert (p['ntiles'], p['tpb'], p['busy_blocks'], p['empty_blocks']) == (2049, 9, 228, 28)
    assert p['max_tiles_per_wave'] == 2 and p['ragged'] and not p['split_branch'] and p['bt'] == 3
    first = p['waves'][:T.BWD_WAVES]
    # tpb = 9 -> tpp = 3: three SIMD pairs take 3 tiles each (older wave 2: the prefetch is carried; younger 1), the fourth none
    assert [t1 - t0 for t0, t1 in first] == [2, 2, 2, 0, 1, 1, 1, 0]
    assert T.bwd_tile_plan(2048 * 16, 58)['max_tiles_per_wave'] == 1                         # one tile fewer: none does
    p = plan('even_split_last')
    assert (p['ntiles'], p['tpp'], p['split_branch'], p['uneven'], p['ragged'], p['bt']) == (7168, 7, False, False, False, 3)
    p = plan('uneven_split_first')
    assert (p['ntiles'], p['tpb'], p['tpp'], p['older']) == (7170, 29, 8, 5)
    assert p['split_branch'] and p['uneven'] and p['ragged'] and p['busy_blocks'] == 248 and p['last_short'] and p['bt'] == 3
    assert p['empty_blocks'] == 8
    # U = 64 takes the same branch with split = 54, which at tpp = 8 rounds to equal shares: the arithmetic runs, the shares are 4 / 4
    p = plan('uneven_split_first', 64)
    assert p['split_branch'] and p['older'] == 4
    p = plan('bt3_last')
    assert p['bt'] == 3 and p['ragged'] and p['uneven'] and p['ntiles'] == 32768
    p = plan('bt2_first')
    assert p['bt'] == 2 and p['ragged'] and p['uneven'] and p['ntiles'] == 32770 and p['ntiles'] > 4 * 4096   # forward: grid-stride past 4 096 blocks
    for R in T.GIN_ROWS:
        assert R in [T.case_rows(n) for n in T.ROW_CASES]


def test_network_cases_pick_the_instantiation_they_are_named_for():
    R = T.case_rows('bt2_first')
    assert T.bwd_variant(8, 8, 50, R) == (4, True, 2, True)
    assert T.bwd_variant(3, 2, 16, R) == (1, False, 2, True)
    assert T.bwd_variant(6, 6, 32, R) == (2, False, 2, True)
    assert T.bwd_variant(5, 3, 33, R) == (3, True, 2, True)
    assert T.bwd_variant(8, 8, 64, R) == (4, False, 2, False)                                # two slab rounds
    assert T.bwd_variant(1, 1, 1, T.case_rows('two_tile_first')) == (1, True, 3, True)
    assert T.bwd_variant(8, 8, 50, T.case_rows('bt3_last'))[2] == 3
    for R, net in T.GIN_CASES:                                                               # gradient-input mode: 3-term at every size
        assert T.bwd_variant(*net, R, gin=True)[2] == 3
    assert T.bwd_variant(8, 8, 64, R, gin=True) == (4, False, 3, False)
    assert T.bwd_split(64) == 54 and T.bwd_split(50) == 58
    # every GPU case is one of the proven row counts at one of the proven networks
    for name, net in T.DECODER_CASES:
        assert name in T.ROW_CASES and (net in (T.SHIPPED_NET, (1, 1, 1)) or net in T.EXTRA_NETS)
    assert len(T.DECODER_CASES) == 7 + 3 * 4 + 1 and len(T.GIN_CASES) == 9


def test_inputs_of_a_row_do_not_depend_on_the_row_count():
    a = T.make_inputs(5, 3, 7, 8, 8, 50, seed=3)
    b = T.make_inputs(6, 3, 7, 8, 8, 50, seed=3)
    for u, v in zip(a[:3], b[:3]):
        assert u.dtype == np.float32 and np.array_equal(u, v[:5])
    for u, v in zip(a[3], b[3]):
        assert np.array_equal(u, v)
    g, h = T.make_gin_inputs(40, 6, 6, 32, seed=1), T.make_gin_inputs(61, 6, 6, 32, seed=1)
    for u, v in zip(g[:3], h[:3]):
        assert np.array_equal(u, v[:40])
