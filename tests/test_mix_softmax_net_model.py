"""The reduce-scatter softmax network of the XDL mixture pass (csrc/vmp_mix.hip: VMP_RS4, row16_bcast_bank) on the host model of
tests/mix_softmax_net_model.py: the bank <-> register map, the rotation directions and the addition tree are fixed here, before any
launch.  For every kind of input: each lane of bank v ends with the maximum / the sum of register v over the row's 16 lanes, the sum
has the fp32 BITS of the butterfly's ((v + ror 8) + ror 4) + ror 2) + ror 1, and each broadcast hands register v its own row's value
in all 16 lanes of all four rows.  No GPU."""
import numpy as np
import pytest

import mix_softmax_net_model as M


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _inputs(kind, seed):
    """four registers x 64 lanes of log2 rho: lane = (row of the wave, component i16)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lg = (rng.standard_normal((4, M.WAVE)) * 10).astype(np.float32)
    if kind == 'dominant':                 # one component per (register, row) far above the others: different ones everywhere
        lg -= np.float32(150)
        for v in range(4):
            for row in range(4):
                lg[v, 16 * row + (5 * v + 3 * row + seed) % 16] = np.float32(rng.standard_normal())
    elif kind == 'inf':                    # components that are out (-inf), never a whole row
        out = rng.random((4, M.WAVE)) < 0.5
        for v in range(4):
            for row in range(4):
                out[v, 16 * row + (v + 7 * row + seed) % 16] = False
        lg[out] = -np.inf
    elif kind == 'one_left':               # fifteen of sixteen are out
        keep = np.zeros((4, M.WAVE), bool)
        for v in range(4):
            for row in range(4):
                keep[v, 16 * row + (11 * v + row + seed) % 16] = True
        lg[~keep] = -np.inf
    else:
        assert kind == 'random'
    return lg


def test_lane_maps_are_the_isa_definitions():
    lane = M.LANE.astype(np.float32)
    ror1, ror12 = M.row_ror(lane, 1), M.row_ror(lane, 12)
    assert ror1[1] == 0 and ror1[0] == 15 and ror1[32] == 47 and ror1[63] == 62           # lane i takes lane i - 1 of its row
    assert ror12[0] == 4 and ror12[3] == 7 and ror12[12] == 0 and ror12[16 + 8] == 16 + 12   # by 12 = by -4: takes lane i + 4
    assert list(M.quad_perm(lane, (2, 3, 0, 1))[:8]) == [2, 3, 0, 1, 6, 7, 4, 5]
    assert list(M.quad_perm(lane, (1, 0, 3, 2))[60:]) == [61, 60, 63, 62]
    assert np.array_equal(M.row_newbcast(lane, 8), 16 * (M.LANE // 16) + 8)
    d = M.dpp_op(np.add, np.zeros(64, np.float32), lane + 1, lane + 1, 0x5)                  # banks 0 and 2 of every row
    assert np.array_equal(d != 0, ((M.LANE % 16) // 4) % 2 == 0) and d[0] == 2 and d[4] == 0 and d[8] == 18 and d[12] == 0


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('kind', ['random', 'dominant', 'inf', 'one_left'])
def test_network_is_the_butterfly(kind, seed):
    lg = _inputs(kind, seed)
    mx0, e0, s0, r0 = M.softmax_old(lg)
    mx1, e1, s1, r1, mxs, ss = M.softmax_new(lg)
    bank = (M.LANE % 16) // 4
    for v in range(4):
        in_bank = bank == M.BANK_OF_REGISTER[v]
        rows = lg[v].reshape(4, 16)
        # every lane of bank v: the row's maximum and the butterfly's sum
        assert np.array_equal(mxs[in_bank].reshape(4, 4), np.repeat(rows.max(1)[:, None], 4, 1)), (kind, v)
        assert _same_bits(mxs[in_bank], mx0[v][in_bank]), (kind, v)
        assert _same_bits(ss[in_bank], s0[v][in_bank]), (kind, v)
        want = e0[v].astype(np.float64).reshape(4, 16).sum(1)
        assert np.all(np.abs(ss[in_bank].reshape(4, 4) - want[:, None]) <= 16 * 2.0 ** -24 * want[:, None]), (kind, v)
        # the broadcasts: register v gets its own row's value in all 64 lanes
        assert _same_bits(mx1[v], mx0[v]) and _same_bits(s1[v], s0[v]), (kind, v)
        assert _same_bits(e1[v], e0[v]) and _same_bits(r1[v], r0[v]), (kind, v)
        assert np.isfinite(r1[v]).all() and np.all(s1[v] >= 1), (kind, v)
    assert np.isfinite(mxs).all() and np.isfinite(ss).all()             # no lane of the result was left unwritten (NaN marks it)


@pytest.mark.parametrize('scale', [2.0 ** -140, 2.0 ** -149, 2.0 ** -127])
def test_denormal_sums_keep_the_butterflys_bits(scale):
    """the addition network alone on registers whose row sums are denormal (or cross into the normal range)"""
    rng = np.random.Generator(np.random.PCG64(7))
    v = (rng.integers(0, 200, (4, M.WAVE)).astype(np.float64) * scale).astype(np.float32)
    assert (v[v != 0] < np.finfo(np.float32).tiny * 256).all() and (v != 0).any()
    ss = M.rs4(np.add, v)
    bank = (M.LANE % 16) // 4
    for r in range(4):
        full = M.butterfly(np.add, v[r])
        assert _same_bits(M.bcast_bank(ss, r), full)
        assert _same_bits(ss[bank == M.BANK_OF_REGISTER[r]], full[bank == M.BANK_OF_REGISTER[r]])
        assert np.array_equal(full.reshape(4, 16)[:, 0].astype(np.float64), v[r].astype(np.float64).reshape(4, 16).sum(1))   # exact: multiples of one quantum


def test_a_wrong_rotation_is_caught():
    """the model tells the two directions apart: with rotations 4 and 12 of step 2 swapped, a bank sums two different rows"""
    lg = _inputs('random', 3)
    a0 = M.dpp_op(np.add, None, M.row_ror(lg[0], 8), lg[0], 0x3)
    a0 = M.dpp_op(np.add, a0, M.row_ror(lg[2], 8), lg[2], 0xc)
    wrong = M.dpp_op(np.add, None, M.row_ror(a0, 4), a0, 0x5)
    right = M.dpp_op(np.add, None, M.row_ror(a0, 12), a0, 0x5)
    s1 = M.dpp_op(np.add, None, M.row_ror(lg[0], 8), lg[0])
    s2 = M.dpp_op(np.add, None, M.row_ror(s1, 4), s1)
    assert _same_bits(right[:4], s2[:4]) and not _same_bits(wrong[:4], s2[:4])
