"""A numpy model of one 64-lane wave under the DPP controls of the reduce-scatter softmax network of the XDL mixture pass
(csrc/vmp_mix.hip: row16_rs4_max / row16_rs4_sum / row16_bcast_bank), against the butterfly it replaces on whole tiles
(row16_max4 / row16_sum4).  Not a test module: tests/test_mix_softmax_net_model.py runs it.

The lane maps are those of the ISA's DPP definitions (a wave of 64 lanes = 4 rows of 16 lanes = 16 banks of 4 lanes):

  row_ror:n          rotate right by n lanes inside the row: lane i of the result takes lane (i - n) mod 16 of the source
  quad_perm:[a,b,c,d] lanes 0..3 of every group of four take lanes a, b, c, d of the same group
  row_newbcast:n     every lane of the row takes lane n of the row
  bank_mask          bit b enables the write of lanes 4 b .. 4 b + 3 of EVERY row; a disabled lane keeps the destination's value

and v_OP_f32_dpp dst, src0, src1 computes dst = OP(dpp(src0), src1).  Arithmetic is numpy's fp32 (IEEE round-to-nearest: the bits
of v_add_f32 / v_max_f32 on finite and infinite operands)."""
import numpy as np

WAVE, ROW, BANK = 64, 16, 4
LANE = np.arange(WAVE)
_ROW0 = LANE & ~(ROW - 1)          # first lane of the lane's row
_I16 = LANE & (ROW - 1)            # position inside the row


def row_ror(src, n):
    assert 1 <= n <= 15
    return src[_ROW0 + ((_I16 - n) % ROW)]


def quad_perm(src, perm):
    assert len(perm) == 4 and all(0 <= p < 4 for p in perm)
    return src[(LANE & ~3) + np.asarray(perm)[LANE & 3]]


def row_newbcast(src, n):
    assert 0 <= n <= 15
    return src[_ROW0 + n]


def dpp_op(op, dst, src0_dpp, src1, bank_mask=0xf):
    """v_OP_f32_dpp dst, src0, src1 <ctrl> row_mask:0xf bank_mask:m with src0 already permuted; dst=None: no earlier value (then
    a lane the mask leaves out holds NaN, so that reading it cannot go unnoticed)"""
    enabled = ((bank_mask >> (_I16 // BANK)) & 1).astype(bool)
    old = np.full(WAVE, np.nan, np.float32) if dst is None else dst
    with np.errstate(invalid='ignore'):
        new = op(src0_dpp.astype(np.float32), src1.astype(np.float32)).astype(np.float32)
    return np.where(enabled, new, old)


def butterfly(op, v):
    """row16_max4 / row16_sum4 on one register: ((v + ror 8) + ror 4) + ror 2) + ror 1, every lane ends with the row's value"""
    s = v.astype(np.float32)
    for n in (8, 4, 2, 1):
        s = dpp_op(op, None, row_ror(s, n), s)
    return s


BANK_OF_REGISTER = (0, 1, 2, 3)    # register v's reduction ends in bank v of every row


def rs4(op, v):
    """row16_rs4_*: v[0..3] (64 lanes each) -> one register; instruction for instruction the sequence of VMP_RS4"""
    a0 = dpp_op(op, None, row_ror(v[0], 8), v[0], 0x3)
    a0 = dpp_op(op, a0, row_ror(v[2], 8), v[2], 0xc)
    a1 = dpp_op(op, None, row_ror(v[1], 8), v[1], 0x3)
    a1 = dpp_op(op, a1, row_ror(v[3], 8), v[3], 0xc)
    b = dpp_op(op, None, row_ror(a0, 12), a0, 0x5)
    b = dpp_op(op, b, row_ror(a1, 4), a1, 0xa)
    b = dpp_op(op, None, quad_perm(b, (2, 3, 0, 1)), b)
    b = dpp_op(op, None, quad_perm(b, (1, 0, 3, 2)), b)
    return b


def bcast_bank(s, v):
    """row16_bcast_bank<v>: the first lane of register v's bank, to the whole row"""
    return row_newbcast(s, 4 * BANK_OF_REGISTER[v])


def softmax_old(lg):
    """the whole-tile softmax of the parent: (max, exp2 argument, sum, r) per register, all-reduce form"""
    mx = [butterfly(np.maximum, lg[v]) for v in range(4)]
    with np.errstate(invalid='ignore'):
        e = [np.exp2((lg[v] - mx[v]).astype(np.float32)).astype(np.float32) for v in range(4)]
    s = [butterfly(np.add, e[v]) for v in range(4)]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        r = [(e[v] * (np.float32(1) / s[v])).astype(np.float32) for v in range(4)]
    return mx, e, s, r


def softmax_new(lg):
    """the same through the reduce-scatter network: ONE reciprocal (of the scattered sums) for the four registers"""
    mxs = rs4(np.maximum, lg)
    mx = [bcast_bank(mxs, v) for v in range(4)]
    with np.errstate(invalid='ignore'):
        e = [np.exp2((lg[v] - mx[v]).astype(np.float32)).astype(np.float32) for v in range(4)]
    ss = rs4(np.add, e)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        inv = (np.float32(1) / ss).astype(np.float32)
    s = [bcast_bank(ss, v) for v in range(4)]
    r = [(e[v] * bcast_bank(inv, v)).astype(np.float32) for v in range(4)]
    return mx, e, s, r, mxs, ss
