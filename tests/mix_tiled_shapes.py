"""Shape tables of the tiled mixture pass (csrc/vmp_mix.hip: pass_kernel<D, KT, FLAV, ESTEP, STATS, MASK>), stated once for
tests/test_mix_tiled_cover.py (pure host: asks vmp_mix_pass_plan where every entry lands and fails when a branch is no longer reached)
and tests/test_mix_tiled_pass_gpu.py (runs every entry against the fp64 oracle).  Not a test module.

pass_plan sends a pass to the tiled form whenever it is not an E-step launch with K <= 16 and no mask: every K > 16 (KT = 2 up to 32
components, 4 above), the stats-only M-pass at any K, the masked E-pass of the GMM.  What the tables have to reach, and why each size
is what it is:

  N = 577       ten tiles of 64 rows - nine whole ones and one of a single row - dealt to two blocks of eight waves: the second block
                has two waves with rows and six that own nothing; nw == 8, the serial block reduction wherever KT (FT + 1) 2048 nw bytes
                exceed 64 KiB (KT = 2 with D >= 5, KT = 4 always), the parallel one at KT = 2 with D <= 4.
  N = 1, 100    one and two tiles = blocks of one and two waves: the parallel reduction (its w < nw guard with nw < NWB) at every
                (D, KT), KT = 4 and D >= 5 included.
  N = 130       three waves: the parallel reduction at KT = 2 for every D and at KT = 4 for D <= 4, the serial one with nw < 8 at
                KT = 4, D >= 5.
  N = 400 037   (the size tests/test_mix_pass_pipeline_gpu.py uses for the XDL form) the plan is split (rpw != rpw_b: 248 / 144 rows
                for the GMM, 240 / 152 for the SMM) and the older waves get rpw >= 192 rows = three whole tiles, i.e. a fp32 -> fp64
                flush (every VMP_MOM_FLUSH = 2nd tile) with another tile after it; the shares are no multiples of 64: ragged tiles.
"""
import ctypes
import itertools

GMM, SMM = 0, 1                    # VMP_GMM, VMP_SMM (include/vmp_hip.h)
TILED, XDL = 1, 2                  # PassPlan::form
TR = 64                            # rows of a wave tile
FLAVOURS = ('gmm', 'smm')

N_SWEEP = 577
KS_TILED = (17, 32, 33, 48, 49, 64)            # KT = 2: 17 (one live lane in the 2nd tile), 32 (exact); KT = 4: 33 and 48 (4th tile
#                                                wholly off), 49 (one live lane in it), 64 (exact: the predicate-free FULL bodies)
SWEEP = [(N_SWEEP, D, K) for D in range(1, 9) for K in KS_TILED]
# blocks of fewer than eight waves (see the module docstring); every (N, D, K) here has K > 16
SMALL = [(1, 2, 17), (1, 5, 33), (1, 8, 64),
         (100, 5, 17), (100, 8, 32), (100, 4, 48), (100, 6, 49), (100, 7, 64), (100, 8, 64),
         (130, 5, 32), (130, 8, 17), (130, 2, 33), (130, 3, 64), (130, 7, 48), (130, 6, 64)]
# the stats-only M-pass is tiled (KT = 1) below 17 components too
STATS_LOW_K = [(N_SWEEP, D, K) for D in (1, 4, 5, 8) for K in (1, 7, 16)]
N_SEVERAL = 400000 + 37
SEVERAL = [(N_SEVERAL, D, K) for K in (17, 33) for D in (3, 8)]
MASKED = [(N, D, K) for N in (63, N_SWEEP) for D in (1, 3, 5, 8) for K in (5, 16, 17, 40, 64)]
MASK_KINDS = ('none', 'random', 'empty_rows', 'byte255')
# a view of x one float into its buffer; the last two take the XDL kernel in their E-step launches
UNALIGNED = [(N_SWEEP, 5, 17), (N_SWEEP, 8, 64), (1024 + 17, 8, 16), (1024 + 17, 3, 10)]
ODD_PACK = (N_SWEEP, 7, 33)        # Geo<7>::PACK = 7 + 28 + 4 = 39 words: the scalar parameter load (PACK % 4 != 0)

STEP_SHAPES = SWEEP + SMALL                    # one fused step + finalize; the E-only pass
STATS_SHAPES = SWEEP + SMALL + STATS_LOW_K     # the stats-only pass

PLAN_FIELDS = ('form', 'kt_mt', 'nw', 'blocks', 'rpw', 'rpw_b', 'par_reduce', 'lds')
FUSED, E_ONLY, M_ONLY, E_MASKED = (1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 0, 1)        # (estep, stats, mask)


def kt_of(K):
    """the 16-component tiles a lane of the tiled form carries"""
    t = (K + 15) // 16
    return t if t <= 2 else 4


def pack_words(D):
    return D + D * (D + 1) // 2 + 4


def plan(lib, N, D, K, flavour, mode):
    """vmp_mix_pass_plan's answer as a dict (pure host: no launch, no device)"""
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    rc = lib.vmp_mix_pass_plan(N, D, K, SMM if flavour in (SMM, 'smm') else GMM, mode[0], mode[1], mode[2], out)
    assert rc == 0, (N, D, K, flavour, mode, rc)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def wave_rows(p, N):
    """rows owned by every wave of the grid, as pass_kernel derives them from (rpw, rpw_b)"""
    rows = []
    for b, w in itertools.product(range(p['blocks']), range(p['nw'])):
        if p['rpw_b'] == p['rpw']:
            lo = (b * p['nw'] + w) * p['rpw']
            hi = lo + p['rpw']
        else:
            hw = p['nw'] // 2
            base = b * hw * (p['rpw'] + p['rpw_b'])
            lo = base + w * p['rpw'] if w < hw else base + hw * p['rpw'] + (w - hw) * p['rpw_b']
            hi = lo + (p['rpw'] if w < hw else p['rpw_b'])
        rows.append(max(0, min(hi, N) - min(lo, N)))
    return rows
