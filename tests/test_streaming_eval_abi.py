"""CPU-side checks of the streaming test-time evaluation (include/vmp_hip.h: vmp_decoder_eval_fwd, vmp_svae_philox_noise_at,
vmp_svae_estep_fwd_rng_at; losses.plan_eval_chunks / streaming_metrics): prototypes, host-side argument checks (every call below
fails before any launch), the new kernels' register files, and the chunk planner."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('vmp_decoder_eval_fwd', 'vmp_svae_philox_noise_at', 'vmp_svae_estep_fwd_rng_at')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def _prototypes():
    txt = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w\s]*?[\s\*]+)(vmp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', txt):
        out[name] = (ret.strip(), [a.strip() for a in args.split(',')])
    return out


def _kind(decl):
    if '*' in decl:
        return ('ptr', 8)
    w = [x for x in decl.split() if x != 'const']
    return {'int': ('int', 4), 'int64_t': ('int', 8), 'uint64_t': ('uint', 8), 'size_t': ('uint', 8), 'float': ('float', 4)}[w[0]]


def _ckind(t):
    if t is ctypes.c_void_p:
        return ('ptr', 8)
    code = t._type_
    return ('float' if code in 'fd' else 'int' if code.islower() else 'uint', ctypes.sizeof(t))


def test_ctypes_table_matches_the_new_prototypes():
    import vmp_for_svae_amd as V
    protos = _prototypes()
    lib = ctypes.CDLL(V._lib.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(lib, name), 'libvmp_hip.so does not export %s' % name
        res, argtypes = V._lib._SIGNATURES[name]
        ret, args = protos[name]
        assert _ckind(res) == _kind(ret)
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for i, (d, t) in enumerate(zip(args, argtypes)):
            assert _ckind(t) == _kind(d), (name, i, d, t)
    assert len(protos['vmp_decoder_eval_fwd'][1]) == 25
    assert lib.vmp_abi_version() == 1                               # exports are only added


def test_decoder_eval_fwd_validates_on_the_host():
    """x, y, the nine parameters and the workspace are required; mask, logw, the stream and ONE of (mse, lse) are optional."""
    lib = _lib()
    P = ctypes.c_void_p(64)
    #       x  y  9 params      mask ms logw  N   K   S   L  Dy  U  mse lse ws  bytes    stream
    args = [P, P] + [P] * 9 + [P, 1, P, 64, 16, 10, 8, 8, 50, P, P, P, 1 << 30, None]
    required = list(range(0, 11)) + [22]
    for i in required:
        rc = lib.vmp_decoder_eval_fwd(*[None if j == i else a for j, a in enumerate(args)])
        assert rc == -1 and b'NULL' in lib.vmp_last_error(), i
    both = [None if j in (20, 21) else a for j, a in enumerate(args)]
    assert lib.vmp_decoder_eval_fwd(*both) == -1 and b'NULL' in lib.vmp_last_error()        # neither output
    # the optional ones NULL: past the pointer checks, refused by the workspace check behind them - nothing is launched
    for opt in ((11,), (13,), (20,), (21,), (11, 13, 20)):
        rest = [None if j in opt else (16 if j == 23 else a) for j, a in enumerate(args)]
        assert lib.vmp_decoder_eval_fwd(*rest) not in (0, -1) and b'workspace' in lib.vmp_last_error(), opt
    # the fused decoder's compiled range: L, Dy <= 8, U <= 64
    for j, v in ((17, 9), (18, 9), (19, 65), (15, 0), (16, 0)):
        bad = [v if i == j else a for i, a in enumerate(args)]
        assert lib.vmp_decoder_eval_fwd(*bad) not in (0, -1) and b'unsupported' in lib.vmp_last_error(), (j, v)
    rows = [2 ** 22 if i == 14 else a for i, a in enumerate(args)]                            # 2^22 * 64 * 10 >= 2^31 sample rows
    rows[15] = 64
    assert lib.vmp_decoder_eval_fwd(*rows) != 0 and b'2^31' in lib.vmp_last_error()
    misaligned = [ctypes.c_void_p(68) if i == 22 else a for i, a in enumerate(args)]
    assert lib.vmp_decoder_eval_fwd(*misaligned) != 0 and b'workspace' in lib.vmp_last_error()


def test_row_offset_forms_validate_on_the_host():
    lib = _lib()
    P = ctypes.c_void_p(64)
    assert lib.vmp_svae_philox_noise_at(1, 0, 64, 16, 8, 10, None, None) == -1 and b'null' in lib.vmp_last_error()
    assert lib.vmp_svae_philox_noise_at(1, -1, 64, 16, 8, 10, P, None) == -1 and b'row0' in lib.vmp_last_error()
    assert lib.vmp_svae_philox_noise_at(1, 5, 64, 16, 9, 10, P, None) != 0                    # L = 9
    #       eta1 eta2d hk Pk bias seed row0 mk Wk kappa nu  N   K  L  S   x  lz Tp ws  stream
    args = [P, P, P, P, P, 7, 128, P, P, P, P, 64, 16, 8, 10, P, P, P, P, None]
    for i in (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17):
        rc = lib.vmp_svae_estep_fwd_rng_at(*[None if j == i else a for j, a in enumerate(args)])
        assert rc == -1 and b'null' in lib.vmp_last_error(), i
    neg = [-3 if j == 6 else a for j, a in enumerate(args)]
    assert lib.vmp_svae_estep_fwd_rng_at(*neg) == -1 and b'row0' in lib.vmp_last_error()
    # nu, noise_ws (an in-kernel shape) and the stream are optional: with them NULL and a size out of range, the call gets past the
    # pointer checks and fails on the size check (K = 65) - nothing is launched
    rest = [None if j in (10, 18, 19) else (65 if j == 12 else a) for j, a in enumerate(args)]
    assert lib.vmp_svae_estep_fwd_rng_at(*rest) not in (0, -1)
    # a shape outside the in-kernel generator needs the noise workspace
    assert lib.vmp_svae_rng_in_kernel(10, 3, 7) == 0
    nows = [None if j == 18 else a for j, a in enumerate(args)]
    nows[12], nows[13], nows[14] = 10, 3, 7
    assert lib.vmp_svae_estep_fwd_rng_at(*nows) != 0 and b'noise workspace' in lib.vmp_last_error()


def _kernel_notes(pattern):
    """{kernel symbol: (private segment bytes, VGPRs)} of the shipped library's kernels whose symbol matches `pattern`"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    readelf = E.OBJDUMP.replace('llvm-objdump', 'llvm-readelf')
    if not os.path.exists(readelf):
        pytest.skip('llvm-readelf not available')
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)', txt, re.S):
            if re.search(pattern, m.group(1)):
                seen[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return seen


def test_evaluation_kernels_use_no_scratch():
    """dec_eval_kernel<U tile> (all four), dec_eval_reduce_kernel and the kernels that gained the row offset: private segment 0.
    Same block size and LDS image as dec_fwd_kernel<U tile>, and at every width no more VGPRs (8 per allocation granule): the
    occupancy is no lower than the forward kernel's."""
    ev = _kernel_notes(r'dec_eval_kernel')
    assert len(ev) == 4, sorted(ev)
    assert all(v[0] == 0 for v in ev.values()), ev
    red = _kernel_notes(r'dec_eval_reduce_kernel')
    assert len(red) == 1 and all(v[0] == 0 for v in red.values()), red
    fwd = _kernel_notes(r'dec_fwd_kernel')
    gran = lambda v: (v + 7) // 8
    for ut in (1, 2, 3, 4):
        e_ = [v for k, v in ev.items() if 'ILi%dE' % ut in k]
        f_ = [v for k, v in fwd.items() if 'ILi%dE' % ut in k]
        assert len(e_) == 1 and len(f_) == 1 and gran(e_[0][1]) <= gran(f_[0][1]), (ut, e_, f_)
    rng = _kernel_notes(r'svae_estep_fwd4_kernelILi\dELi(0|10)ELb1E|philox_noise_kernel')
    assert len(rng) >= 17 and all(v[0] == 0 for v in rng.values()), rng


@pytest.mark.parametrize('in_kernel', [True, False])
def test_plan_eval_chunks_honours_the_budget(in_kernel):
    """Every chunk-sized buffer of the chunk loop is counted: x (K,S,L), the noise workspace when the generator is not in-kernel, the
    per-row pair (K,S,2), the encoder outputs (2 L) and the K-sized cell values."""
    from vmp_for_svae_amd import losses
    for N in (1, 17, 300, 10 ** 6):
        for K, S, Ld, Dy in ((16, 100, 8, 8), (10, 100, 6, 7), (16, 10, 8, 8), (5, 7, 2, 3), (64, 100, 8, 8), (1, 1, 1, 1)):
            floor = 4 * (K * S * Ld * (1 if in_kernel else 2) + 2 * K * S + 2 * Ld)        # x (+ noise) + pairs + encoder outputs
            for budget in (floor, 1 << 20, 7 << 20, 256 << 20):
                budget = max(budget, floor + 24 * K)                                       # at least one row (+ its six K-sized cell values)
                rows = losses.plan_eval_chunks(N, K, S, Ld, Dy, budget, in_kernel=in_kernel)
                assert 1 <= rows <= N
                assert rows * floor <= budget, (N, K, S, Ld, Dy, budget, rows)
                assert rows * K * S < 2 ** 31
                if rows < N and (rows + 1) * K * S < 2 ** 31:                               # and not needlessly small
                    assert (rows + 1) * (floor + 24 * K) > budget                        # + the six K-sized cell values
    # the not-in-kernel case costs a second x-sized buffer
    a = losses.plan_eval_chunks(10 ** 6, 10, 7, 3, 7, 1 << 20, in_kernel=True)
    b = losses.plan_eval_chunks(10 ** 6, 10, 7, 3, 7, 1 << 20, in_kernel=False)
    assert b < a and b >= a // 2 - 1


def test_plan_eval_chunks_asks_the_library_about_the_noise():
    from vmp_for_svae_amd import losses
    lib = _lib()
    assert lib.vmp_svae_rng_in_kernel(16, 8, 100) == 1 and lib.vmp_svae_rng_in_kernel(10, 3, 7) == 0
    assert losses.plan_eval_chunks(10 ** 6, 16, 100, 8, 8, 64 << 20) == losses.plan_eval_chunks(10 ** 6, 16, 100, 8, 8, 64 << 20, in_kernel=True)
    assert losses.plan_eval_chunks(10 ** 6, 10, 7, 3, 7, 1 << 20) == losses.plan_eval_chunks(10 ** 6, 10, 7, 3, 7, 1 << 20, in_kernel=False)
    # the default budget: a chunk's x stays below the 256 MB last-level cache
    rows = losses.plan_eval_chunks(10 ** 6, 16, 100, 8, 8)
    assert rows * 16 * 100 * 8 * 4 < 256 << 20 and rows > 3000


def test_plan_eval_chunks_counts_the_torch_mlp_of_an_unfused_decoder():
    """fused=False: per sample row the hidden activations of the torch MLP (both layers, one more of the widest) and six head-sized
    tensors are counted instead of the per-row pair; an encoder outside the fused range likewise (per data row)."""
    from vmp_for_svae_amd import losses
    K, S, Ld, Dy, U = 16, 100, 8, 8, 100
    fused = losses._eval_row_bytes(K, S, Ld, Dy, True, True)
    unf = losses._eval_row_bytes(K, S, Ld, Dy, True, False, hidden=(U, U))
    assert unf - fused == 4 * K * S * (3 * U + 6 * Dy - 2)
    assert losses._eval_row_bytes(K, S, Ld, Dy, True, True, enc_hidden=(U, U)) - fused == 4 * (3 * U + 6 * Ld - 2 * Ld)
    for budget in (unf, 10 * unf + 5, 256 << 20):
        rows = losses.plan_eval_chunks(10 ** 6, K, S, Ld, Dy, budget, in_kernel=True, fused=False, hidden=(U, U))
        assert rows * unf <= budget < (rows + 1) * unf
    assert losses.plan_eval_chunks(10 ** 6, K, S, Ld, Dy, 256 << 20, in_kernel=True, fused=False, hidden=(U, U)) < \
        losses.plan_eval_chunks(10 ** 6, K, S, Ld, Dy, 256 << 20, in_kernel=True) // 20


def test_plan_eval_chunks_raises_below_one_row():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd import losses
    with pytest.raises(V._lib.VmpError, match='one evaluation row'):
        losses.plan_eval_chunks(1000, 16, 100, 8, 8, 16 * 100 * 8 * 4, in_kernel=True)          # x alone fills it
    with pytest.raises(V._lib.VmpError):
        losses.plan_eval_chunks(1000, 16, 100, 8, 8, 0, in_kernel=True)
    with pytest.raises(V._lib.VmpError):
        losses.plan_eval_chunks(0, 16, 100, 8, 8, 1 << 20, in_kernel=True)


def test_bernoulli_head_raises():
    from vmp_for_svae_amd import losses
    y = torch.zeros(4, 8)
    enc = [(50, torch.tanh), (50, torch.tanh), (8, 'natparam')]
    dec = [(50, torch.tanh), (50, torch.tanh), (8, 'bernoulli')]
    with pytest.raises(NotImplementedError, match='bernoulli'):
        losses.streaming_metrics(y, None, enc, dec, 10)
    with pytest.raises(NotImplementedError, match='bernoulli'):
        losses.streaming_imputation_losses(y, torch.zeros(4, 8, dtype=torch.bool), None, enc, dec, 2, 3)


def test_philox_noise_row_offset_argument_rules():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _svae_ops
    n = _svae_ops.PhiloxNoise(3, 10)
    assert n.row0 == 0 and not n.at
    assert _svae_ops.PhiloxNoise(3, 10, row0=128).at and _svae_ops.PhiloxNoise(3, 10, at=True).at
    with pytest.raises(V._lib.VmpError):
        _svae_ops.PhiloxNoise(3, 10, row0=-1)
    with pytest.raises(V._lib.VmpError):
        _svae_ops.PhiloxNoise(3, 10, row0=5, epilogue=True)
