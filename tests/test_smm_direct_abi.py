"""CPU-side checks of the SMM-SVAE's minibatch step entry points (include/vmp_hip.h, "The same six-launch minibatch step for the
Student-t mixture SVAE"): argument checks and the coverage query are host logic - every call below fails before any launch - and the
Student-t instances of the minibatch backward kernel fit their registers."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_student_t_coverage_query_envelope():
    """The Gaussian form's envelope: <= 256 tiles of 64 / K rows, S <= 16 (K = 64: one row per tile), and nothing outside it."""
    q = _lib().vmp_svae_bwd_tail_applies_t
    assert q(64, 16, 8, 10) == 1                                   # C5 minibatch
    assert q(256 * 4, 16, 8, 10) == 1 and q(256 * 4 + 1, 16, 8, 10) == 0     # 256 / 257 tiles at K = 16
    assert q(256, 64, 8, 10) == 1 and q(257, 64, 8, 10) == 0       # K = 64: one row per tile
    assert q(64, 10, 8, 16) == 1 and q(64, 10, 8, 17) == 0         # S = 16 / 17
    assert q(512, 8, 6, 10) == 1 and q(1, 1, 1, 4) == 1
    assert q(0, 16, 8, 10) == 0 and q(64, 65, 8, 10) == 0 and q(64, 16, 9, 10) == 0 and q(64, 16, 8, 0) == 0
    for args in ((64, 16, 8, 10), (1024, 16, 8, 16), (64, 10, 8, 17)):   # the Gaussian query answers alike
        assert q(*args) == _lib().vmp_svae_bwd_tail_applies(*args)


def test_smm_step_entry_points_validate_on_the_host():
    lib = _lib()
    P = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 9)(*[64] * 9)
    # launch 1
    rc = lib.vmp_mlp_gauss_head_fwd_prep_smm(*([P] * 10), 64, 8, 8, 50, -0.5, P, P, *([P] * 6), 16, *([P] * 6), P, 0, None, None, None)
    assert rc != 0 and b'scalar table' in lib.vmp_last_error()                 # a table without rows
    rc = lib.vmp_mlp_gauss_head_fwd_prep_smm(*([P] * 10), 64, 8, 8, 50, -0.5, P, P, P, P, P, P, None, P, 16, *([P] * 6), None, 0, None,
                                             None, None)
    assert rc != 0 and b'NULL' in lib.vmp_last_error()                         # theta/L_k missing
    rc = lib.vmp_mlp_gauss_head_fwd_prep_smm(*([P] * 10), 64, 8, 8, 50, -0.5, P, P, P, P, P, P, P, None, 16, *([P] * 6), None, 0, None,
                                             None, None)
    assert rc != 0 and b'NULL' in lib.vmp_last_error()                         # DoF missing
    rc = lib.vmp_mlp_gauss_head_fwd_prep_smm(*([P] * 10), 64, 8, 9, 50, -0.5, P, P, *([P] * 6), 16, *([P] * 6), None, 0, None, None, None)
    assert rc != 0                                                              # latent size 9
    rc = lib.vmp_mlp_gauss_head_fwd_prep_smm(*([P] * 10), 64, 8, 8, 50, -0.5, P, P, *([P] * 6), 65, *([P] * 6), None, 0, None, None, None)
    assert rc != 0                                                              # K = 65
    # launch 4
    bwd = lambda nu, N, K, S, sigma=-1.0, pbytes=1 << 30: lib.vmp_svae_estep_bwd_tail_t(*([P] * 7), nu, *([P] * 4), sigma, P, N, K, 8, S, P, P,
                                                                                      P, pbytes, P, P, 1 << 20, None)
    assert bwd(None, 64, 16, 10) != 0 and b'null' in lib.vmp_last_error()        # nu is required
    assert bwd(P, 64, 16, 10, sigma=0.0) != 0 and b'sigma' in lib.vmp_last_error()
    assert bwd(P, 10**6, 16, 10) != 0 and b'minibatch form' in lib.vmp_last_error()
    assert bwd(P, 64, 10, 18) != 0 and b'minibatch form' in lib.vmp_last_error()
    assert bwd(P, 64, 16, 10, pbytes=16) != 0 and b'too small' in lib.vmp_last_error()
    assert bwd(P, 0, 16, 10) != 0
    # launch 6
    fin = lambda N, nblk, th=arr, alpha=P: lib.vmp_svae_step_final_smm(P, 100, 8, 50, 8, arr, arr, arr, arr, P, 1, 8, 50, 8, arr, arr, arr, arr,
                                                                       P, nblk, P, arr, arr, arr, arr, th, th, th, th, P, N, P, alpha, None,
                                                                       None, 0.2, 16, 8, P, P, 16, 8, P, 0.9, 0.999, 1e-8, 1e-3, None, None)
    assert fin(513, 16) != 0 and b'range' in lib.vmp_last_error()               # N > 512
    assert fin(64, 0) != 0                                                      # no partial rows
    assert fin(64, 16, th=None) != 0 and b'NULL' in lib.vmp_last_error()        # theta tensors missing
    assert fin(64, 16, alpha=None) != 0 and b'NULL' in lib.vmp_last_error()     # alpha missing
    pack = lambda n, xbuf=P: lib.vmp_svae_step_pack_smm(xbuf, n, P, 100, 8, 50, 8, arr, arr, P, 1, 8, 50, 8, arr, arr, P, 16, P, arr, arr, arr,
                                                        arr, P, 64, 16, 8, P, 16, 8, P, None)
    assert pack(10) != 0 and b'too small' in lib.vmp_last_error()
    assert pack(1 << 20, xbuf=None) != 0 and b'NULL' in lib.vmp_last_error()
    # The closing launch checks its pointers by form: each one that vmp_svae_step_final_smm / _pack_smm reads is refused when NULL
    # (VMP_E_BADARG = -1); with every one that it does NOT read NULL (alpha_star, the device words of the step sizes, the stream) the
    # call gets past the pointer checks and fails on the size check behind them (N = 513: VMP_E_DIM = -2) - nothing is launched either way.
    nul = (ctypes.c_void_p * 9)(*([0] + [64] * 8))                              # an array whose first tensor is NULL
    final = [P, 100, 8, 50, 8, arr, arr, arr, arr, P, 1, 8, 50, 8, arr, arr, arr, arr, P, 16, P, arr, arr, arr, arr, arr, arr, arr, arr, P, 64, P, P, P,
             P, 0.2, 16, 8, P, P, 16, 8, P, 0.9, 0.999, 1e-8, 1e-3, P, None]
    packed = [P, 1 << 20, P, 100, 8, 50, 8, arr, arr, P, 1, 8, 50, 8, arr, arr, P, 16, P, arr, arr, arr, arr, P, 64, 16, 8, P, 16, 8, P, None]
    for fn, args, n_at, needed, unread in ((lib.vmp_svae_step_final_smm, final, 30, (0, 5, 6, 7, 8, 9, 14, 15, 16, 17, 18, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 31, 32,
                                                                                38, 39, 42), (33, 34, 47, 48)),
                                           (lib.vmp_svae_step_pack_smm, packed, 24, (0, 2, 7, 8, 9, 14, 15, 16, 18, 19, 20, 21, 22, 23, 27, 30), (31,))):
        for i in needed:
            assert fn(*[None if j == i else a for j, a in enumerate(args)]) == -1 and b'NULL' in lib.vmp_last_error(), (fn.__name__, i)
            if args[i] is arr:
                assert fn(*[nul if j == i else a for j, a in enumerate(args)]) == -1 and b'NULL' in lib.vmp_last_error(), (fn.__name__, i)
        rest = [None if j in unread else (513 if j == n_at else a) for j, a in enumerate(args)]
        assert fn(*rest) == -2 and b'range' in lib.vmp_last_error(), fn.__name__


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


def test_smm_prep_and_closing_kernels_add_no_scratch():
    """Launch 1 of the SMM step (enc_prep_smm_kernel<U tile, L>, every instance): private segment size 0.  Launch 6
    (step_final_kernel<L, true>): no more private segment than the GMM step's step_final_kernel<L, false> - the block roles the two
    share (the phi_gmm role's backward of the recognition unpacking indexes two L-sized fp64 arrays by lane, pick<L>, which the compiler
    keeps in scratch at L >= 3/4 in both instances); the SMM theta role itself adds none."""
    prep = _kernel_notes(r'enc_prep_smm_kernel')
    assert len(prep) >= 8, sorted(prep)
    assert all(v[0] == 0 for v in prep.values()), prep
    fin = _kernel_notes(r'step_final_kernelILi\dELb[01]E')
    for L in range(1, 9):
        smm = [v for k, v in fin.items() if 'ILi%dELb1E' % L in k]
        gmm = [v for k, v in fin.items() if 'ILi%dELb0E' % L in k]
        assert len(smm) == 1 and len(gmm) == 1, (L, sorted(fin))
        assert smm[0][0] <= gmm[0][0], (L, smm, gmm)
    assert all(v[0] == 0 for k, v in fin.items() if re.search(r'ILi[12]ELb1E', k)), fin


def test_student_t_minibatch_backward_kernels_do_not_spill():
    """svae_estep_bwd1_kernel<L, true, true> (the SMM step's launch 4) for L = 1..8: private segment size 0 in the code object's
    metadata (the per-pair theta sums add L + TRI registers per lane beside the Gaussian form's)."""
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
        for m in re.finditer(r'\.name:\s+(\S*svae_estep_bwd1_kernelILi(\d)ELb1ELb1E\S*).*?\.private_segment_fixed_size:\s+(\d+).*?'
                             r'\.vgpr_count:\s+(\d+)', txt, re.S):
            seen[int(m.group(2))] = (int(m.group(3)), int(m.group(4)))
    assert sorted(seen) == list(range(1, 9)), sorted(seen)
    assert all(v[0] == 0 for v in seen.values()), seen
    assert all(v[1] <= 256 for v in seen.values()), seen
