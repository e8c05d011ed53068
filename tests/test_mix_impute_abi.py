"""Host side of mixture imputation (csrc/vmp_impute.hip; include/vmp_hip.h "Mixture imputation"): the five exports exist and agree
with the ctypes table, the size queries are host arithmetic, every argument refusal of vmp_mixture_impute / the two pack builders
happens before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a launch on a
machine without a GPU would return a positive HIP code), the Python wrappers refuse mismatched shapes before they touch the library
or the device, and no instantiation of the kernels uses private memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_impute_pack_words', 'vmp_mixture_impute_pack_niw', 'vmp_mixture_impute_pack_t',
         'vmp_mixture_impute_workspace_bytes', 'vmp_mixture_impute')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_five_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n


def test_pack_words_and_workspace_bytes():
    lib = _lib()
    for D in range(1, 9):
        # mu | Lambda | log w, nu, log det Lambda, 1 / nu | G[0..D]
        assert lib.vmp_mixture_impute_pack_words(D) == D + D * (D + 1) // 2 + 4 + (D + 1), D
    assert lib.vmp_mixture_impute_pack_words(0) == 0 and lib.vmp_mixture_impute_pack_words(9) == 0
    prev = 0
    for N in (1, 2, 63, 64, 65, 255, 256, 257, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
        b = lib.vmp_mixture_impute_workspace_bytes(N, 8, 16)
        assert b > 0 and b % 8 == 0 and b >= prev, (N, b, prev)
        prev = b
    assert prev <= 1 << 20                           # bounded: one fp64 word per block of a capped grid
    assert lib.vmp_mixture_impute_workspace_bytes(10 ** 6, 1, 1) == lib.vmp_mixture_impute_workspace_bytes(10 ** 6, 8, 64)


#             x  mask N    D  K   pack x_out logp resp sum ws  ws_bytes  stream
IMPUTE_OK = [P, P, 100, 8, 16, P, P, P, P, P, P, 1 << 20, None]


def _impute(**kw):
    idx = dict(x=0, mask=1, N=2, D=3, K=4, pack=5, x_out=6, logp=7, resp=8, sum=9, ws=10, ws_bytes=11)
    args = list(IMPUTE_OK)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return lib.vmp_mixture_impute(*args), lib.vmp_last_error()


@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=9), DIM, b'D=9'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(mask=None), BADARG, b'(mask)'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(x_out=None, logp=None, resp=None, sum=None), BADARG, b'no output'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(N=0), BADARG, b'N'),
    (dict(N=-3), BADARG, b'N'),
])
def test_impute_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _impute(**kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_impute' in msg and word in msg, (kw, msg)


def test_impute_workspace_is_only_needed_for_the_sum():
    """without sum_out a NULL workspace passes the host checks: what is refused next is N (nothing launched)"""
    rc, msg = _impute(sum=None, ws=None, ws_bytes=0, N=0)
    assert rc == BADARG and b'N must be positive' in msg, (rc, msg)
    need = _lib().vmp_mixture_impute_workspace_bytes(10 ** 6, 8, 16)
    rc, msg = _impute(N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)


@pytest.mark.parametrize('name,nptr', [('vmp_mixture_impute_pack_niw', 6), ('vmp_mixture_impute_pack_t', 5)])
def test_pack_builders_check_on_the_host(name, nptr):
    lib = _lib()
    fn = getattr(lib, name)
    for D, K, word in ((0, 4, b'D=0'), (9, 4, b'D=9'), (3, 65, b'K=65'), (3, 0, b'K=0')):
        assert fn(D, K, *([P] * nptr), None) == DIM and word in lib.vmp_last_error(), (name, D, K)
    for i in range(nptr):
        ptrs = [None if j == i else P for j in range(nptr)]
        assert fn(3, 4, *ptrs, None) == BADARG and name.encode() in lib.vmp_last_error(), (name, i)


def _theta(K, D):
    return (torch.ones(K), torch.ones(K), torch.zeros(K, D), torch.eye(D).expand(K, D, D).contiguous(), torch.full((K,), D + 2.0))


def test_wrappers_refuse_shape_mismatch_before_the_library():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import gmm, smm
    E = V._lib.VmpError
    N, D, K = 7, 3, 4
    x, miss = torch.zeros(N, D), torch.zeros(N, D, dtype=torch.uint8)
    al, be, m, C, v = _theta(K, D)
    kap = torch.full((K,), 5.0)
    bad = [(torch.zeros(N, D + 1), miss, al, be, m, C, v), (x, miss[:, :2], al, be, m, C, v), (x, miss[:3], al, be, m, C, v),
           (x, None, al, be, m, C, v), (x, miss, al[:3], be, m, C, v), (x, miss, al, be[:3], m, C, v),
           (x, miss, al, be, torch.zeros(K, D + 1), C, v), (x, miss, al, be, m, C[:, :2], v), (x, miss, al, be, m, C[:3], v),
           (x, miss, al, be, m, C, v[:, None]), (torch.zeros(N), miss, al, be, m, C, v)]
    for args in bad:
        with pytest.raises(E, match='shape|must be'):
            gmm.predictive_impute(*args)
        with pytest.raises(E, match='shape|must be'):
            smm.heldout_impute(*args, kap)
    with pytest.raises(E, match='kappa_k has shape'):
        smm.heldout_impute(x, miss, al, be, m, C, v, kap[:2])
    log_pi = torch.zeros(K)
    for args in ((torch.zeros(N, D + 1), miss, m, C, v, log_pi), (x, miss[:, :1], m, C, v, log_pi), (x, miss, m, C[:3], v, log_pi),
                 (x, miss, m, C, v[:2], log_pi), (x, miss, m, C, v, log_pi[:1]), (x, miss, m, torch.zeros(K, D, D + 1), v, log_pi)):
        with pytest.raises(E, match='shape|must be'):
            student_t.mixture_impute(*args)
    with pytest.raises(E, match='compiled range'):
        gmm.predictive_impute(torch.zeros(N, 9), torch.zeros(N, 9, dtype=torch.uint8), *_theta(K, 9))
    with pytest.raises(E, match='compiled range'):
        gmm.predictive_impute(x, miss, *_theta(65, D))


def test_wrappers_have_no_cpu_fallback():
    """well-formed CPU operands: refused by the operand check (VmpError), not evaluated in torch"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import gmm, smm
    al, be, m, C, v = _theta(4, 3)
    x, miss = torch.zeros(7, 3), torch.zeros(7, 3, dtype=torch.bool)
    with pytest.raises(V._lib.VmpError, match='cpu'):
        gmm.predictive_impute(x, miss, al, be, m, C, v)
    with pytest.raises(V._lib.VmpError, match='cpu'):
        smm.heldout_impute(x, miss, al, be, m, C, v, torch.full((4,), 5.0))
    with pytest.raises(V._lib.VmpError, match='cpu'):
        student_t.mixture_impute(x, miss, m, C, v, torch.zeros(4))


def test_loop_has_impute():
    from vmp_for_svae_amd.models import _mix, parallel_mix
    for cls in (_mix.VMPLoop, parallel_mix.DistributedVMPLoop):
        assert callable(getattr(cls, 'impute')) and callable(getattr(cls, 'impute_pack'))


def _readelf(objdump):
    """llvm-readelf of the ROCm toolchain that built the library: beside the llvm-objdump of tools/erratum_scan.py, else beside the
    clang that hipcc drives, else on PATH.  Not found = a failure, not a skip: this check is the only guard against a spill."""
    import shutil
    cands = [objdump.replace('llvm-objdump', 'llvm-readelf')]
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if os.path.exists(hipcc):
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
        cands += [os.path.join(rocm, 'llvm', 'bin', 'llvm-readelf'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'llvm-readelf')]
    cands.append(shutil.which('llvm-readelf') or '')
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise AssertionError('llvm-readelf of the ROCm toolchain not found (tried %s): the no-scratch check cannot run' % cands)


def test_impute_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..8 x (K <= 16 | K > 16)), the two pack builders and the sum: private segment
    size 0 in the shipped code object - a spill inside the row loop is a defect (profiles/NOTES_mix_impute.md lists the registers)"""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    readelf = _readelf(E.OBJDUMP)
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S*impute_(?:kernel|pack_niw_kernel|pack_t_kernel|sum_kernel)\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 8 * 2 + 8 + 8 + 1, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
