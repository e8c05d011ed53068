"""Host side of the mixture fit on partly observed rows (csrc/vmp_missfit.hip; include/vmp_hip.h "Mixture fitting on partly observed
rows"): the five exports exist and agree with the ctypes table, the size queries are host arithmetic, every argument refusal of the
pack builder, the pass and the iteration happens before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3;
a call that reached a launch on a machine without a GPU would return a positive HIP code), VMPLoop(..., miss=) refuses what it cannot
do before it touches the device, and no instantiation of the new kernels uses private memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, 8-byte aligned, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_fit_pack_words', 'vmp_mixture_fit_pack', 'vmp_mixture_fit_workspace_bytes', 'vmp_mixture_fit_pass',
         'vmp_mixture_fit_iterate')


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
        assert lib.vmp_mixture_fit_pack_words(D) == D + D * (D + 1) // 2 + 1, D          # m | Lbar | c
    assert lib.vmp_mixture_fit_pack_words(0) == 0 and lib.vmp_mixture_fit_pack_words(9) == 0
    prev = 0
    for N in (1, 2, 63, 127, 128, 129, 511, 512, 513, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
        b = lib.vmp_mixture_fit_workspace_bytes(N, 8, 16)
        assert b > 0 and b % 8 == 0 and b >= prev, (N, b, prev)
        prev = b
    # bounded: the fp64 moments (1 + D + D(D+1)/2 words per component) of every wave of a capped grid
    assert prev == lib.vmp_mixture_fit_workspace_bytes(2 ** 50, 8, 16) and prev % (16 * 45 * 8) == 0 and prev <= 64 << 20
    assert lib.vmp_mixture_fit_workspace_bytes(10 ** 6, 8, 64) == 4 * prev
    for D, K in ((0, 4), (9, 4), (3, 0), (3, 65)):
        assert lib.vmp_mixture_fit_workspace_bytes(1000, D, K) == 0


#          x  mask N    D  K   pack r  logr fill stats ws ws_bytes  stream
PASS_OK = [P, P, 100, 8, 16, P, P, P, P, P, P, 1 << 30, None]
PASS_IDX = dict(x=0, mask=1, N=2, D=3, K=4, pack=5, r=6, logr=7, fill=8, stats=9, ws=10, ws_bytes=11)
#          x  mask N    D  K   prior x 5        r  logr fill posterior x 8              pack stats ws ws_bytes its stream
ITER_OK = [P, P, 100, 8, 16, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 1 << 30, 3, None]
ITER_IDX = dict(x=0, mask=1, N=2, D=3, K=4, alpha0=5, v0=9, r=10, logr=11, fill=12, alpha=13, v=17, xbar=18, S=19, pi=20, pack=21,
                stats=22, ws=23, ws_bytes=24, iterations=25)


def _call(name, ok, idx, **kw):
    args = list(ok)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return getattr(lib, name)(*args), lib.vmp_last_error()


CASES = [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=9), DIM, b'D=9'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(mask=None), BADARG, b'(mask)'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(r=None), BADARG, b'no output'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'aligned'),
]


@pytest.mark.parametrize('kw,code,word', CASES)
def test_pass_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_fit_pass', PASS_OK, PASS_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_fit_pass' in msg and word in msg, (kw, msg)


@pytest.mark.parametrize('kw,code,word', CASES + [
    (dict(iterations=-1), BADARG, b'iterations'),
    (dict(alpha0=None), BADARG, b'null pointer'),
    (dict(v0=None), BADARG, b'null pointer'),
    (dict(alpha=None), BADARG, b'null pointer'),
    (dict(v=None), BADARG, b'null pointer'),
    (dict(stats=None), BADARG, b'null pointer'),
])
def test_iterate_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_fit_iterate', ITER_OK, ITER_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_fit_iterate' in msg and word in msg, (kw, msg)


def test_iterate_with_zero_iterations_launches_nothing():
    rc, msg = _call('vmp_mixture_fit_iterate', ITER_OK, ITER_IDX, iterations=0)
    assert rc == 0, (rc, msg)


def test_workspace_bound_is_exact():
    need = _lib().vmp_mixture_fit_workspace_bytes(10 ** 6, 8, 16)
    rc, msg = _call('vmp_mixture_fit_pass', PASS_OK, PASS_IDX, N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)


def test_pack_builder_checks_on_the_host():
    lib = _lib()
    fn = lib.vmp_mixture_fit_pack
    for D, K, word in ((0, 4, b'D=0'), (9, 4, b'D=9'), (3, 65, b'K=65'), (3, 0, b'K=0')):
        assert fn(D, K, *([P] * 6), None) == DIM and word in lib.vmp_last_error(), (D, K)
    for i in range(6):
        ptrs = [None if j == i else P for j in range(6)]
        assert fn(3, 4, *ptrs, None) == BADARG and b'vmp_mixture_fit_pack' in lib.vmp_last_error(), i


def test_masked_loop_refusals_come_before_the_device():
    """CPU tensors throughout: each call is refused for the stated reason, not for being on the CPU"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm
    E = V._lib.VmpError
    N, D, K = 7, 3, 4
    x, r0 = torch.zeros(N, D), torch.full((N, K), 1.0 / K)
    miss = torch.zeros(N, D, dtype=torch.bool)
    with pytest.raises(E, match='Student-t'):
        _mix.VMPLoop(x, r0, V._lib.VMP_SMM, kappa=torch.full((K,), 5.0), miss=miss)
    with pytest.raises(E, match='accurate'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, accurate=True, miss=miss)
    for bad in (miss[:, :2], miss[:3], torch.zeros(N), 'mask', torch.zeros(N, D, 1)):
        with pytest.raises(E, match='mask has shape'):
            _mix.VMPLoop(x, r0, V._lib.VMP_GMM, miss=bad)
        with pytest.raises(E, match='mask has shape'):
            gmm.inference_missing(x, bad, K, 0, r_init=r0)
    with pytest.raises(E, match='mask is on meta'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, miss=torch.zeros(N, D, dtype=torch.uint8, device='meta'))
    # a well-formed masked loop on CPU tensors: no CPU fallback
    with pytest.raises(E, match='cpu'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, miss=miss)
    with pytest.raises(E, match='cpu'):
        gmm.inference_missing(x, miss, K, 0, r_init=r0)
    # miss=None is the loop as it was: the first thing refused is x on the CPU
    with pytest.raises(E, match='cpu'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM)


def test_pass_wrappers_refuse_mismatch_before_the_library():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    E = V._lib.VmpError
    K, D = 4, 3
    th = (torch.ones(K), torch.ones(K), torch.zeros(K, D), torch.eye(D).expand(K, D, D).contiguous(), torch.full((K,), D + 2.0))
    for i, bad in enumerate((torch.ones(3), torch.ones(K, 1), torch.zeros(K, D + 1), torch.zeros(K, D, 2), torch.ones(K, 2))):
        args = list(th)
        args[i] = bad
        with pytest.raises(E, match='shape'):
            _mix.fit_pack(*args)
    with pytest.raises(E, match='cpu'):
        _mix.fit_pack(*th)
    with pytest.raises(E, match='cpu'):
        _mix.mixture_fit_pass(torch.zeros(7, D), torch.zeros(7, D, dtype=torch.uint8), torch.zeros(K, 10))
    assert callable(_mix.VMPLoop.filled)


def _readelf(objdump):
    """llvm-readelf of the ROCm toolchain that built the library; not found = a failure, not a skip"""
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


def test_fit_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..8 x (K <= 16 | K > 16)), the pack builder and the reduction: private
    segment size 0 in the shipped code object (profiles/NOTES_mix_missfit.md lists the registers)"""
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
        for m in re.finditer(r'\.name:\s+(\S*fit_(?:kernel|pack_kernel|reduce_kernel)\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 8 * 2 + 8 + 8, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
