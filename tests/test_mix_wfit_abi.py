"""Host side of the mixture fit on weighted rows (csrc/vmp_wfit.hip; include/vmp_hip.h "Mixture fitting on weighted rows"): the three
exports exist and agree with the ctypes table, the size query is host arithmetic, every argument refusal of the pass and the
iteration happens before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a launch
on a machine without a GPU would return a positive HIP code), the Python layer refuses what it cannot do before it touches a device,
and no instantiation of the new kernels uses private memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, 8-byte aligned, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_wfit_workspace_bytes', 'vmp_mixture_wfit_pass', 'vmp_mixture_wfit_iterate')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_three_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert 'Mixture fitting on weighted rows' in header
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n
    assert _lib().vmp_abi_version() == 1


def test_workspace_bytes_is_host_arithmetic():
    lib = _lib()
    prev = 0
    for N in (1, 2, 63, 127, 128, 129, 511, 512, 513, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
        b = lib.vmp_mixture_wfit_workspace_bytes(N, 8, 16)
        assert b > 0 and b % 8 == 0 and b >= prev, (N, b, prev)
        # the slab of the masked fit (the same geometry) plus one fp64 partial per block of 512 rows, at most 512 blocks
        blocks = min(512, max(1, -(-N // 512)))
        assert b == lib.vmp_mixture_fit_workspace_bytes(N, 8, 16) + 8 * blocks, N
        prev = b
    assert prev == lib.vmp_mixture_wfit_workspace_bytes(2 ** 50, 8, 16) <= 64 << 20
    for D, K in ((0, 4), (9, 4), (3, 0), (3, 65)):
        assert lib.vmp_mixture_wfit_workspace_bytes(1000, D, K) == 0


#          x  w  mask N    D  K   pack r  logr fill stats bound ws ws_bytes  stream
PASS_OK = [P, P, P, 100, 8, 16, P, P, P, P, P, P, P, 1 << 30, None]
PASS_IDX = dict(x=0, w=1, mask=2, N=3, D=4, K=5, pack=6, r=7, logr=8, fill=9, stats=10, bound=11, ws=12, ws_bytes=13)
#          x  w  mask N    D  K   prior x 5        r  logr fill posterior x 8              pack stats bound ws ws_bytes its stream
ITER_OK = [P, P, P, 100, 8, 16, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 1 << 30, 3, None]
ITER_IDX = dict(x=0, w=1, mask=2, N=3, D=4, K=5, alpha0=6, v0=10, r=11, logr=12, fill=13, alpha=14, v=18, xbar=19, S=20, pi=21, pack=22,
                stats=23, bound=24, ws=25, ws_bytes=26, iterations=27)


def _call(name, ok, idx, **kw):
    args = list(ok)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return getattr(lib, name)(*args), lib.vmp_last_error()


COMMON = [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=9), DIM, b'D=9'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(w=None), BADARG, b'(w)'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(mask=None), BADARG, b'x_fill_out needs a mask'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'aligned'),
]


@pytest.mark.parametrize('kw,code,word', COMMON + [
    (dict(r=None), BADARG, b'stats_out needs r_out'),
    (dict(r=None, stats=None), BADARG, b'logr_out needs r_out'),
    (dict(r=None, logr=None, fill=None, stats=None, bound=None), BADARG, b'no output'),
])
def test_pass_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_wfit_pass', PASS_OK, PASS_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_wfit_pass' in msg and word in msg, (kw, msg)


@pytest.mark.parametrize('kw,code,word', COMMON + [
    (dict(iterations=-1), BADARG, b'iterations'),
    (dict(alpha0=None), BADARG, b'null pointer'),
    (dict(v0=None), BADARG, b'null pointer'),
    (dict(alpha=None), BADARG, b'null pointer'),
    (dict(v=None), BADARG, b'null pointer'),
    (dict(stats=None), BADARG, b'null pointer (stats)'),
    (dict(r=None), BADARG, b'null pointer (r)'),
])
def test_iterate_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_wfit_iterate', ITER_OK, ITER_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_wfit_iterate' in msg and word in msg, (kw, msg)


def test_iterate_with_zero_iterations_launches_nothing():
    rc, msg = _call('vmp_mixture_wfit_iterate', ITER_OK, ITER_IDX, iterations=0)
    assert rc == 0, (rc, msg)
    # without a mask and without x_fill the same holds; so does the iteration without a bound
    rc, msg = _call('vmp_mixture_wfit_iterate', ITER_OK, ITER_IDX, iterations=0, mask=None, fill=None, bound=None, logr=None)
    assert rc == 0, (rc, msg)


def test_workspace_bound_is_exact():
    need = _lib().vmp_mixture_wfit_workspace_bytes(10 ** 6, 8, 16)
    rc, msg = _call('vmp_mixture_wfit_pass', PASS_OK, PASS_IDX, N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)


def _cpu_case():
    N, D, K = 7, 3, 4
    x, r0 = torch.zeros(N, D), torch.full((N, K), 1.0 / K)
    return N, D, K, x, r0, torch.ones(N), torch.zeros(N, D, dtype=torch.bool)


def test_weighted_loop_refusals_come_before_the_device():
    """CPU tensors throughout: each call is refused for the stated reason, not for being on the CPU"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm, parallel_mix
    E = V._lib.VmpError
    N, D, K, x, r0, w, miss = _cpu_case()
    with pytest.raises(E, match='Student-t'):
        _mix.VMPLoop(x, r0, V._lib.VMP_SMM, kappa=torch.full((K,), 5.0), weights=w)
    with pytest.raises(E, match='accurate'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, accurate=True, weights=w)
    with pytest.raises(E, match='Student-t'):
        _mix.VMPLoop.from_seed_weighted(x, w, K, V._lib.VMP_SMM, 0)
    for bad in (w[:3], torch.ones(N, 1), torch.ones(N + 1), 'w', 1.0):
        with pytest.raises(E, match='weights have shape'):
            _mix.VMPLoop(x, r0, V._lib.VMP_GMM, weights=bad)
        with pytest.raises(E, match='weights have shape'):
            gmm.inference_weighted(x, bad, K, 0, r_init=r0)
        with pytest.raises(E, match='weights have shape'):
            _mix.check_weights(x, bad)
    with pytest.raises(E, match='weights are on meta'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, weights=torch.ones(N, device='meta'))
    with pytest.raises(E, match='float32'):
        _mix.check_weights(x, torch.ones(N, dtype=torch.float64))
    for bad, word in ((torch.tensor([1., 1, -0.5, 1, 1, 1, 1]), 'negative'), (torch.tensor([1., 1, float('nan'), 1, 1, 1, 1]), 'finite'),
                      (torch.tensor([1., 1, float('inf'), 1, 1, 1, 1]), 'finite'), (torch.zeros(N), 'zero')):
        with pytest.raises(E, match=word):
            _mix.check_weights(x, bad)
        with pytest.raises(E, match=word):
            _mix.VMPLoop(x, r0, V._lib.VMP_GMM, weights=bad)
        with pytest.raises(E, match=word):
            _mix.VMPLoop.from_seed_weighted(x, bad, K, V._lib.VMP_GMM, 0)
        with pytest.raises(E, match=word):
            gmm.inference_weighted(x, bad, K, 0)
    assert _mix.check_weights(x, w) is w
    # the mask of a weighted loop is checked as that of a masked one
    with pytest.raises(E, match='mask has shape'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, weights=w, miss=miss[:, :2])
    # a well-formed weighted loop on CPU tensors: no CPU fallback
    with pytest.raises(E, match='cpu'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, weights=w)
    with pytest.raises(E, match='cpu'):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM, weights=w, miss=miss)
    with pytest.raises(E, match='cpu'):
        gmm.inference_weighted(x, w, K, 0, r_init=r0)
    # the data-parallel loop has no weighted pass
    with pytest.raises(E, match='single-device'):
        parallel_mix.DistributedVMPLoop(x, r0, V._lib.VMP_GMM, weights=w)


def test_pass_and_bound_wrappers_refuse_mismatch_before_the_library():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm
    E = V._lib.VmpError
    N, D, K, x, r0, w, miss = _cpu_case()
    pack = torch.zeros(K, D + D * (D + 1) // 2 + 1)
    with pytest.raises(E, match='no fit pack'):
        _mix.mixture_wfit_pass(x, w, torch.zeros(K, D + D * (D + 1) // 2 + 4))
    with pytest.raises(E, match='x must be'):
        _mix.mixture_wfit_pass(torch.zeros(N), w, pack)
    with pytest.raises(E, match='weights have shape'):
        _mix.mixture_wfit_pass(x, w[:3], pack)
    with pytest.raises(E, match='mask has shape'):
        _mix.mixture_wfit_pass(x, w, pack, miss=miss[:3])
    with pytest.raises(E, match='no output'):
        _mix.mixture_wfit_pass(x, w, pack, want_r=False, want_stats=False)
    with pytest.raises(E, match='need want_r'):
        _mix.mixture_wfit_pass(x, w, pack, want_r=False, want_bound=True)
    with pytest.raises(E, match='need want_r'):
        _mix.mixture_wfit_pass(x, w, pack, want_r=False, want_stats=False, want_logr=True)
    with pytest.raises(E, match='needs a mask'):
        _mix.mixture_wfit_pass(x, w, pack, want_fill=True)
    with pytest.raises(E, match='cpu'):
        _mix.mixture_wfit_pass(x, w, pack)
    with pytest.raises(E, match='cpu'):
        _mix.mixture_wfit_pass(x, w, pack, miss=miss, want_fill=True, want_bound=True)
    th = (torch.ones(K), torch.ones(K), torch.zeros(K, D), torch.eye(D).expand(K, D, D).contiguous(), torch.full((K,), D + 2.0))
    with pytest.raises(E, match='weights have shape'):
        _mix.lower_bound(x, th, weights=w[:3])
    with pytest.raises(E, match='weights have shape'):
        gmm.lower_bound(x, *th, weights=torch.ones(N, 2))
    with pytest.raises(E, match='cpu'):
        gmm.lower_bound(x, *th, weights=w)


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


def test_wfit_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..8 x (K <= 16 | K > 16) x (complete | masked)), the reduction and the
    one-wave sum: private segment size 0 in the shipped code object (profiles/NOTES_mix_wfit.md lists the registers)"""
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
        for m in re.finditer(r'\.name:\s+(\S*wfit_(?:pass_kernel|unshift_kernel|sum_kernel)\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 8 * 2 * 2 + 8 + 1, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
