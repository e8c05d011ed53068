"""Host side of the diagonal-covariance mixture fit (csrc/vmp_diagfit.hip; include/vmp_hip.h "Diagonal-covariance mixture fitting on
wide rows"): the exports exist and agree with the ctypes table, the size queries are host arithmetic, every argument refusal happens
before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a launch on a machine
without a GPU would return a positive HIP code), the Python layer refuses what it cannot do before it touches a device, the existing
full-covariance loop still stops at D = 8, and no instantiation of the new kernels uses private memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, 8-byte aligned, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_diag_pack_words', 'vmp_mixture_diag_workspace_bytes', 'vmp_mixture_diag_pack', 'vmp_mixture_diag_pass',
         'vmp_mixture_diag_finalize', 'vmp_mixture_diag_bound_terms', 'vmp_mixture_diag_iterate')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert 'Diagonal-covariance mixture fitting on wide rows' in header and re.search(r'#define\s+VMP_DIAG_MAX_D\s+64\b', header)
    assert re.search(r'#define\s+VMP_MAX_D\s+8\b', header)
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n
    assert _lib().vmp_abi_version() == 1
    assert V._lib.DIAG_MAX_D == 64 and V._lib.MAX_D == 8


def test_size_queries_are_host_arithmetic():
    lib = _lib()
    for D in (1, 9, 17, 64):
        assert lib.vmp_mixture_diag_pack_words(D) == 2 * D + 1
    assert lib.vmp_mixture_diag_pack_words(0) == 0 and lib.vmp_mixture_diag_pack_words(65) == 0
    for D, K in ((16, 16), (64, 64)):
        prev = 0
        for N in (1, 63, 64, 65, 2047, 2048, 2049, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
            b = lib.vmp_mixture_diag_workspace_bytes(N, D, K)
            cap = 512 if K * (1 + 2 * D) <= 2048 else 256
            blocks = min(cap, max(1, -(-N // 2048)))
            # the fp64 moments of every wave (4 per block), one fp64 word per block, the pivot
            assert b == blocks * 4 * K * (1 + 2 * D) * 8 + blocks * 8 + 256, (N, D, K, b)
            assert b % 8 == 0 and b >= prev
            prev = b
        assert prev <= 80 << 20
    for D, K in ((0, 4), (65, 4), (3, 0), (3, 65)):
        assert lib.vmp_mixture_diag_workspace_bytes(1000, D, K) == 0


#          x  N    D   K   pack r_in  r  logr stats bound ws ws_bytes stream
PASS_OK = [P, 100, 33, 16, P, None, P, P, P, P, P, 1 << 30, None]
PASS_IDX = dict(x=0, N=1, D=2, K=3, pack=4, r_in=5, r=6, logr=7, stats=8, bound=9, ws=10, ws_bytes=11)
#          x  N    D   K   prior x 5      r  logr posterior x 8           pack stats bound ws ws_bytes its stream
ITER_OK = [P, 100, 33, 16, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 1 << 30, 3, None]
ITER_IDX = dict(x=0, N=1, D=2, K=3, alpha0=4, b0=8, r=9, logr=10, alpha=11, b=15, xbar=16, S=17, pi=18, pack=19, stats=20, bound=21,
                ws=22, ws_bytes=23, iterations=24)


def _call(name, ok, idx, **kw):
    args = list(ok)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return getattr(lib, name)(*args), lib.vmp_last_error()


COMMON = [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=65), DIM, b'D=65'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(r=None), BADARG, b'logr_out needs r_out'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'aligned'),
]


@pytest.mark.parametrize('kw,code,word', COMMON + [
    (dict(r=None, logr=None, stats=None, bound=None), BADARG, b'no output'),
    (dict(r_in=P), BADARG, b'r_in'),
    (dict(r_in=P, r=None, logr=None), BADARG, b'r_in'),
])
def test_pass_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_diag_pass', PASS_OK, PASS_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_pass' in msg and word in msg, (kw, msg)


@pytest.mark.parametrize('kw,code,word', COMMON + [
    (dict(iterations=-1), BADARG, b'iterations'),
    (dict(alpha0=None), BADARG, b'null pointer'),
    (dict(b0=None), BADARG, b'null pointer'),
    (dict(alpha=None), BADARG, b'null pointer'),
    (dict(b=None), BADARG, b'null pointer'),
    (dict(stats=None), BADARG, b'null pointer (stats)'),
])
def test_iterate_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_diag_iterate', ITER_OK, ITER_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_iterate' in msg and word in msg, (kw, msg)


def test_iterate_with_zero_iterations_launches_nothing():
    rc, msg = _call('vmp_mixture_diag_iterate', ITER_OK, ITER_IDX, iterations=0)
    assert rc == 0, (rc, msg)
    rc, msg = _call('vmp_mixture_diag_iterate', ITER_OK, ITER_IDX, iterations=0, r=None, logr=None, bound=None, xbar=None, S=None, pi=None)
    assert rc == 0, (rc, msg)


def test_workspace_bound_is_exact():
    need = _lib().vmp_mixture_diag_workspace_bytes(10 ** 6, 33, 16)
    rc, msg = _call('vmp_mixture_diag_pass', PASS_OK, PASS_IDX, N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)


def test_k_sized_entry_points_refuse_on_the_host():
    lib = _lib()
    pack = [33, 16, P, P, P, P, P, P, None]
    fin = [P, 33, 16] + [P] * 5 + [P] * 8 + [None]
    terms = [33, 16] + [P] * 10 + [P, None]
    for name, ok, d_at, k_at, ptrs in (('vmp_mixture_diag_pack', pack, 0, 1, range(2, 8)),
                                        ('vmp_mixture_diag_finalize', fin, 1, 2, [0] + list(range(3, 13))),
                                        ('vmp_mixture_diag_bound_terms', terms, 0, 1, range(2, 13))):
        fn = getattr(lib, name)
        for at, v in ((d_at, 0), (d_at, 65), (k_at, 0), (k_at, 65)):
            assert fn(*[v if j == at else a for j, a in enumerate(ok)]) == DIM and name.encode() in lib.vmp_last_error(), (name, at, v)
        for i in ptrs:
            assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == BADARG and b'null pointer' in lib.vmp_last_error(), (name, i)


def _cpu_case():
    N, D, K = 7, 12, 3
    return N, D, K, torch.zeros(N, D), torch.full((N, K), 1.0 / K)


def test_the_full_covariance_loop_still_stops_at_8_dimensions():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm
    x, r0 = torch.zeros(7, 9), torch.full((7, 3), 1.0 / 3)
    with pytest.raises(V._lib.VmpError):
        _mix.VMPLoop(x, r0, V._lib.VMP_GMM)
    with pytest.raises(V._lib.VmpError, match='D=9'):
        _mix._dims(x, 3)                                        # the check VMPLoop makes once x is on a device (tests/test_mix_diag_gpu.py)
    lib = _lib()
    assert lib.vmp_mixture_wfit_workspace_bytes(100, 9, 3) == 0 and lib.vmp_mixture_fit_workspace_bytes(100, 9, 3) == 0
    assert lib.vmp_mix_stats_ws(P, P, None, P, 100, 9, 3, P, 1 << 30, None) == DIM and b'D=9' in lib.vmp_last_error()
    assert lib.vmp_mix_pack_words(8) == 48 and V._lib.MAX_D == 8


def test_python_refusals_come_before_the_device():
    """CPU tensors throughout: each call is refused for the stated reason, not for being on the CPU"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _diag, _mix, gmm
    E = V._lib.VmpError
    N, D, K, x, r0 = _cpu_case()
    assert _mix.DiagLoop is _diag.DiagLoop and _mix.default_diag_prior is _diag.default_diag_prior
    for kw, word in ((dict(miss=torch.zeros(N, D, dtype=torch.bool)), 'no masks'), (dict(weights=torch.ones(N)), 'no weights'),
                     (dict(flavour=V._lib.VMP_SMM), 'Student-t'), (dict(accurate=True), 'accurate')):
        with pytest.raises(E, match=word):
            _mix.DiagLoop(x, r0, **kw)
    with pytest.raises(E, match='D=65'):
        _mix.DiagLoop(torch.zeros(N, 65), r0)
    with pytest.raises(E, match='K=65'):
        _mix.DiagLoop(x, torch.zeros(N, 65))
    with pytest.raises(E, match='r_init has shape'):
        _mix.DiagLoop(x, r0[:3])
    with pytest.raises(E, match='alpha_0 has shape'):
        _mix.DiagLoop(x, r0, prior=_mix.default_diag_prior(x, K + 1))
    with pytest.raises(E, match='cpu'):
        _mix.DiagLoop(x, r0)
    with pytest.raises(E, match='cpu'):
        gmm.inference_diag(x, K, 0)
    with pytest.raises(E, match="only 'random'"):
        gmm.inference_diag(x, K, 0, init='kmeans++')
    pack = torch.zeros(K, 2 * D + 1)
    with pytest.raises(E, match='no diagonal pack'):
        _mix.mixture_diag_pass(x, torch.zeros(K, 2 * D))
    with pytest.raises(E, match='no output'):
        _mix.mixture_diag_pass(x, pack, want_r=False, want_stats=False)
    with pytest.raises(E, match='needs want_r'):
        _mix.mixture_diag_pass(x, pack, want_r=False, want_logr=True)
    with pytest.raises(E, match='r_in has shape'):
        _mix.mixture_diag_pass(x, pack, r_in=r0[:3], want_r=False)
    with pytest.raises(E, match='moments only'):
        _mix.mixture_diag_pass(x, pack, r_in=r0)
    with pytest.raises(E, match='cpu'):
        _mix.mixture_diag_pass(x, pack)
    prior = _mix.default_diag_prior(x, K)
    assert [tuple(t.shape) for t in prior] == [(K,), (K,), (K, D), (K,), (K, D)]
    assert prior[0][0].item() == pytest.approx(0.05 / K) and prior[1][0].item() == 0.5 and prior[3][0].item() == 1 and prior[4][0, 0].item() == 1
    with pytest.raises(E, match='b has shape'):
        _mix.diag_pack(prior[0], prior[1], prior[2], prior[3], prior[4][:, :2])
    with pytest.raises(E, match='cpu'):
        _mix.diag_pack(*prior)
    with pytest.raises(E, match='cpu'):
        gmm.lower_bound_diag(x, *prior)
    with pytest.raises(E, match='float64'):
        _mix.diag_finalize(torch.zeros(K, 1 + 2 * D), prior)
    with pytest.raises(E, match='cpu'):
        _mix.diag_finalize(torch.zeros(K, 1 + 2 * D, dtype=torch.float64), prior)
    with pytest.raises(E, match='cpu'):
        _mix.diag_bound_terms(prior, prior)
    with pytest.raises(E, match='smooth'):
        _mix.DiagLoop.from_centers(x, torch.zeros(K, D), smooth=1.0)
    with pytest.raises(E, match='centers has shape'):
        _mix.DiagLoop.from_centers(x, torch.zeros(K, D + 1))
    # the nearest-centre start is torch plumbing: ties go to the lowest k, the smoothing is seed_assign's
    r = _mix.nearest_center_r(torch.tensor([[0.0, 0.0], [4.0, 0.0], [1.0, 0.0]]), torch.tensor([[2.0, 0.0], [0.0, 0.0], [2.0, 0.0]]), smooth=0.3)
    assert r.argmax(1).tolist() == [1, 0, 0] and r.dtype == torch.float32
    assert r[0].tolist() == pytest.approx([0.1, 0.8, 0.1])


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


def test_diag_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..64 x (K <= 16 | K > 16)) and the four K-sized kernels: private segment
    size 0 in the shipped code object (profiles/NOTES_mix_diagfit.md lists the registers)"""
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
        for m in re.finditer(r'\.name:\s+(\S*diag_(?:pass|reduce|mstep|pack|terms)_kernel\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 64 * 2 + 4, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
