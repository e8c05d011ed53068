"""Host side of the seeded start of the diagonal mixture on wide rows (csrc/vmp_diagseed.hip; include/vmp_hip.h "Diagonal-covariance
mixture: seeded start on wide rows"): the exports exist with the declared signatures, the workspace query is host arithmetic, every
argument refusal happens before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a
launch on a machine without a GPU would return a positive HIP code), the Python surface refuses before it calls the library, and no
instantiation of the two kernels uses private memory."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import test_mix_diag_abi as A

ROOT = A.ROOT
P = A.P
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_diag_seed_workspace_bytes', 'vmp_mixture_diag_seed_centers', 'vmp_mixture_diag_seed_assign')
BIG = 1 << 40


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert 'Diagonal-covariance mixture: seeded start on wide rows' in header
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n) and n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n
    c = ctypes
    assert V._lib._SIGNATURES[NAMES[0]] == (c.c_size_t, [c.c_int64, c.c_int, c.c_int])
    # x N D K seed centers_out index_out mind2_out ws ws_bytes stream
    assert V._lib._SIGNATURES[NAMES[1]] == (c.c_int, [c.c_void_p, c.c_int64, c.c_int, c.c_int, c.c_uint64] + [c.c_void_p] * 4
                                            + [c.c_size_t, c.c_void_p])
    # x N D K centers smooth r_out z_out stream
    assert V._lib._SIGNATURES[NAMES[2]] == (c.c_int, [c.c_void_p, c.c_int64, c.c_int, c.c_int, c.c_void_p, c.c_float] + [c.c_void_p] * 3)
    decl = {n: re.search(r'\b%s\s*\(([^)]*)\)' % n, header).group(1) for n in NAMES}
    assert [len(decl[n].split(',')) for n in NAMES] == [3, 11, 9]
    assert re.search(r'uint64_t\s+seed', decl[NAMES[1]]) and re.search(r'int64_t\s*\*\s*index_out', decl[NAMES[1]])
    assert re.search(r'float\s+smooth', decl[NAMES[2]]) and re.search(r'int32_t\s*\*\s*z_out', decl[NAMES[2]])
    assert 'mask' not in decl[NAMES[1]] and 'mask' not in decl[NAMES[2]]


def test_the_workspace_query_is_host_arithmetic():
    q = _lib().vmp_mixture_diag_seed_workspace_bytes
    assert q(0, 16, 16) == 0 and q(-5, 16, 16) == 0
    for D, K in ((0, 4), (65, 4), (3, 0), (3, 65)):
        assert q(1000, D, K) == 0
    for D in (1, 9, 32, 33, 64):
        cap = 512 if D > 32 else 1024
        prev = 0
        for N in (1, 2, 63, 64, 65, 1024, 1025, 4099, 512 * 1024, 512 * 1024 + 1, 10 ** 6, 1 << 20, (1 << 20) + 1, 1 << 31, 1 << 40):
            b = q(N, D, 16)
            blocks = min(cap, -(-N // 1024))
            # the header's formula: w padded to 16 bytes, then the double-buffered candidates (int64 row, fp32 value) padded to 16
            assert b == -(-4 * N // 16) * 16 + -(-2 * blocks * 12 // 16) * 16, (N, D, b)
            assert b % 8 == 0 and b >= prev, (N, D, b)
            assert q(N, D, 1) == b and q(N, D, 64) == b                         # a function of (N, D)
            prev = b


#             x  N    D   K   seed centers index mind2 ws ws_bytes stream
CENTERS_OK = [P, 100, 33, 16, 7, P, P, P, P, BIG, None]
CENTERS_AT = dict(x=0, N=1, D=2, K=3, seed=4, centers_out=5, index_out=6, mind2_out=7, ws=8, ws_bytes=9)
#            x  N    D   K   centers smooth r_out z_out stream
ASSIGN_OK = [P, 100, 33, 16, P, 0.0, P, P, None]
ASSIGN_AT = dict(x=0, N=1, D=2, K=3, centers=4, smooth=5, r_out=6, z_out=7)


def _call(name, ok, at, kw):
    args = list(ok)
    for k, v in kw.items():
        args[at[k]] = v
    lib = _lib()
    return getattr(lib, name)(*args), lib.vmp_last_error() or b''


def test_the_complete_argument_lists_pass_the_checks_up_to_the_size_of_the_workspace():
    """the tables above are well-formed: with a workspace one byte short the only complaint is the workspace"""
    need = _lib().vmp_mixture_diag_seed_workspace_bytes(100, 33, 16)
    for kw in (dict(), dict(index_out=None), dict(mind2_out=None), dict(index_out=None, mind2_out=None), dict(D=64, K=64), dict(D=1, K=1)):
        kw['ws_bytes'] = need - 1
        rc, msg = _call('vmp_mixture_diag_seed_centers', CENTERS_OK, CENTERS_AT, kw)
        assert rc == WS and b'workspace too small' in msg, (kw, rc, msg)


@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=65), DIM, b'D=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(K=65), DIM, b'K=65'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(centers_out=None), BADARG, b'(centers_out)'),
    (dict(ws=None), WS, b'workspace too small'),
    (dict(ws_bytes=16), WS, b'workspace too small'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'not 8-byte aligned'),
])
def test_centers_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_diag_seed_centers', CENTERS_OK, CENTERS_AT, kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_seed_centers' in msg and word in msg, (kw, msg)


@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=65), DIM, b'D=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(K=65), DIM, b'K=65'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(centers=None), BADARG, b'(centers)'),
    (dict(r_out=None, z_out=None), BADARG, b'no output'),
    (dict(smooth=1.0), BADARG, b'smooth'),
    (dict(smooth=-0.25), BADARG, b'smooth'),
    (dict(smooth=float('nan')), BADARG, b'smooth'),
    (dict(smooth=float('inf')), BADARG, b'smooth'),
])
def test_assign_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_diag_seed_assign', ASSIGN_OK, ASSIGN_AT, kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_seed_assign' in msg and word in msg, (kw, msg)


def test_the_surface_exists():
    from vmp_for_svae_amd.models import _diag, _mix, gmm
    assert _mix.diag_seed_centers is _diag.diag_seed_centers and _mix.diag_seed_assign is _diag.diag_seed_assign
    assert list(inspect.signature(_mix.diag_seed_centers).parameters) == ['x', 'K', 'seed', 'want_index', 'want_mind2']
    assert list(inspect.signature(_mix.diag_seed_assign).parameters) == ['x', 'centers', 'smooth', 'want_z']
    assert inspect.ismethod(_mix.DiagLoop.from_seed)                            # a classmethod
    sig = inspect.signature(_mix.DiagLoop.from_seed).parameters
    assert list(sig) == ['x', 'K', 'seed', 'smooth', 'prior']
    assert sig['smooth'].default == inspect.signature(_mix.VMPLoop.from_seed).parameters['smooth'].default
    assert inspect.signature(gmm.inference_diag).parameters['init'].default == 'random'


def test_wrappers_refuse_before_the_library_is_called(monkeypatch):
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm
    E = V._lib.VmpError

    def no_library():
        raise AssertionError('the library was called')
    monkeypatch.setattr(V._lib, 'lib', no_library)
    N, D, K = 7, 12, 3
    x, cen = torch.zeros(N, D), torch.zeros(K, D)
    for xb in (torch.zeros(N), None, torch.zeros(0, D)):
        with pytest.raises(E, match='must be'):
            _mix.diag_seed_centers(xb, K, 1)
    for xb, cb in ((torch.zeros(N), cen), (x, torch.zeros(K, D + 1)), (x, torch.zeros(K)), (x, None)):
        with pytest.raises(E, match='shape|must be'):
            _mix.diag_seed_assign(xb, cb)
    with pytest.raises(E, match='centers is on meta'):
        _mix.diag_seed_assign(x, torch.zeros(K, D, device='meta'))
    for seed in (-1, 1 << 64):
        with pytest.raises(E, match='seed'):
            _mix.diag_seed_centers(x, K, seed)
    for smooth in (1.0, -0.1, float('nan')):
        with pytest.raises(E, match='smooth'):
            _mix.diag_seed_assign(x, cen, smooth=smooth)
    with pytest.raises(E, match='D=65'):
        _mix.diag_seed_centers(torch.zeros(N, 65), K, 1)
    with pytest.raises(E, match='K=65'):
        _mix.diag_seed_centers(x, 65, 1)
    with pytest.raises(E, match='K=0'):
        _mix.diag_seed_centers(x, 0, 1)
    # well-formed operands on the CPU: refused by the operand check - there is no CPU fallback
    with pytest.raises(E, match='cpu'):
        _mix.diag_seed_centers(x, K, 1)
    with pytest.raises(E, match='cpu'):
        _mix.diag_seed_assign(x, cen)
    with pytest.raises(E, match='cpu'):
        _mix.DiagLoop.from_seed(x, K, 1)
    with pytest.raises(E, match='cpu'):
        gmm.inference_diag(x, K, 0, init='kmeans++')
    with pytest.raises(E, match="init='nonsense'"):
        gmm.inference_diag(x, K, 0, init='nonsense')


def test_diagseed_kernels_use_no_scratch():
    """every instantiation of the two kernels (D = 1..64): private segment size 0 in the shipped code object
    (profiles/NOTES_mix_diagseed.md lists the registers)"""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    readelf = A._readelf(E.OBJDUMP)
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S*(?:18dseed_round_kernelILi|19dseed_assign_kernelILi)\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 64 * 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
