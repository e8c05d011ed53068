"""Host side of mixture scoring (csrc/vmp_score.hip; include/vmp_hip.h "Mixture scoring"): the four exports exist and agree with
the ctypes table, the workspace query is host arithmetic, every argument refusal of vmp_mix_score / the two pack builders happens
before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a launch on a machine
without a GPU would return hipGetLastError()'s positive code), and the Python wrappers refuse mismatched shapes before they touch
the library or the device (CPU tensors)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mix_score_pack_niw', 'vmp_mix_score_pack_t', 'vmp_mix_score_workspace_bytes', 'vmp_mix_score')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_four_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n
    assert raw.vmp_abi_version() == 1


def test_header_prototypes_match_the_ctypes_table():
    """argument by argument: pointer / integer width, as tests/test_abi.py does for the whole header"""
    import vmp_for_svae_amd as V
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    c = ctypes
    want = {'int': c.c_int, 'int64_t': c.c_int64, 'size_t': c.c_size_t}
    for n in NAMES:
        m = re.search(r'([A-Za-z_]\w*)\s+%s\s*\(([^()]*)\)\s*;' % n, header)
        assert m, n
        res, argtypes = V._lib._SIGNATURES[n]
        assert res is want[m.group(1)], (n, m.group(1))
        decls = [a.strip() for a in m.group(2).split(',')]
        assert len(decls) == len(argtypes), n
        for i, (d, t) in enumerate(zip(decls, argtypes)):
            if '*' in d:
                assert t is c.c_void_p, (n, i, d)
            else:
                assert t is want[[w for w in d.split() if w != 'const'][0]], (n, i, d)


def test_workspace_bytes_is_positive_and_monotone_in_n():
    lib = _lib()
    prev = 0
    for N in (1, 2, 63, 64, 65, 255, 256, 257, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
        b = lib.vmp_mix_score_workspace_bytes(N, 8, 16)
        assert b > 0 and b % 8 == 0, (N, b)
        assert b >= prev, (N, b, prev)
        prev = b
    assert prev <= 1 << 20                           # bounded: one fp64 word per block of a capped grid
    assert lib.vmp_mix_score_workspace_bytes(10 ** 6, 1, 1) == lib.vmp_mix_score_workspace_bytes(10 ** 6, 8, 64)


#               x  N    D  K   pack logp resp sum ws  ws_bytes  stream
SCORE_OK = [P, 100, 8, 16, P, P, P, P, P, 1 << 20, None]


def _score(**kw):
    idx = dict(x=0, N=1, D=2, K=3, pack=4, logp=5, resp=6, sum=7, ws=8, ws_bytes=9)
    args = list(SCORE_OK)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return lib.vmp_mix_score(*args), lib.vmp_last_error()


@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=9), DIM, b'D=9'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(x=None), BADARG, b'x'),
    (dict(pack=None), BADARG, b'pack'),
    (dict(logp=None, resp=None, sum=None), BADARG, b'no output'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(N=0), BADARG, b'N'),
    (dict(N=-3), BADARG, b'N'),
])
def test_score_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _score(**kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mix_score' in msg and word in msg, (kw, msg)


def test_score_workspace_is_only_needed_for_the_sum():
    """without sum_out a NULL workspace passes the host checks: what is refused next is the dimension (nothing launched)"""
    rc, msg = _score(sum=None, ws=None, ws_bytes=0, D=9)
    assert rc == DIM, (rc, msg)
    need = _lib().vmp_mix_score_workspace_bytes(10 ** 6, 8, 16)
    rc, msg = _score(N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)


@pytest.mark.parametrize('name,nptr', [('vmp_mix_score_pack_niw', 6), ('vmp_mix_score_pack_t', 5)])
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
    x = torch.zeros(N, D)
    al, be, m, C, v = _theta(K, D)
    kap = torch.full((K,), 5.0)
    bad_gmm = [(torch.zeros(N, D + 1), al, be, m, C, v), (x, al[:3], be, m, C, v), (x, al, be[:3], m, C, v),
               (x, al, be, torch.zeros(K, D + 1), C, v), (x, al, be, m, C[:, :2], v), (x, al, be, m, C[:3], v),
               (x, al, be, m, C, v[:, None]), (torch.zeros(N), al, be, m, C, v)]
    for args in bad_gmm:
        with pytest.raises(E, match='shape|must be'):
            gmm.predictive_logprob(*args)
    for args in bad_gmm:
        with pytest.raises(E, match='shape|must be'):
            smm.heldout_logprob(*args, kap)
    with pytest.raises(E, match='kappa_k has shape'):
        smm.heldout_logprob(x, al, be, m, C, v, kap[:2])
    log_pi = torch.zeros(K)
    for args in ((torch.zeros(N, D + 1), m, C, v, log_pi), (x, m, C[:3], v, log_pi), (x, m, C, v[:2], log_pi), (x, m, C, v, log_pi[:1]),
                 (x, m, torch.zeros(K, D, D + 1), v, log_pi)):
        with pytest.raises(E, match='shape|must be'):
            student_t.mixture_logprob(*args)
    with pytest.raises(E, match='compiled range'):
        gmm.predictive_logprob(torch.zeros(N, 9), *_theta(K, 9))
    with pytest.raises(E, match='compiled range'):
        gmm.predictive_logprob(x, *_theta(65, D))


def test_wrappers_have_no_cpu_fallback():
    """well-formed CPU operands: refused by the operand check (VmpError), not evaluated in torch"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import gmm, smm
    al, be, m, C, v = _theta(4, 3)
    x = torch.zeros(7, 3)
    with pytest.raises(V._lib.VmpError, match='cpu'):
        gmm.predictive_logprob(x, al, be, m, C, v)
    with pytest.raises(V._lib.VmpError, match='cpu'):
        smm.heldout_logprob(x, al, be, m, C, v, torch.full((4,), 5.0))
    with pytest.raises(V._lib.VmpError, match='cpu'):
        student_t.mixture_logprob(x, m, C, v, torch.zeros(4))


def test_loop_has_score_and_run_until():
    from vmp_for_svae_amd.models import _mix, parallel_mix
    for cls in (_mix.VMPLoop, parallel_mix.DistributedVMPLoop):
        assert callable(getattr(cls, 'score')) and callable(getattr(cls, 'run_until'))
    assert parallel_mix.DistributedVMPLoop.score is _mix.VMPLoop.score            # inherited: local rows, no collective
    assert 'no collective' in parallel_mix.DistributedVMPLoop.__doc__


def test_score_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..8 x 1..4 component tiles), the two pack builders and the sum: private
    segment size 0 in the shipped code object (DESIGN.md section 6 lists the register counts)"""
    import subprocess
    import sys
    import tempfile
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
        for m in re.finditer(r'\.name:\s+(\S*score_(?:kernel|pack_niw_kernel|pack_t_kernel|sum_kernel)\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 8 * 4 + 8 + 8 + 1, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
