"""Host side of the fused mixture pass without its r / u stores (include/vmp_hip.h: vmp_mixture_estep_fused_nostore,
vmp_mixture_iterate_nostore; csrc/vmp_mix.hip).  No device: every call below is refused before a launch, and the kernels are read from
the built library's code-object notes.
- both symbols are exported and their prototypes are in the ctypes table, argument for argument what vmp_mix_estep_fused and
  vmp_mix_iterate take without r_out, u_out and logr_out (tests/test_abi.py holds the table to the header);
- each pointer the calls need, the sizes, the flavour and the workspace size are refused with the codes of vmp_mix_estep_fused, and
  K > 16 - the tiled pass, which has no such instance - with VMP_E_NOIMPL, by the iteration before its first launch;
- the D = 8 instances (general and overlap form, both flavours, 2- and 3-term moment operands) have no private segment and fit the
  256 vector registers of two waves per SIMD; they carry names of their own, so that the patterns of tests/test_abi.py and
  tests/test_mix_pass_tail_abi.py go on matching the storing instances alone."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)                    # a non-NULL pointer that is never dereferenced: every call fails its checks first
BIG = 1 << 40
E_BADARG, E_DIM, E_WS, E_NOIMPL = -1, -2, -3, -4


def _lib():
    import vmp_for_svae_amd as V
    return V._lib


def _pass(N=100, D=8, K=16, fl=0, x=P, pack=P, pivot=P, ws=P, nb=BIG):
    return [x, N, D, K, fl, pack, pivot, ws, nb, None]


def _iterate(N=100, D=8, K=16, fl=0, x=P, kappa=P, pack=P, ws=P, nb=BIG, iterations=1, prior=None):
    return [x, N, D, K, fl] + (prior or [P] * 5) + [kappa, P] + [P] * 8 + [pack, ws, nb, iterations, None]


def test_symbols_and_prototypes():
    L = _lib()
    lib = ctypes.CDLL(L.LIB_PATH)
    sig = L._SIGNATURES
    for new, old, dropped in (('vmp_mixture_estep_fused_nostore', 'vmp_mix_estep_fused', (6, 7, 8)),
                              ('vmp_mixture_iterate_nostore', 'vmp_mix_iterate', (12, 13))):
        assert hasattr(lib, new) and new in L.exported_symbols()
        res, args = sig[new]
        ores, oargs = sig[old]
        kept = [a for i, a in enumerate(oargs) if i not in dropped]
        if new == 'vmp_mixture_estep_fused_nostore':
            assert oargs[9] is ctypes.c_void_p                  # pivot, which follows the three outputs there and the pack here
        assert res is ores and args == kept, new
    hdr = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert re.search(r'#define\s+VMP_E_NOIMPL\s+\(-4\)', hdr)


def test_pass_validates_on_the_host():
    lib = _lib().lib()
    f = lib.vmp_mixture_estep_fused_nostore
    for kw, code in ((dict(x=None), E_BADARG), (dict(pack=None), E_BADARG), (dict(ws=None), E_BADARG), (dict(fl=2), E_BADARG),
                     (dict(N=0), E_BADARG), (dict(D=0), E_DIM), (dict(D=9), E_DIM), (dict(K=0), E_DIM), (dict(K=65), E_DIM),
                     (dict(nb=8), E_WS), (dict(K=17), E_NOIMPL), (dict(K=64, fl=1), E_NOIMPL)):
        assert f(*_pass(**kw)) == code, kw
        msg = lib.vmp_last_error()
        # the size checks (N, D, K) and the missing instance are shared with the other passes; the rest names the entry point
        assert msg and (set(kw) & {'N', 'D', 'K'} or b'vmp_mixture_estep_fused_nostore' in msg), (kw, msg)
    assert f(*_pass(K=17)) == E_NOIMPL and b'K = 17' in lib.vmp_last_error()
    # the pivot is optional, as for vmp_mix_estep_fused: with it NULL the call gets to the size check behind the pointer checks
    assert f(*_pass(pivot=None, nb=8)) == E_WS


def test_iteration_refuses_before_its_first_launch():
    lib = _lib().lib()
    f = lib.vmp_mixture_iterate_nostore
    for kw, code in ((dict(pack=None), E_BADARG), (dict(iterations=-1), E_BADARG), (dict(x=None), E_BADARG), (dict(ws=None), E_BADARG),
                     (dict(fl=3), E_BADARG), (dict(N=0), E_BADARG), (dict(D=9), E_DIM), (dict(K=65), E_DIM), (dict(nb=8), E_WS),
                     (dict(K=17), E_NOIMPL), (dict(K=33, fl=1), E_NOIMPL)):
        assert f(*_iterate(**kw)) == code, kw
        assert lib.vmp_last_error()
    # what the first launch's entry point refuses (a NULL prior, the SMM's kappa) comes back from it, as from vmp_mix_iterate
    assert f(*_iterate(prior=[None] + [P] * 4)) == E_BADARG and b'vmp_mix_finalize_ws' in lib.vmp_last_error()
    assert f(*_iterate(fl=1, kappa=None)) == E_BADARG and b'kappa' in lib.vmp_last_error()
    assert f(*_iterate(iterations=0)) == 0                    # nothing to enqueue


def _notes(pattern):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    readelf = E.OBJDUMP.replace('llvm-objdump', 'llvm-readelf')
    assert os.path.exists(readelf), 'llvm-readelf not found at %s: the private segments cannot be read' % readelf
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S*' + pattern + r'\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return seen


@pytest.mark.parametrize('new,old', [('pass_xdl_nostore_kernel', 'pass_xdl_kernel'), ('pass_xdl_overlap_nostore_kernel', 'pass_xdl_overlap_kernel')])
def test_d8_instances_fit_their_registers(new, old):
    got = _notes(new + r'ILi8ELi[01]ELi[23]E')
    ref = _notes(old + r'ILi8ELi[01]ELb1ELi[23]E')
    assert len(got) == 4 and len(ref) == 4, (sorted(got), sorted(ref))
    for name, (scratch, vgprs) in got.items():
        assert scratch == 0, (name, scratch)
        assert vgprs <= 256, (name, vgprs)                       # two waves per SIMD, as the storing instances run
