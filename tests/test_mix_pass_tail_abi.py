"""The K == 16 instances of the XDL mixture pass that run a wave's last rows as an overlapping whole tile
(pass_xdl_overlap_kernel, csrc/vmp_mix.hip) hold no general form: the D = 8 instances - E-only, and fused with 2- and 3-term moment
operands, both flavours - must stay without a private segment and under the register count of the general instances beside
them (pass_xdl_kernel: 135 / 141 E-only, 239 / 249 / 255 fused).  Read from the built library's code-object notes; no device."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _notes(pattern):
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
        for m in re.finditer(r'\.name:\s+(\S*' + pattern + r'\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return seen


def test_overlap_instances_are_leaner_than_the_general_ones():
    new = _notes(r'pass_xdl_overlap_kernelILi8ELi[01]ELb[01]ELi[23]E')
    gen = _notes(r'pass_xdl_kernelILi8ELi[01]ELb[01]ELi[23]E')
    assert len(new) == 6 and len(gen) == 6, (sorted(new), sorted(gen))
    for name, (scratch, vgprs) in new.items():
        twin = name.replace('pass_xdl_overlap_kernel', 'pass_xdl_kernel').replace('_123', '_115')      # length prefix of the mangled name
        assert twin in gen, (name, sorted(gen))
        assert scratch == 0, (name, scratch)
        assert vgprs <= gen[twin][1], (name, vgprs, gen[twin])
