"""Resources of the fixed-base comb kernel and the variable-base ladder, read from the code-object metadata of the
built ed25519.o -- no GPU needed: no scratch and three waves per SIMD (<= 170 registers) for the comb, the window
loop's budget and scratch unchanged by its signed table loads."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "kyber_amd", "csrc", "ed25519.o")
LLVM = "/opt/rocm/lib/llvm/bin"


def _kernels():
    """{kernel symbol: (total VGPRs, private segment bytes per lane)} of the gfx950 code object in ed25519.o"""
    if not os.path.exists(OBJ):
        pytest.skip("ed25519.o not built (python -c 'import __graft_entry__ as g; g.build()')")
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "ed25519.o")
        shutil.copy(OBJ, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        cos = glob.glob(os.path.join(tmp, "*gfx950*"))
        assert cos, "no gfx950 code object in ed25519.o"
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", cos[0]], check=True,
                               capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return out


def _find(table, part):
    hits = [v for k, v in table.items() if part in k]
    assert len(hits) == 1, (part, sorted(table))
    return hits[0]


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_comb_and_window_kernels_resources():
    k = _kernels()
    for g in (2, 4):  # the radix-256 table's instance and the wide comb's
        vgpr, scratch = _find(k, "23ed25519_mul_base_kernelILi%dE" % g)
        assert vgpr <= 170 and scratch == 0, (g, vgpr, scratch)
    vgpr, scratch = _find(k, "ed25519_mul_kernelILb1ELb0E")  # the headline's variable-base ladder
    assert vgpr <= 170 and scratch <= 572, (vgpr, scratch)
