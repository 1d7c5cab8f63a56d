"""What the resource tests of the Ed25519 units (tests/test_ed_*_resources.py) share: one reader of a unit's code-object
metadata and one table of how many kernels each unit holds.  A kernel added to a unit changes one number, here."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.test_ed25519_comb_resources import LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kyber_amd", "csrc")

# kernels in each unit's gfx950 code object
KERNEL_COUNT = {"ed25519.o": 37, "ed25519_verify.o": 4, "ed25519_dleq.o": 3, "ed25519_ring.o": 3, "ed25519_shuffle.o": 5, "ed25519_dkg.o": 8,
                "ed25519_proof.o": 4, "ed25519_cosi.o": 7, "ed25519_vss.o": 11, "ed25519_anonenc.o": 10, "ed25519_dss.o": 9,
                "ed25519_eddsa.o": 4}

# headers the units share: none of them may define a kernel
SHARED_HEADERS = ("ed25519_dev.cuh", "ed25519_launch.h", "ed_spans.h", "aes256gcm.cuh")


def kernel_counts(*units):
    return {unit: KERNEL_COUNT[unit] for unit in units}


def kernels(unit):
    """{mangled name: (VGPRs, scratch bytes, LDS bytes)} of every kernel of kyber_amd/csrc/<unit>"""
    obj = os.path.join(CSRC, unit)
    if not os.path.exists(obj):
        pytest.skip(unit + " not built (python -c 'import __graft_entry__ as g; g.build()')")
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, unit)
        shutil.copy(obj, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", glob.glob(os.path.join(tmp, "*gfx950*"))[0]],
                               check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (g("vgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"))
    return out
