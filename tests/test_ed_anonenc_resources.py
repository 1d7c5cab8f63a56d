"""Resources of the kernels of ed25519_anonenc.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_vss_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernels -- the shared set's tables, the two heads, the two product passes -- declare three waves per SIMD
    (at most 170 registers), keep their scratch below ONE window table (1 280 B: the ladders' tables live in the global
    slab or in the workspace) and use no LDS;
  * the encoder declares two waves per SIMD (256 registers) and keeps the ENC_CHUNK = 16 prefix products of the shared
    inversion in scratch (640 B, plus at most a few spilled words), no LDS;
  * the slot and body passes declare two waves per SIMD; they keep no array in scratch, so what is there is spilled hash
    state: at most one message block (128 B), one chaining value (64 B) and one work vector (128 B), 320 B; no LDS;
  * the unit holds exactly the ten kernels DESIGN.md section 5 item 67 lists, none defined in a header, and the source
    does not shard over a device set."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_anonenc.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")

LANE = ("26ed25519_anon_tables_kernel", "29ed25519_anon_seal_head_kernel", "29ed25519_anon_open_head_kernel",
        "26ed25519_anon_points_kernelILb0E", "26ed25519_anon_points_kernelILb1E")
ENCODERS = ("26ed25519_anon_encode_kernel",)
HASH = ("24ed25519_anon_slot_kernelILb0E", "24ed25519_anon_slot_kernelILb1E", "24ed25519_anon_body_kernelILb0E",
        "24ed25519_anon_body_kernelILb1E")


def _kernels():
    assert os.path.exists(OBJ), "ed25519_anonenc.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_anonenc_kernels_keep_their_budgets():
    k = _kernels()
    assert len(k) == 10, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in LANE:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    for name in ENCODERS:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (name, vgpr, scratch, lds)
    for name in HASH:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 256 and scratch <= 128 + 64 + 128 and lds == 0, (name, vgpr, scratch, lds)


def test_the_unit_holds_exactly_the_kernels_design_lists():
    """DESIGN.md section 5 item 67 names the unit's kernels one by one; the source and the code object hold those and no
    other, and no kernel of the unit is defined in a header"""
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("67. **`sign/anon` Encrypt"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The unit's ten kernels:"):]
    listed = set(re.findall(r"`(ed25519_\w+_kernel(?:<\w+>)?)`", listed[:listed.index(".\n")]))
    assert len(listed) == 10, sorted(listed)
    csrc = os.path.join(R.ROOT, "kyber_amd", "csrc")
    src = open(os.path.join(csrc, "ed25519_anonenc.hip")).read()
    assert set(re.findall(r"void (ed25519_\w+_kernel)\(", src)) == {name.split("<")[0] for name in listed}
    for header in ("ed25519_anonenc.cuh", "ed25519_ring.cuh", "ed25519_dkg.cuh", "blake2xb.cuh") + R.SHARED_HEADERS:
        assert "__global__" not in open(os.path.join(csrc, header)).read(), header
    assert "md_active(" not in src  # the entries stage through the one helper and do not shard over devices
    if os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        built = set()
        for mangled in _kernels():  # _ZN3kyb<len><name>[ILb<k>EE]...
            m = re.match(r"_ZN3kyb\d+(ed25519_\w+?_kernel)(?:ILb(\d)E)?", mangled)
            built.add(m.group(1) + ("<%s>" % ("true" if m.group(2) == "1" else "false") if m.group(2) else ""))
        assert built == listed, built ^ listed
    for name in ("ed_slab_anon", "ed_anon_piece", "WS_ED_ANON", "KYB_ANON_MAX_RING", "global memory", "Not done"):
        assert name in item, name
