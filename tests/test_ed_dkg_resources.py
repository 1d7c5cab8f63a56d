"""Resources of the kernels of ed25519_dkg.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_shuffle_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernels -- the two ECIES point passes, the commitment decoder and the deal check -- declare three waves per
    SIMD (at most 170 registers), keep their scratch below ONE window table (1 280 B: the ladder's table lives in the
    global slab, the deal kernels have none) and use no LDS;
  * the two encoders declare two waves per SIMD (256 registers) and keep the ENC_CHUNK = 16 prefix products of the shared
    inversion in scratch (640 B, plus at most a few spilled words), no LDS;
  * the two AEAD kernels declare two waves per SIMD; their LDS is what the layout says: the S-box (256 B) and 60
    round-key words for each of the block's 64 lanes, 15 616 B; round keys in LDS mean none in scratch: below 256 B;
  * the unit holds exactly the eight kernels DESIGN.md section 5 item 63 lists, and the other Ed25519 units gained none."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_dkg.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")

LANE = ("25ed25519_ecies_seal_kernel", "25ed25519_ecies_open_kernel", "26ed25519_deal_decode_kernel", "25ed25519_deal_check_kernel")
ENCODERS = ("27ed25519_ecies_encode_kernelILi1E", "27ed25519_ecies_encode_kernelILi2E")
AEAD = ("30ed25519_ecies_seal_aead_kernel", "30ed25519_ecies_open_aead_kernel")
AEAD_LDS = 256 + 60 * 64 * 4


def _kernels():
    assert os.path.exists(OBJ), "ed25519_dkg.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_dkg_kernels_keep_their_budgets():
    k = _kernels()
    assert len(k) == 8, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in LANE:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    for name in ENCODERS:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (name, vgpr, scratch, lds)
    for name in AEAD:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 256 and scratch < 256 and lds == AEAD_LDS == 15616, (name, vgpr, scratch, lds)


def test_the_unit_holds_exactly_the_kernels_design_lists():
    """DESIGN.md section 5 item 63 names the unit's kernels one by one; the code object holds those and no other"""
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("63. **`encrypt/ecies`"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The unit's eight kernels:"):]
    listed = set(re.findall(r"`(ed25519_\w+_kernel(?:<\d>)?)`", listed[:listed.index(".\n")]))
    assert len(listed) == 8, sorted(listed)
    src = open(os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_dkg.hip")).read()
    assert set(re.findall(r"void (ed25519_\w+_kernel)\(", src)) == {name.split("<")[0] for name in listed}
    if os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        built = set()
        for mangled in _kernels():  # _ZN3kyb<len><name>[ILi<k>EE]...
            m = re.match(r"_ZN3kyb\d+(ed25519_\w+?_kernel)(?:ILi(\d)E)?", mangled)
            built.add(m.group(1) + ("<%s>" % m.group(2) if m.group(2) else ""))
        assert built == listed, built ^ listed
    for name in ("15 616 B", "ED_SLAB_ECIES_SEAL", "ED_SLAB_ECIES_OPEN"):
        assert name in item, name


# kernels of the other Ed25519 units as they stand: this feature adds none to them
OTHER_UNITS = R.kernel_counts("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o", "ed25519_ring.o", "ed25519_shuffle.o")


@needs_llvm
def test_the_other_ed25519_units_gained_no_kernel():
    for unit, count in OTHER_UNITS.items():
        names = _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit))
        assert len(names) == count, (unit, len(names))
        assert not any("ecies" in name or "deal" in name or "aead" in name for name in names), unit
