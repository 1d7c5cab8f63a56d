"""Resources of the kernels of ed25519_vss.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_dkg_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernels -- the two Schnorr passes, the seal's and the open's point passes, the decoder and Rabin's share
    check -- declare three waves per SIMD (at most 170 registers), keep their scratch below ONE window table (1 280 B: the
    ladders' tables live in the global slab or in the workspace) and use no LDS;
  * the three encoders declare two waves per SIMD (256 registers) and keep the ENC_CHUNK = 16 prefix products of the
    shared inversion in scratch (640 B, plus at most a few spilled words), no LDS;
  * the two AEAD kernels declare two waves per SIMD; their LDS is what the layout says: the S-box (256 B) and 60
    round-key words for each of the block's 64 lanes, 15 616 B; round keys in LDS mean none in scratch: below 256 B;
  * the unit holds exactly the eleven kernels DESIGN.md section 5 item 66 lists, and every other Ed25519 unit has the
    kernels it had."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_vss.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")

LANE = ("29ed25519_schnorr_points_kernel", "27ed25519_schnorr_sign_kernel", "23ed25519_vss_seal_kernel", "23ed25519_vss_open_kernel",
        "30ed25519_vss_deal_decode_kernel", "30ed25519_vss_deal_check2_kernel")
ENCODERS = ("29ed25519_schnorr_encode_kernel", "25ed25519_vss_encode_kernelILi1E", "25ed25519_vss_encode_kernelILi3E")
AEAD = ("28ed25519_vss_seal_aead_kernel", "28ed25519_vss_open_aead_kernel")
AEAD_LDS = 256 + 60 * 64 * 4


def _kernels():
    assert os.path.exists(OBJ), "ed25519_vss.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_vss_kernels_keep_their_budgets():
    k = _kernels()
    assert len(k) == 11, sorted(k)
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
    """DESIGN.md section 5 item 66 names the unit's kernels one by one; the source and the code object hold those and no
    other, and no kernel of the unit is defined in a header"""
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("66. **`share/vss`"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The unit's eleven kernels:"):]
    listed = set(re.findall(r"`(ed25519_\w+_kernel(?:<\d>)?)`", listed[:listed.index(".\n")]))
    assert len(listed) == 11, sorted(listed)
    csrc = os.path.join(R.ROOT, "kyber_amd", "csrc")
    src = open(os.path.join(csrc, "ed25519_vss.hip")).read()
    assert set(re.findall(r"void (ed25519_\w+_kernel)\(", src)) == {name.split("<")[0] for name in listed}
    for header in ("ed25519_vss.cuh", "ed25519_dkg.cuh", "aes256gcm.cuh") + R.SHARED_HEADERS:
        assert "__global__" not in open(os.path.join(csrc, header)).read(), header
    assert "md_active(" not in src  # the entries stage through the one helper and do not shard over devices
    if os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        built = set()
        for mangled in _kernels():  # _ZN3kyb<len><name>[ILi<k>EE]...
            m = re.match(r"_ZN3kyb\d+(ed25519_\w+?_kernel)(?:ILi(\d)E)?", mangled)
            built.add(m.group(1) + ("<%s>" % m.group(2) if m.group(2) else ""))
        assert built == listed, built ^ listed
    for name in ("15 616 B", "ED_SLAB_SCHNORR_SIGN", "ED_SLAB_VSS_SEAL", "ED_SLAB_VSS_OPEN", "WS_ED_VSS", "global memory"):
        assert name in item, name


# kernels of the other Ed25519 units as they stand: this feature adds none to them
OTHER_UNITS = R.kernel_counts("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o", "ed25519_ring.o", "ed25519_shuffle.o",
                               "ed25519_dkg.o", "ed25519_proof.o", "ed25519_cosi.o")


@needs_llvm
def test_the_other_ed25519_units_gained_no_kernel():
    for unit, count in OTHER_UNITS.items():
        names = _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit))
        assert len(names) == count, (unit, len(names))
        assert not any("vss" in name or "schnorr" in name or "check2" in name for name in names), unit
