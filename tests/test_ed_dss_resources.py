"""Resources of the kernels of ed25519_dss.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_vss_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernels -- the session pass, the fold, its decoder, the signature pass, the share pass and the two passes of
    PartialSig -- declare three waves per SIMD (at most 170 registers), keep their scratch below ONE window table
    (1 280 B: the ladders' tables live in the global slab) and use no LDS;
  * the two encoders declare two waves per SIMD (256 registers) and keep the ENC_CHUNK = 16 prefix products of the
    shared inversion in scratch (640 B, plus at most a few spilled words), no LDS;
  * the unit holds exactly the nine kernels DESIGN.md section 5 item 69 lists, none defined in a header, no md_active( site,
    and every other Ed25519 unit has the kernels its own resource test pins."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_dss.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")

LANE = ("26ed25519_dss_session_kernel", "23ed25519_dss_fold_kernel", "30ed25519_dss_fold_decode_kernel", "25ed25519_dss_verify_kernel",
        "24ed25519_dss_share_kernel", "33ed25519_dss_partial_points_kernel", "31ed25519_dss_partial_sign_kernel")
ENCODERS = ("25ed25519_dss_encode_kernel", "32ed25519_dss_verify_encode_kernel")


def _kernels():
    assert os.path.exists(OBJ), "ed25519_dss.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_dss_kernels_keep_their_budgets():
    k = _kernels()
    assert len(k) == 9, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in LANE:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    for name in ENCODERS:
        vgpr, scratch, lds = find(name)
        assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (name, vgpr, scratch, lds)


def test_the_unit_holds_exactly_the_kernels_design_lists():
    """DESIGN.md section 5 item 69 names the unit's kernels one by one; the source and the code object hold those and no
    other, and no kernel of the unit is defined in a header"""
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("69. **`sign/dss`"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The unit's nine kernels:"):]
    listed = set(re.findall(r"`(ed25519_\w+_kernel)`", listed[:listed.index(".\n")]))
    assert len(listed) == 9, sorted(listed)
    csrc = os.path.join(R.ROOT, "kyber_amd", "csrc")
    src = open(os.path.join(csrc, "ed25519_dss.hip")).read()
    assert set(re.findall(r"void (ed25519_\w+_kernel)\(", src)) == listed
    assert all(name.startswith("ed25519_dss_") for name in listed)
    for header in ("ed25519_dss.cuh", "ed25519_vss.cuh", "ed25519_dkg.cuh", "ed25519_verify.cuh") + R.SHARED_HEADERS:
        assert "__global__" not in open(os.path.join(csrc, header)).read(), header
    assert "md_active(" not in src  # the entries stage through the one helper and do not shard over devices
    assert "staged_call(" in src and "ed_for_pieces(" in src and "hipMalloc" not in src
    assert "ed25519_dss.hip" in open(os.path.join(csrc, "Makefile")).read()
    if os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        built = set()
        for mangled in _kernels():
            built.add(re.match(r"_ZN3kyb\d+(ed25519_\w+?_kernel)E", mangled).group(1))
        assert built == listed, built ^ listed
    for name in ("ED_SLAB_DSS_FOLD", "ED_SLAB_DSS_VERIFY", "ED_SLAB_DSS_PARTIAL", "WS_ED_DSS", "Not measured", "Not done"):
        assert name in item, name


# kernels of the other Ed25519 units as their own resource tests pin them: this feature adds none to them
OTHER_UNITS = R.kernel_counts("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o", "ed25519_ring.o", "ed25519_shuffle.o",
                               "ed25519_dkg.o", "ed25519_proof.o", "ed25519_cosi.o", "ed25519_vss.o")


@needs_llvm
def test_the_other_ed25519_units_gained_no_kernel():
    for unit, count in OTHER_UNITS.items():
        names = _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit))
        assert len(names) == count, (unit, len(names))
        assert not any("dss" in name for name in names), unit
