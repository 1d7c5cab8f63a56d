"""Resources of the kernels of ed25519_proof.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_dkg_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernel declares three waves per SIMD (at most 170 registers), keeps its scratch below ONE window table
    (1 280 B: its tables live in the global slab and in the call's workspace, its digits are parked) and uses no LDS;
  * the encoder and the challenge kernel declare two waves per SIMD (256 registers); the encoder keeps the ENC_CHUNK = 16
    prefix products of the shared inversion in scratch (640 B, plus at most a few spilled words); the challenge kernel
    keeps no table at all: below 1 280 B; neither uses LDS;
  * the table kernel runs ks <= 4 lanes once per call and declares a block of 64 alone;
  * the unit holds exactly the four kernels DESIGN.md section 5 item 64 lists, and the other Ed25519 units gained none."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_proof.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")


def _kernels():
    assert os.path.exists(OBJ), "ed25519_proof.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_proof_kernels_keep_their_budgets():
    k = _kernels()
    assert len(k) == 4, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    vgpr, scratch, lds = find("22ed25519_lincomb_kernel")
    assert vgpr <= 170 and scratch < 1280 and lds == 0, (vgpr, scratch, lds)
    vgpr, scratch, lds = find("29ed25519_lincomb_encode_kernel")
    assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (vgpr, scratch, lds)
    vgpr, scratch, lds = find("27ed25519_fs_challenge_kernel")
    assert vgpr <= 256 and scratch < 1280 and lds == 0, (vgpr, scratch, lds)
    vgpr, scratch, lds = find("29ed25519_lincomb_tables_kernel")
    assert vgpr <= 512 and lds == 0, (vgpr, scratch, lds)


def test_the_unit_holds_exactly_the_kernels_design_lists():
    """DESIGN.md section 5 item 64 names the unit's kernels one by one; the code object holds those and no other"""
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("64. **`proof/proof.go`"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The unit's four kernels:"):]
    listed = set(re.findall(r"`(ed25519_\w+_kernel)`", listed[:listed.index(".\n")]))
    assert len(listed) == 4, sorted(listed)
    src = open(os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_proof.hip")).read()
    assert set(re.findall(r"void (ed25519_\w+_kernel)\(", src)) == listed
    assert "__launch_bounds__(128, 3) void ed25519_lincomb_kernel(" in src  # the budget the test above holds it to
    if os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        built = {re.match(r"_ZN3kyb\d+(ed25519_\w+?_kernel)E", mangled).group(1) for mangled in _kernels()}
        assert built == listed, built ^ listed
    for name in ("ed_slab_lincomb", "WS_ED_PROOF"):
        assert name in item, name


# kernels of the other Ed25519 units as they stand: this feature adds none to them
OTHER_UNITS = R.kernel_counts("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o", "ed25519_ring.o", "ed25519_shuffle.o", "ed25519_dkg.o")


@needs_llvm
def test_the_other_ed25519_units_gained_no_kernel():
    for unit, count in OTHER_UNITS.items():
        names = _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit))
        assert len(names) == count, (unit, len(names))
        assert not any("lincomb" in name or "fs_challenge" in name for name in names), unit
