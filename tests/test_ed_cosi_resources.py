"""Resources of the kernels of ed25519_cosi.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_proof_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the aggregate and the check kernel declare three waves per SIMD (at most 170 registers); their tables live in the
    call's workspace and in the global slab, so their scratch stays below ONE window table (1 280 B); no LDS;
  * the two encode passes declare two waves per SIMD (256 registers) and keep the ENC_CHUNK = 16 prefix products of the
    shared inversion in scratch (640 B, plus at most a few spilled words); no LDS;
  * the roster kernel declares a block of 64 alone, the table kernel a block of 256 (at most 256 registers for one
    wave per SIMD and block) without LDS, the T_all kernel a block of 256 whose tree hands 40 words a lane through LDS:
    40 960 B, and the 256 B of the block's vote;
  * the unit holds exactly the seven kernels DESIGN.md section 5 item 65 lists, and the other Ed25519 units gained none."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_cosi.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")


def _kernels():
    assert os.path.exists(OBJ), "ed25519_cosi.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_cosi_kernels_keep_their_budgets():
    k = _kernels()
    assert len(k) == 7, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for lane in ("29ed25519_cosi_aggregate_kernel", "25ed25519_cosi_check_kernel"):
        vgpr, scratch, lds = find(lane)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (lane, vgpr, scratch, lds)
    for enc in ("26ed25519_cosi_encode_kernel", "27ed25519_cosi_verdict_kernel"):
        vgpr, scratch, lds = find(enc)
        assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (enc, vgpr, scratch, lds)
    vgpr, scratch, lds = find("26ed25519_cosi_roster_kernel")
    assert vgpr <= 512 and scratch < 1280 and lds == 0, (vgpr, scratch, lds)
    vgpr, scratch, lds = find("26ed25519_cosi_tables_kernel")
    assert vgpr <= 256 and scratch < 1280 and lds == 0, (vgpr, scratch, lds)
    vgpr, scratch, lds = find("25ed25519_cosi_total_kernel")
    assert vgpr <= 256 and scratch < 1280 and 40 * 256 * 4 <= lds <= 40 * 256 * 4 + 256, (vgpr, scratch, lds)


def test_the_unit_holds_exactly_the_kernels_design_lists():
    """DESIGN.md section 5 item 65 names the unit's kernels one by one; the code object holds those and no other"""
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("65. **`sign/cosi`"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The unit's seven kernels:"):]
    listed = set(re.findall(r"`(ed25519_\w+_kernel)`", listed[:listed.index(".\n")]))
    assert len(listed) == 7, sorted(listed)
    src = open(os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_cosi.hip")).read()
    assert set(re.findall(r"void (ed25519_\w+_kernel)\(", src)) == listed
    for budget in ("__launch_bounds__(128, 3) void ed25519_cosi_aggregate_kernel(", "__launch_bounds__(128, 3) void ed25519_cosi_check_kernel("):
        assert budget in src  # the budgets the test above holds them to
    assert len(re.findall(r"__global__ __launch_bounds__\(", src)) == 7  # every kernel declares its block
    if os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        built = {re.match(r"_ZN3kyb\d+(ed25519_\w+?_kernel)E", mangled).group(1) for mangled in _kernels()}
        assert built == listed, built ^ listed
    for name in ("ED_SLAB_COSI_VERIFY", "ED_SLAB_COSI_AGGREGATE", "WS_ED_COSI", "ed_cosi_group_width", "not been measured"):
        assert name in item, name


# kernels of the other Ed25519 units as they stand: this feature adds none to them
OTHER_UNITS = R.kernel_counts("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o", "ed25519_ring.o",
                               "ed25519_shuffle.o", "ed25519_dkg.o", "ed25519_proof.o")


@needs_llvm
def test_the_other_ed25519_units_gained_no_kernel():
    for unit, count in OTHER_UNITS.items():
        names = _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit))
        assert len(names) == count, (unit, len(names))
        assert not any("cosi" in name for name in names), unit
