"""Resources of the kernels of ed25519_shuffle.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_dleq_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernels -- the theta program and the two passes that compute a candidate draw per lane -- stay within 170
    registers (three waves per SIMD, what the theta kernel declares), keep their scratch below ONE window table
    (1 280 B: the theta kernel's two tables live in the global slab) and use no LDS;
  * the verdict encoder declares two waves per SIMD (256 registers) and keeps the ENC_CHUNK = 16 prefix products of the
    shared inversion in scratch (640 B, plus at most a few spilled words), no LDS;
  * the scan is one workgroup of 256 lanes with one word of LDS per lane;
  * the unit holds exactly these five kernels, and the other Ed25519 units gained none."""
import os

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_shuffle.o")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")


def _kernels():
    assert os.path.exists(OBJ), "ed25519_shuffle.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@needs_llvm
def test_shuffle_kernels_keep_their_budgets_and_their_tables_out_of_scratch():
    k = _kernels()
    assert len(k) == 5, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in ("20ed25519_theta_kernel", "24ed25519_xof_count_kernel", "26ed25519_xof_scatter_kernel"):
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    vgpr, scratch, lds = find("27ed25519_theta_encode_kernel")
    assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (vgpr, scratch, lds)
    vgpr, scratch, lds = find("23ed25519_xof_scan_kernel")
    assert vgpr <= 128 and scratch == 0 and lds == 256 * 4, (vgpr, scratch, lds)


@needs_llvm
def test_the_other_ed25519_units_gained_no_kernel():
    for unit in ("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o", "ed25519_ring.o"):
        names = _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit))
        assert names and not any("theta" in name or "xof" in name for name in names), unit
