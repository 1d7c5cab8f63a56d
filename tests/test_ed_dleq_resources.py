"""Resources of the kernels of ed25519_dleq.o, read from the code-object metadata -- no GPU needed.  As in
tests/test_ed_verify_resources.py the bounds come from the budgets the kernels declare and from the sizes of the data they
may keep in scratch, not from what the compiler happened to give:
  * the lane kernels (the two-sided verify program with the hash inlined, and the challenge kernel) declare
    __launch_bounds__(128, 3): three waves per SIMD, at most 170 registers (512 / 3);
  * the verify kernel's two window tables live in the global slab, so its scratch must stay below ONE window table
    (1 280 B): spills and the two digit arrays only;
  * the encoder declares two waves per SIMD (256 registers) and keeps the ENC_CHUNK = 16 prefix products of the shared
    inversion in scratch (640 B); it parks two points per proof, hence at most 2 x 640 + 64 B;
  * no kernel uses LDS, and the unit holds exactly these three kernels: ed25519.o and ed25519_verify.o gained none."""
import os

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_dleq.o")


def _kernels():
    assert os.path.exists(OBJ), "ed25519_dleq.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(os.path.basename(OBJ))


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_dleq_kernels_keep_their_budgets_and_their_tables_out_of_scratch():
    k = _kernels()
    assert len(k) == 3, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in ("19ed25519_dleq_kernel", "29ed25519_dleq_challenge_kernel"):
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    vgpr, scratch, lds = find("26ed25519_dleq_encode_kernel")
    assert vgpr <= 256 and scratch <= 2 * 640 + 64 and lds == 0, (vgpr, scratch, lds)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_the_other_ed25519_units_gained_no_kernel():
    for unit in ("ed25519.o", "ed25519_verify.o"):
        assert not any("dleq" in name for name in _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit)))
