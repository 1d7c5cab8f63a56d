"""Resources of the kernels of ed25519_verify.o, read from the code-object metadata -- no GPU needed.  Bounds come from
the budgets the kernels declare and from the sizes of the data they are allowed to keep in scratch, not from what the
compiler happened to give:
  * the two lane programs declare __launch_bounds__(128, 3): three waves per SIMD, at most 170 registers
    (512 / 3, the bound tests/test_kernel_resources.py pins for the ladder they share);
  * their window tables live in the global slab, so their scratch must stay below ONE window table (1 280 B): spills
    and the digit arrays only;
  * the encoders declare two waves per SIMD (256 registers) and keep the ENC_CHUNK = 16 prefix products of the shared
    inversion (16 x 40 B = 640 B) in scratch like ed25519_encode_kernel, plus at most a few spilled words (<= 64 B);
  * no kernel of the unit is without a budget: none may exceed 256 registers, none uses LDS."""
import os

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_new_kernels_keep_their_budgets_and_their_tables_out_of_scratch():
    k = R.kernels("ed25519_verify.o")
    assert len(k) == 4, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in ("21ed25519_verify_kernel", "19ed25519_mul2_kernel"):
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    for name in ("ed25519_verify_encode_kernel", "ed25519_mul2_encode_kernel"):
        vgpr, scratch, lds = find(name)
        assert vgpr <= 256 and scratch <= 640 + 64 and lds == 0, (name, vgpr, scratch, lds)
    assert all(v[0] <= 256 for v in k.values())


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_the_tuned_kernels_of_ed25519_o_did_not_move():
    """the reason the new kernels have a unit of their own: ed25519.o's ladders and combs at three waves per SIMD"""
    ed = _kernel_regs(os.path.join(R.CSRC, "ed25519.o"))
    assert not any("verify" in name or "mul2" in name for name in ed)
    for part in ("ed25519_mul_kernelILb1ELb0E", "ed25519_mul_kernelILb0ELb0E", "23ed25519_mul_base_kernelILi4E"):
        assert [v for name, v in ed.items() if part in name][0] <= 170, part
