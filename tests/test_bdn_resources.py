"""Resources of the kernels of bls12381_bdn.o, bn256_bdn.o and bn254_bdn.o, read from the code-object metadata -- no GPU
needed.  As in tests/test_ed_cosi_resources.py the bounds come from the budgets the kernels declare and from the data
they may keep in scratch, not from what the compiler happened to give:
  * the BN units declare two waves per SIMD for every kernel (KYB_TU_WAVES 2, the ladders' KYB_BN_MUL_WAVES 2): at most
    256 registers; the BLS12-381 unit follows its suite's one wave per SIMD: at most 512;
  * the aggregation kernels -- tables, T_all, slices, fold, finish -- keep their tables, partial sums and trees in the
    call's workspace: their scratch holds the accumulator, one entry, the sum and the temporaries of the out-of-line
    addition, at most six points of E = 3 coordinates (no array of points, no table);
  * LDS: the root kernel's vote (256 B), the first-rejected index of the T_all kernel (4 B), and what the suite's
    standing G2 ladder keeps there under the terms kernel (2 048 B); nothing else;
  * each unit holds exactly the nine kernels DESIGN.md section 5 item 68 lists, once per group, and no other unit of
    the pairing suites gained or lost a kernel."""
import os
import re

import pytest

from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

CSRC = os.path.join(R.ROOT, "kyber_amd", "csrc")
needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
KERNELS = ("bdn_roster_kernel", "bdn_root_kernel", "bdn_terms_kernel", "bdn_points_kernel", "bdn_tables_kernel", "bdn_total_kernel",
           "bdn_slices_kernel", "bdn_fold_kernel", "bdn_finish_kernel")
# unit -> (register budget, bytes of a field element)
UNITS = {"bls12381_bdn.o": (512, 48), "bn256_bdn.o": (256, 32), "bn254_bdn.o": (256, 32)}


def _kernels(unit):
    obj = os.path.join(CSRC, unit)
    assert os.path.exists(obj), unit + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    return R.kernels(unit)


@needs_llvm
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_bdn_kernels_keep_their_budgets(unit):
    budget, fe = UNITS[unit]
    k = _kernels(unit)
    assert len(k) == 2 * len(KERNELS), sorted(k)
    for name, (vgpr, scratch, lds) in k.items():
        kernel = re.match(r"_ZN3kyb\d+(bdn_\w+?_kernel)I", name).group(1)
        assert kernel in KERNELS, name
        g2 = "2G2E" in name
        assert vgpr <= budget, (name, vgpr)
        if kernel in ("bdn_tables_kernel", "bdn_total_kernel", "bdn_slices_kernel", "bdn_fold_kernel", "bdn_finish_kernel"):
            assert scratch <= 6 * 3 * fe * (2 if g2 else 1), (name, scratch)
        want_lds = {"bdn_root_kernel": (256, 256), "bdn_total_kernel": (4, 4), "bdn_terms_kernel": (0, 2048)}.get(kernel, (0, 0))
        assert want_lds[0] <= lds <= want_lds[1], (name, lds)
    assert {re.match(r"_ZN3kyb\d+(bdn_\w+?_kernel)I", name).group(1) for name in k} == set(KERNELS)


def test_the_units_hold_exactly_the_kernels_design_lists():
    design = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    item = design[design.index("68. **`sign/bdn`"):design.index("## 6. Multi-GPU")]
    listed = item[item.index("The nine kernels"):]
    listed = set(re.findall(r"`(bdn_\w+_kernel)`", listed[:listed.index(".\n")]))
    assert listed == set(KERNELS), listed ^ set(KERNELS)
    src = open(os.path.join(CSRC, "bdn_launch.cuh")).read()
    assert set(re.findall(r"void (bdn_\w+_kernel)\(", src)) == listed
    assert len(re.findall(r"__global__ __launch_bounds__\(", src)) == len(KERNELS)  # every kernel declares its block
    for name in ("WS_BDN", "BDN_FILL", "bdn_plan", "kyb_bdn_debug_set_slices", "not measured"):
        assert name in item, name


# kernels of the pairing suites' other units as they stand: this feature adds none to them
OTHER_UNITS = {"bls12381.o": 18, "bls12381_fb.o": 11, "bls12381_g1split.o": 2, "bls12381_h2c.o": 2, "bls12381_ibe.o": 5, "bls12381_msm.o": 50,
               "bls12381_msm_gls.o": 29, "bls12381_msm_plain.o": 31, "bls12381_pair.o": 7, "bls12381_prep.o": 2, "bls12381_unm2.o": 4,
               "bn254.o": 17, "bn254_msm.o": 48, "bn254_msm_glv.o": 29, "bn254_pair.o": 6, "bn256.o": 21, "bn256_msm.o": 48,
               "bn256_msm_glv.o": 29, "bn256_pair.o": 7, **R.kernel_counts("ed25519_cosi.o")}


@needs_llvm
def test_the_other_units_gained_no_kernel():
    for unit, count in OTHER_UNITS.items():
        names = _kernel_regs(os.path.join(CSRC, unit))
        assert len(names) == count, (unit, len(names))
        assert not any("bdn" in name for name in names), unit
