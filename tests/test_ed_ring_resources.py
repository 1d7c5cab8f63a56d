"""Resources of the kernels of ed25519_ring.o, read from the code-object metadata, and the C ABI's argument checks of
the ring entry points -- no GPU needed.  The bounds come from the budgets the kernels declare:
  * the chain and the challenge kernel declare __launch_bounds__(128, 3): three waves per SIMD, at most 170 registers;
  * every window table lives in global memory (the call's shared tables, the lane's slab), so scratch must stay below
    ONE window table (1 280 B): spills and the two digit arrays only;
  * the table builder declares blocks of 64 lanes and no occupancy: the whole register file of a SIMD lane (512);
  * no kernel uses LDS, the unit holds exactly these three kernels, and the other Ed25519 units gained none."""
import ctypes as C
import os

import pytest

from kyber_amd import _lib
from tests import _ed_units as R
from tests.test_ed25519_comb_resources import LLVM
from tests.test_kernel_resources import _kernel_regs

OBJ = os.path.join(R.ROOT, "kyber_amd", "csrc", "ed25519_ring.o")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_ring_kernels_keep_their_budgets_and_their_tables_out_of_scratch():
    assert os.path.exists(OBJ), "ed25519_ring.o not built (python -c 'import __graft_entry__ as g; g.build()')"
    k = R.kernels(os.path.basename(OBJ))
    assert len(k) == 3, sorted(k)
    find = lambda part: [v for name, v in k.items() if part in name][0]
    for name in ("25ed25519_ring_chain_kernel", "29ed25519_ring_challenge_kernel"):
        vgpr, scratch, lds = find(name)
        assert vgpr <= 170 and scratch < 1280 and lds == 0, (name, vgpr, scratch, lds)
    vgpr, scratch, lds = find("26ed25519_ring_tables_kernel")
    assert vgpr <= 512 and scratch < 1280 and lds == 0, (vgpr, scratch, lds)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no llvm-readelf")
def test_the_other_ed25519_units_gained_no_kernel():
    for unit in ("ed25519.o", "ed25519_verify.o", "ed25519_dleq.o"):
        assert not any("ring" in name for name in _kernel_regs(os.path.join(R.ROOT, "kyber_amd", "csrc", unit)))


def test_argument_errors_and_empty_batches_never_touch_a_device():
    lib = _lib.load()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    off = (C.c_uint64 * 2)(0, 0)
    o = C.cast(off, C.c_void_p)

    def chain(n=1, ring=3, key_stride=0, scope=None, base=None, sig_stride=None, flags=0, host=True):
        ss = 32 * (ring + (2 if scope else 1)) if sig_stride is None else sig_stride
        args = [n, ring, p, key_stride, p, o, scope, 5 if scope else 0, base, p, ss, None, ring, p, p, p, p, flags]
        return lib.kyb_ed25519_ring_chain(*args) if host else lib.kyb_ed25519_ring_chain_dev(*args, None)

    for host in (True, False):
        assert chain(ring=0, host=host) == -1
        assert chain(key_stride=32, host=host) == -1 and chain(key_stride=64, host=host) == -1
        assert chain(sig_stride=32 * 5, host=host) == -1 and chain(sig_stride=32 * 3, host=host) == -1
        assert chain(scope=p, base=p, sig_stride=32 * 4, host=host) == -1
        assert chain(scope=p, host=host) == -1 and chain(base=p, host=host) == -1
        assert chain(flags=_lib.KYB_F_UNIFORM, host=host) == -1 and chain(flags=2, host=host) == -1
        assert chain(flags=_lib.KYB_F_UNIFORM | _lib.KYB_F_VARTIME, host=host) == -1
        assert chain(n=0, host=host) == 0 and chain(n=0, key_stride=96, scope=p, base=p, flags=1, host=host) == 0
        assert chain(n=0, ring=0, host=host) == -1
    assert b"bad argument" in lib.kyb_last_error()
    bad_start = (C.c_uint32 * 1)(3)
    assert lib.kyb_ed25519_ring_chain(1, 3, p, 0, p, o, None, 0, None, p, 128, C.cast(bad_start, C.c_void_p), 2, p, p, p, p, 0) == -1
    down = (C.c_uint64 * 2)(4, 0)
    assert lib.kyb_ed25519_ring_chain(1, 3, p, 0, p, C.cast(down, C.c_void_p), None, 0, None, p, 128, None, 3, p, p, p, p, 0) == -1
    assert lib.kyb_ed25519_ring_challenge(0, None, None, None, 0, None, None, None, None, None) == 0
    assert lib.kyb_ed25519_ring_challenge(1, p, o, None, 0, p, p, None, p, None) == -1   # a tag without a scope
    assert lib.kyb_ed25519_ring_challenge(1, p, o, p, 4, None, p, p, p, None) == -1      # a scope without a tag
    assert lib.kyb_ed25519_ring_challenge(1, p, o, None, 0, None, None, None, p, None) == -1
    assert lib.kyb_ed25519_ring_challenge(1, p, C.cast(down, C.c_void_p), None, 0, None, p, None, p, None) == -1
    assert lib.kyb_ed25519_ring_challenge_dev(1, p, o, None, 0, None, p, p, p, None, None) == -1
