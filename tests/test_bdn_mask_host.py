"""sign/bdn's Mask without a GPU: the scenarios of mask_test.go that need no coefficient (NewMask with a key returns
before any exists, mask.go:40-49), the reference's error strings, SetMask's aliasing, the stray bits the positional
queries walk, Clone's sharing, and the refusal to aggregate with a mask that holds no terms."""
import random

import pytest

from kyber_amd.pairing import bn256
from kyber_amd.sign import bdn
from oracle import bn256 as ON

N = 17  # mask_test.go:13


@pytest.fixture(scope="module")
def publics():
    return [bn256.G1Elt(ON.g1_marshal(ON.g1_mul(1000 + 7 * i, ON.G1_GEN))) for i in range(N)]


@pytest.fixture()
def mask(publics):
    return bdn.NewMask(bn256.NewSuite().G1(), publics, publics[2])


def test_create_mask_with_a_key(publics, mask):  # TestMask_CreateMask, second half
    assert len(mask.Publics()) == N and mask.CountEnabled() == 1 and mask.CountTotal() == N and mask.Len() == N // 8 + 1
    assert mask.Mask()[0] == 0x4 and mask.publicCoefs is None and mask.publicTerms is None
    with pytest.raises(ValueError, match="key not found"):
        bdn.NewMask(bn256.NewSuite().G1(), publics, bn256.G1Elt())
    assert bdn.NewMask(bn256.NewSuite().G1(), [p.enc for p in publics], publics[5].enc).Mask()[0] == 0x20  # bytes serve too


def test_set_bit(publics, mask):  # TestMask_SetBit
    assert mask.GetBit(1) is False and mask.GetBit(2) is True
    for _ in range(2):  # setting a set bit changes nothing
        mask.SetBit(1, True)
        assert mask.Mask()[0] == 0x6 and len(mask.Participants()) == 2 and mask.GetBit(1)
    mask.SetBit(2, False)
    assert mask.Mask()[0] == 0x2 and len(mask.Participants()) == 1 and not mask.GetBit(2)
    mask.SetBit(10, True)
    assert (mask.Mask()[0], mask.Mask()[1]) == (0x2, 0x4) and len(mask.Participants()) == 2 and mask.GetBit(10)
    assert mask.Participants() == [publics[1], publics[10]]
    for i in (-1, N):
        for call in (lambda: mask.SetBit(i, True), lambda: mask.GetBit(i)):
            with pytest.raises(IndexError, match="index out of range"):
                call()


def test_set_and_merge(mask):  # TestMask_SetAndMerge
    with pytest.raises(ValueError, match="mismatching mask lengths"):
        mask.SetMask(b"")
    mask.SetMask(bytes(3))
    with pytest.raises(ValueError, match="mismatching mask length"):
        mask.Merge(b"")
    mask.Merge(bytes([0x6, 0, 0]))
    assert mask.Mask()[0] == 0x6


def test_set_mask_aliases_the_buffer_and_mask_copies(mask):
    buf = bytearray(3)
    mask.SetMask(buf)
    mask.SetBit(9, True)
    assert buf == bytearray([0, 2, 0])  # the reference keeps the caller's slice (mask.go:84)
    buf[0] = 1
    assert mask.GetBit(0)
    out = mask.Mask()
    mask.SetBit(0, False)
    assert out[0] == 1  # Mask() is a copy (mask.go:67-71)


def test_set_mask_aliases_any_writable_buffer(mask):
    import numpy as np

    arr = np.zeros(3, dtype=np.uint8)
    mask.SetMask(arr)
    mask.SetBit(9, True)
    arr[0] = 1
    assert arr[1] == 2 and mask.GetBit(0) and mask.Mask() == bytes([1, 2, 0])
    backing = bytearray(3)
    mask.SetMask(memoryview(backing))
    mask.SetBit(16, True)
    assert backing == bytearray([0, 0, 1])
    mask.Merge(bytes([4, 0, 0]))
    assert backing[0] == 4 and mask.CountEnabled() == 2
    ro = memoryview(bytes(3))
    mask.SetMask(ro)  # nothing to share with: copied
    mask.SetBit(1, True)
    assert bytes(ro) == bytes(3) and mask.GetBit(1)


def test_positional_queries_walk_stray_bits(mask):  # TestMask_PositionalQueries
    rng = random.Random(5)
    for _ in range(300):
        bb = bytearray(rng.randbytes(3))
        bb[2] &= 1 << 7  # the reference's own mask: bit 23, a STRAY bit, may be set
        mask.SetMask(bb)
        enabled = [i for i in range(24) if bb[i >> 3] >> (i & 7) & 1]
        for j in range(mask.CountEnabled()):
            idx = mask.IndexOfNthEnabled(j)
            assert mask.NthEnabledAtIndex(idx) == j and idx == enabled[j]
        assert mask.IndexOfNthEnabled(mask.CountEnabled() + 1) == -1 and mask.NthEnabledAtIndex(-1) == -1
        assert mask.CountEnabled() == sum(1 for i in enabled if i < N)  # CountEnabled loops over publics: no stray bit
        if bb[2]:
            assert mask.IndexOfNthEnabled(len(enabled) - 1) == 23  # forEachBitEnabled does reach it


def test_clone_shares_everything_but_the_bitmask(publics, mask):
    mask.publicCoefs, mask.publicTerms = [1, 2, 3], object()
    c = mask.Clone()
    c.SetBit(0, True)
    assert not mask.GetBit(0) and c.GetBit(2)
    assert c.publics is mask.publics and c.publicCoefs is mask.publicCoefs and c.publicTerms is mask.publicTerms


def test_a_mask_made_with_a_key_cannot_aggregate(mask):
    """the reference indexes nil publicTerms / publicCoefs and panics (bdn.go:150, 177)"""
    for suite_scheme in (bdn.NewSchemeOnG2(bn256), bdn.NewSchemeOnG1(bn256)):
        with pytest.raises(IndexError, match="index out of range"):
            suite_scheme.AggregatePublicKeys(mask)
        with pytest.raises(IndexError, match="index out of range"):
            suite_scheme.AggregateSignatures([], mask)
    with pytest.raises(IndexError):
        bdn.AggregatePublicKeys(bn256, mask)


def test_key_pair_draw_is_util_randoms_int():
    """rand.go:19-46: BitLen(order) bits, big-endian, the top byte masked, redrawn while not below the order.  Checked on
    the scalar alone (the public key is an engine call): a first draw at or above the order is skipped."""
    order = bn256.ORDER
    bits = order.bit_length()
    nbytes = (bits + 7) // 8
    high = (order + 5).to_bytes(nbytes, "big")
    low = (12345).to_bytes(nbytes, "big")
    stream = iter([bytes([0xFF]) + high[1:], low])
    drawn = []

    class Stop(Exception):
        pass

    sch = bdn.NewSchemeOnG1(bn256)

    class FakeElt:
        def Mul(self, x, base):
            drawn.append(x.v)
            raise Stop

    sch._elt = {1: FakeElt, 2: FakeElt}
    with pytest.raises(Stop):
        sch.NewKeyPair(lambda n: next(stream))
    masked = int.from_bytes(bytes([0xFF & ~(0xFF << (bits & 7)) & 0xFF if bits & 7 else 0xFF]) + high[1:], "big")
    assert drawn == [12345] if masked >= order else drawn == [masked]
