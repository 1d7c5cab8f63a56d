"""kyber_amd.sign.eddsa's signing half without a GPU.  The two new engine calls are answered by the lane programs
themselves, compiled for the CPU (tests/eddsa_harness.cpp through tests/test_eddsa_host.py's entry points), and the
standing verify call by a stand-in over the oracle (tests/_ed_verify_oracle.py), as tests/test_vss_callers_host.py does.
Under test is the host logic: who is asked what and how often, in which order the random stream is read, which error
is raised for which rejected signature -- and eddsa_test.go's TestEdDSAMarshalling, TestEdDSASigning and
TestEdDSASigningRandom restated."""
import numpy as np
import pytest

from kyber_amd.util import blake2xb
from tests import _ed_verify_oracle as VO
from tests import _eddsa_oracle as EO
from tests import test_eddsa_host as H


class ConstantStream:
    """eddsa_test.go:269-282: a cipher.Stream that always returns the same value"""

    def __init__(self, seed: bytes):
        self.seed = bytes(seed)

    def XORKeyStream(self, src: bytes) -> bytes:
        return self.seed[:len(src)]


@pytest.fixture(scope="module")
def harness():
    return H.build_harness()


@pytest.fixture
def calls(monkeypatch, harness):
    """the engine behind kyber_amd.group.edwards25519 replaced; returns the count of calls per entry"""
    from kyber_amd.group import edwards25519 as ed

    count = {}

    def counted(name):
        def wrap(f):
            def g(*a, **k):
                count[name] = count.get(name, 0) + 1
                return f(*a, **k)
            return g
        return wrap

    @counted("eddsa_expand")
    def eddsa_expand(seeds):
        return H.expand(harness, bytes(seeds))

    @counted("eddsa_sign")
    def eddsa_sign(secrets, prefixes, pubs, msgs):
        return H.sign(harness, bytes(secrets), bytes(prefixes), bytes(pubs), msgs), np.zeros(len(msgs), dtype=np.uint8)

    @counted("verify")
    def verify(pubs, msgs, sigs, want_status=True):
        rows = [(bytes(p), bytes(m), bytes(s)) for p, m, s in zip(pubs, msgs, sigs)]
        ok = np.array([VO.verify_with_checks(*r)[0] for r in rows], dtype=np.uint8)
        return ok, (np.array([VO.abi_status(*r) for r in rows], dtype=np.uint8) if want_status else None)

    def no_other(name):
        def f(*a, **k):
            raise AssertionError(f"{name}: sign/eddsa makes no such call")
        return f

    for name, f in (("batch_eddsa_expand", eddsa_expand), ("batch_eddsa_sign", eddsa_sign), ("batch_verify", verify),
                    ("batch_mul_base", no_other("batch_mul_base")), ("batch_mul", no_other("batch_mul")), ("batch_add", no_other("batch_add")),
                    ("batch_unmarshal", no_other("batch_unmarshal")), ("batch_schnorr_sign", no_other("batch_schnorr_sign"))):
        monkeypatch.setattr(ed, name, f)
    return count


# ---------------------------------------------------------------------------------------------- eddsa_test.go, restated
def test_marshalling(calls):
    """TestEdDSAMarshalling (eddsa_test.go:55-74)"""
    from kyber_amd.sign import eddsa

    for seed, pub, _, _ in EO.rfc8032():
        key = eddsa.NewEdDSA(ConstantStream(seed))
        assert key.Public.String() == pub.hex()
        marshalled = key.MarshalBinary()
        assert marshalled == seed + pub
        back = eddsa.EdDSA().UnmarshalBinary(marshalled)
        assert back == key and back.Secret.v == EO.expand(seed)[0] and back.prefix == EO.expand(seed)[1] and back.seed == seed
    assert calls == {"eddsa_expand": 10}


def test_signing(calls):
    """TestEdDSASigning (eddsa_test.go:76-107)"""
    from kyber_amd.sign import eddsa

    for seed, pub, msg, sig in EO.rfc8032():
        key = eddsa.NewEdDSA(ConstantStream(seed))
        assert key.Public.MarshalBinary() == pub
        assert key.Sign(msg) == sig
        assert eddsa.Verify(key.Public, msg, sig) is None
    assert calls == {"eddsa_expand": 5, "eddsa_sign": 5, "verify": 5}


def test_signing_random(calls):
    """TestEdDSASigningRandom (eddsa_test.go:247-267), sixteen rounds on a seeded stream"""
    from kyber_amd.sign import eddsa

    rand = blake2xb.New(b"eddsa signing random")
    for _ in range(16):
        key = eddsa.NewEdDSA(rand)
        msg = rand.Read(32)
        sig = key.Sign(msg)
        assert sig[63] & 0xE0 == 0  # RFC 8032 section 5.1.6 item 6
        assert eddsa.Verify(key.Public, msg, sig) is None


# -------------------------------------------------------------------------------------------------------- the batch forms
def test_new_batch_is_one_expand_and_equals_the_sequential_keys(calls):
    from kyber_amd.sign import eddsa

    n = 9
    keys = eddsa.NewEdDSABatch(blake2xb.New(b"eddsa batch"), n)
    assert calls == {"eddsa_expand": 1}
    stream = blake2xb.New(b"eddsa batch")
    one_by_one = [eddsa.NewEdDSA(stream) for _ in range(n)]
    assert calls == {"eddsa_expand": 1 + n}
    assert keys == one_by_one and len({k.seed for k in keys}) == n
    want = blake2xb.New(b"eddsa batch")
    for k in keys:  # 32 stream bytes a key, in order, and the oracle's expansion of them
        seed = want.Read(32)
        assert (k.seed, k.Secret.v, k.prefix, k.Public.MarshalBinary()) == (seed,) + EO.expand(seed)
    assert eddsa.NewEdDSABatch(blake2xb.New(b"none"), 0) == [] and calls == {"eddsa_expand": 1 + n}


def test_new_requires_a_stream(calls):
    from kyber_amd.sign import eddsa

    with pytest.raises(ValueError, match="^stream is required$"):
        eddsa.NewEdDSA(None)
    with pytest.raises(ValueError, match="^stream is required$"):
        eddsa.NewEdDSABatch(None, 3)
    assert calls == {}


def test_unmarshal_round_trips_and_refuses_a_wrong_length(calls):
    from kyber_amd.sign import eddsa

    keys = eddsa.NewEdDSABatch(blake2xb.New(b"eddsa marshal"), 4)
    buffs = [k.MarshalBinary() for k in keys]
    assert all(len(b) == 64 and b == k.seed + k.Public.MarshalBinary() for b, k in zip(buffs, keys))
    calls.clear()
    assert eddsa.UnmarshalBinaryBatch(buffs) == keys and calls == {"eddsa_expand": 1}
    assert [eddsa.EdDSA().UnmarshalBinary(b) for b in buffs] == keys
    # Public is recomputed from the seed, not read (eddsa.go:81-86)
    assert eddsa.EdDSA().UnmarshalBinary(buffs[0][:32] + buffs[1][32:]) == keys[0]
    calls.clear()
    for bad in (b"", buffs[0][:63], buffs[0] + b"\0", buffs[0][:32]):
        with pytest.raises(ValueError, match="^error: wrong length for decoding EdDSA private$"):
            eddsa.EdDSA().UnmarshalBinary(bad)
        with pytest.raises(ValueError, match="^error: wrong length for decoding EdDSA private$"):
            eddsa.UnmarshalBinaryBatch([buffs[1], bad])
    assert calls == {}  # the lengths are checked before anything is expanded


def test_sign_batch_is_one_call_for_one_key_and_for_n_keys(calls):
    from kyber_amd.sign import eddsa

    seeds, _, msgs, sigs = EO.sign_input()
    rows = [0, 1, 79, 80, 96, 97, 223, 224, 1023]
    keys = eddsa.UnmarshalBinaryBatch([bytes(seeds[i]) + bytes(32) for i in rows])
    calls.clear()
    got = eddsa.SignBatch(keys, [msgs[i] for i in rows])
    assert calls == {"eddsa_sign": 1}
    assert got == [sigs[i] for i in rows]
    assert got == [k.Sign(msgs[i]) for k, i in zip(keys, rows)] and calls == {"eddsa_sign": 1 + len(rows)}
    calls.clear()
    one = eddsa.SignBatch(keys[3], [msgs[i] for i in rows])
    assert calls == {"eddsa_sign": 1}
    assert one == [keys[3].Sign(msgs[i]) for i in rows]
    assert one == [EO.sign(keys[3].Secret.v, keys[3].prefix, keys[3].Public.MarshalBinary(), msgs[i]) for i in rows]
    calls.clear()
    assert eddsa.SignBatch([], []) == [] and eddsa.SignBatch(keys[0], []) == [] and calls == {}
    with pytest.raises(ValueError, match="length mismatch"):
        eddsa.SignBatch(keys[:3], [b"a", b"b"])


# ------------------------------------------------------------------------------------------------------------- Verify
TEXT = {
    VO.S_NONCANONICAL: "error: signature is not canonical",
    VO.R_NONCANONICAL: "error: point R is not canonical",
    VO.R_NOT_A_POINT: "error: point R invalid: invalid Ed25519 curve point",
    VO.R_SMALL_ORDER: "error: point R has small order",
    VO.A_NONCANONICAL: "error: public key is not canonical",
    VO.A_NOT_A_POINT: "error: invalid public key: invalid Ed25519 curve point",
    VO.A_SMALL_ORDER: "error: public key has small order",
    VO.EQUATION: "error: reconstructed S is not equal to signature",
}


def _raised(f, *a):
    try:
        assert f(*a) is None
        return None
    except ValueError as e:
        return str(e)


def test_verify_raises_the_references_nine_errors_in_its_order(calls):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import eddsa

    pub, msg, sig = VO.sign_input()[33]
    cases = [(p, m, s) for p, m, s, _ in VO.wycheproof()] + VO.synthetic_rejects()
    cases.append((pub, msg, sig[:63]))  # a 63-byte signature
    cases.append((pub, msg, sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]))  # an altered S
    cases.append((pub, msg, sig))
    seen = set()
    for p, m, s in cases:
        assert len(p) == 32
        before = calls.get("verify", 0)
        got = _raised(eddsa.VerifyWithChecks, p, m, s)
        if len(s) != 64:
            assert got == f"error: signature length invalid: expect 64 but got {len(s)}" and calls.get("verify", 0) == before
            seen.add(VO.LENGTH)
            continue
        assert calls["verify"] == before + 1  # one engine call each
        good, why = VO.verify_with_checks(p, m, s)
        assert got == (None if good else TEXT[why]), (p.hex(), s.hex(), why)
        seen.add(why)
        # the form that takes a point marshals it and goes the same way
        assert _raised(eddsa.Verify, ed.Point(p), m, s) == got
    assert seen == set(VO.REASONS)  # valid, and every one of the nine errors
    valid = [c for c in VO.wycheproof() if c[3] and len(c[2]) == 64]
    assert len(valid) == 88 and all(_raised(eddsa.VerifyWithChecks, *c[:3]) is None for c in valid[:8])
    # a key of another length fails IsCanonical (eddsa.go:197-199), behind R's checks
    assert _raised(eddsa.VerifyWithChecks, pub[:31], msg, sig) == TEXT[VO.A_NONCANONICAL]
    with pytest.raises(TypeError):
        eddsa.Verify(pub, msg, sig)
