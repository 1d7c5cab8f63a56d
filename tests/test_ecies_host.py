"""encrypt/ecies and the deal check without a GPU: kyber_amd/csrc/aes256gcm.cuh and ed25519_dkg.cuh compiled for the CPU
(tests/dkg_harness.cpp) against the OpenSSL fixtures of tests/golden/aes256gcm.json, hmac / hashlib and the oracles
(tests/_ecies_oracle.py, oracle/ed25519.py); the C ABI's argument checks.

The reference prints no ECIES bytes and no Go toolchain is at hand, so no transcript of the Go program is pinned: the
fixtures pin AES-GCM, RFC 5869 pins the HKDF, and the composition is the oracle's, written from ecies.go's text."""
import ctypes as C
import hashlib
import hmac
import json
import os
import subprocess

import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _ecies_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "aes256gcm.json")))


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libdkgharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "dkg_harness.cpp")])
    h = C.CDLL(out)
    sz, b = C.c_size_t, C.c_char_p
    h.dkg_sbox.argtypes = [b]
    h.dkg_aes_expand.argtypes = [b, b]
    h.dkg_aes_block.argtypes = [b, b, b]
    h.dkg_gcm_seal.argtypes = [b, b, b, sz, b]
    h.dkg_gcm_open.argtypes = [b, b, b, sz, b]
    h.dkg_hkdf.argtypes = [b, C.c_int, b]
    h.dkg_ecies_seal.argtypes = [b, b, b, sz, b]
    h.dkg_ecies_open.argtypes = [b, b, sz, b]
    h.dkg_deal_check.argtypes = [b, C.c_uint32, sz, b]
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _cases():
    return [tuple(bytes.fromhex(c[k]) for k in ("key", "nonce", "msg", "sealed")) + (c["name"],) for c in GOLDEN["aes256gcm"]]


def test_fixtures_hold_the_specification_cases_and_every_length():
    by_name = {c["name"]: c for c in GOLDEN["aes256gcm"]}
    assert by_name["gcm-spec test case 13"]["sealed"] == "530f8afbc74536b9a963b4f1c4cb738b"
    assert by_name["gcm-spec test case 14"]["sealed"] == "cea7403d4d606b6e074ec5d3baf39d18" + "d0d1c8a799996bf0265b98b5d48ab919"
    assert sorted(len(bytes.fromhex(c["msg"])) for c in GOLDEN["aes256gcm"] if c["name"].startswith("random")) == sorted(EO.LENGTHS)
    k = GOLDEN["hkdf_sha256"][0]
    assert k["okm"] == "8da4e775a563c18f715f802a063c5a31b8a11f5c5ee1879ec3454e5f3c738d2d9d201395faa4b61a96c8"


def test_python_oracle_matches_the_fixtures():
    for key, nonce, msg, sealed, name in _cases():
        assert EO.gcm_seal(key, nonce, msg) == sealed, name
        assert EO.gcm_open(key, nonce, sealed) == msg, name
        if sealed:
            bad = sealed[:-1] + bytes([sealed[-1] ^ 1])
            assert EO.gcm_open(key, nonce, bad) is None, name
    k = GOLDEN["hkdf_sha256"][0]
    assert EO.hkdf_sha256(bytes.fromhex(k["ikm"]), k["length"]).hex() == k["okm"]


def test_sbox_key_schedule_and_block_match_the_oracle(harness):
    out = C.create_string_buffer(256)
    harness.dkg_sbox(out)
    assert list(out.raw) == EO.SBOX
    assert out.raw[:4].hex() == "637c777b" and out.raw[255] == 0x16  # FIPS 197 figure 7's corners
    for key, _, _, _, name in _cases():
        rk = C.create_string_buffer(240)
        assert harness.dkg_aes_expand(key, rk) == 1, name  # the LDS layout and the plain one agree
        w = EO.expand_key(key)
        assert rk.raw == b"".join(w), name
        for block in (bytes(16), bytes(range(16)), hashlib.sha256(key).digest()[:16]):
            o = C.create_string_buffer(16)
            harness.dkg_aes_block(key, block, o)
            assert o.raw == EO.encrypt_block(w, block), name
    # FIPS 197 appendix C.3
    o = C.create_string_buffer(16)
    harness.dkg_aes_block(bytes(range(32)), bytes.fromhex("00112233445566778899aabbccddeeff"), o)
    assert o.raw.hex() == "8ea2b7ca516745bfeafc49904b496089"


def test_gcm_seal_and_open_match_the_fixtures_at_every_length(harness):
    for key, nonce, msg, sealed, name in _cases():
        out = C.create_string_buffer(len(msg) + 16)
        harness.dkg_gcm_seal(key, nonce, msg, len(msg), out)
        assert out.raw == sealed, name
        back = C.create_string_buffer(b"\xff" * (len(msg) + 1), len(msg) + 1)
        assert harness.dkg_gcm_open(key, nonce, sealed, len(msg), back) == 1, name
        assert back.raw[:len(msg)] == msg and back.raw[len(msg)] == 0xFF, name


def test_hkdf_matches_hmac_and_rfc5869(harness):
    out = C.create_string_buffer(64)
    k = GOLDEN["hkdf_sha256"][0]
    harness.dkg_hkdf(bytes.fromhex(k["ikm"]), 22, out)
    assert out.raw[:42].hex() == k["okm"]
    for i in range(8):
        dh = hashlib.sha256(b"dh %d" % i).digest()
        harness.dkg_hkdf(dh, 32, out)
        prk = hmac.new(bytes(32), dh, hashlib.sha256).digest()
        t1 = hmac.new(prk, b"\x01", hashlib.sha256).digest()
        t2 = hmac.new(prk, t1 + b"\x02", hashlib.sha256).digest()
        assert out.raw == t1 + t2
        assert EO.derive(dh) == (t1, t2[:12])


R_SCALAR = DC.le(DC.scalar(b"ecies host r"))
X_SCALAR = DC.le(DC.scalar(b"ecies host x"))
PUB = O.mul_base(X_SCALAR)


def _msg(ln: int) -> bytes:
    return hashlib.shake_256(b"ecies host msg %d" % ln).digest(ln)


@pytest.fixture(scope="module")
def sealed():
    return {ln: EO.encrypt(R_SCALAR, PUB, _msg(ln)) for ln in EO.LENGTHS}


def _open(harness, priv, ctx):
    out = C.create_string_buffer(b"\xff" * (len(ctx) + 1), len(ctx) + 1)
    st = harness.dkg_ecies_open(priv, ctx, len(ctx), out)
    assert out.raw[len(ctx)] == 0xFF  # nothing written past the element's slot
    return st, out.raw[:len(ctx)]


def test_ecies_lane_programs_match_the_oracle_at_every_length(harness, sealed):
    for ln in EO.LENGTHS:
        out = C.create_string_buffer(b"\xff" * (ln + 49), ln + 49)
        assert harness.dkg_ecies_seal(R_SCALAR, PUB, _msg(ln), ln, out) == 0
        assert out.raw == sealed[ln] + b"\xff", ln
        st, slot = _open(harness, X_SCALAR, sealed[ln])
        assert st == 0 and slot == _msg(ln) + bytes(48), ln
        assert EO.decrypt(X_SCALAR, sealed[ln]) == (_msg(ln), 0)


def test_ecies_special_recipients(harness):
    msg = _msg(33)
    for pub in (DC.IDENTITY, DC.ORDER8, DC.NONCANONICAL):
        out = C.create_string_buffer(33 + 48)
        assert harness.dkg_ecies_seal(R_SCALAR, pub, msg, 33, out) == 0
        assert out.raw == EO.encrypt(R_SCALAR, pub, msg)
    out = C.create_string_buffer(b"\xff" * (33 + 48), 33 + 48)
    assert harness.dkg_ecies_seal(R_SCALAR, DC.UNDECODABLE, msg, 33, out) == _lib.ST_BAD_POINT
    assert out.raw == bytes(33 + 48) and EO.encrypt(R_SCALAR, DC.UNDECODABLE, msg) is None


def test_every_tamper_is_an_authentication_failure_with_a_zeroed_slot(harness, sealed):
    for ln in EO.LENGTHS:
        ctx = sealed[ln]
        for at in ({32, len(ctx) - 17, len(ctx) - 1} if ln else {len(ctx) - 1}):  # first / last ciphertext byte, last tag byte
            bad = bytearray(ctx)
            bad[at] ^= 0x40
            st, slot = _open(harness, X_SCALAR, bytes(bad))
            assert st == _lib.ST_ECIES_AUTH and slot == bytes(len(ctx)), (ln, at)
            assert EO.decrypt(X_SCALAR, bytes(bad)) == (None, EO.ST_ECIES_AUTH)
    # R itself: another point (authentication fails) or no point at all -- the oracle says which
    for flip in range(8):
        bad = bytearray(sealed[32])
        bad[0] ^= 1 << flip
        want = EO.decrypt(X_SCALAR, bytes(bad))[1]
        assert want in (EO.ST_BAD_POINT, EO.ST_ECIES_AUTH)
        st, slot = _open(harness, X_SCALAR, bytes(bad))
        assert st == want and slot == bytes(len(bad)), flip
    bad = DC.UNDECODABLE + sealed[32][32:]
    assert _open(harness, X_SCALAR, bad) == (_lib.ST_BAD_POINT, bytes(len(bad)))


def test_short_elements(harness, sealed):
    for ln in (0, 31, 32, 47):
        ctx = sealed[64][:ln]
        st, slot = _open(harness, X_SCALAR, ctx)
        assert st == _lib.ST_ECIES_SHORT and slot == bytes(ln), ln
        assert EO.decrypt(X_SCALAR, ctx) == (None, EO.ST_ECIES_SHORT)
    assert _open(harness, X_SCALAR, sealed[0])[0] == 0  # 48 bytes: an empty message


def test_deal_check_lane_program_on_the_share_table(harness):
    coeffs = [DC.scalar(b"deal host %d" % j) for j in range(4)]
    for t in (0, 1, 2, 3, 4):
        commits = [O.mul_base(DC.le(c)) for c in coeffs[:t]]
        for idx in DC.INDICES:
            for label, share in DC.share_table(coeffs[:t], idx):
                want = DC.expected_ok(share, commits, idx)
                if label in ("right", "right + l"):
                    assert want == 1, (t, idx, label)
                if label == "right + 1":
                    assert want == 0
                assert harness.dkg_deal_check(share, idx, t, b"".join(commits)) == want, (t, idx, label)
    # the all-identity polynomial takes the share 0; commitments off the subgroup or written non-canonically
    ident = [DC.IDENTITY, DC.NONCANONICAL, DC.IDENTITY]
    assert harness.dkg_deal_check(bytes(32), 7, 3, b"".join(ident)) == 1 == DC.expected_ok(bytes(32), ident, 7)
    assert harness.dkg_deal_check(DC.le(DC.L), 7, 3, b"".join(ident)) == 1
    mixed = [O.mul_base(DC.le(coeffs[0])), DC.ORDER8, DC.NONCANONICAL]
    for idx in (0, 1, 2, 7):  # x = 8 kills the order-8 component: the evaluation is back in the subgroup
        share = DC.le(coeffs[0])
        want = DC.expected_ok(share, mixed, idx)
        assert want == (1 if idx == 7 else 0)
        assert harness.dkg_deal_check(share, idx, 3, b"".join(mixed)) == want, idx
    assert harness.dkg_deal_check(bytes(32), 0, 3, b"".join([DC.IDENTITY, DC.UNDECODABLE, DC.IDENTITY])) == -1


def test_argument_errors_and_empty_batches_never_touch_the_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert lib.kyb_ed25519_ecies_seal(0, p, p, 32, p, p, p, p) == 0
    assert lib.kyb_ed25519_ecies_seal_dev(0, p, p, 0, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_ecies_open(0, p, 0, p, p, p, p) == 0
    assert lib.kyb_ed25519_ecies_open_dev(0, p, 32, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_deal_check(0, p, p, p, 0, 0, p, p, p) == 0
    assert lib.kyb_ed25519_deal_check_dev(0, p, p, p, 3, 2, p, p, p, None) == 0
    off = (C.c_uint64 * 3)(0, 40, 8)  # decreasing
    po = C.addressof(off)
    one = (C.c_uint32 * 2)(0, 1)  # names polynomial 1 of a table of one
    bad = [
        ("kyb_ed25519_ecies_seal", (2, p, p, 32, p, po, p, p)),
        ("kyb_ed25519_ecies_seal", (2, p, p, 16, p, p, p, p)),
        ("kyb_ed25519_ecies_seal", (2, None, p, 32, p, p, p, p)),
        ("kyb_ed25519_ecies_seal_dev", (2, p, p, 33, p, p, p, p, None)),
        ("kyb_ed25519_ecies_open", (2, p, 0, p, po, p, p)),
        ("kyb_ed25519_ecies_open", (2, p, 8, p, p, p, p)),
        ("kyb_ed25519_ecies_open", (2, p, 32, p, p, None, p)),
        ("kyb_ed25519_ecies_open_dev", (2, p, 64, p, p, p, p, None)),
        ("kyb_ed25519_deal_check", (2, C.addressof(one), p, p, 1, 2, p, p, p)),
        ("kyb_ed25519_deal_check", (2, p, p, None, 1, 2, p, p, p)),
        ("kyb_ed25519_deal_check_dev", (2, p, p, p, 1, 2, None, p, p, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, name
        assert name.encode() in lib.kyb_last_error()
    assert lib.kyb_ed25519_deal_check(2, p, p, p, 1 << 40, 1 << 40, p, p, p) == -4  # KYB_E_ALLOC: no such workspace
