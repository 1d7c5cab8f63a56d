"""share/vss's engine calls without a GPU: kyber_amd/csrc/ed25519_vss.cuh and the additional-data GCM of aes256gcm.cuh
compiled for the CPU (tests/vss_harness.cpp) against the OpenSSL fixtures of tests/golden/aes256gcm_aad.json, RFC 5869 and
the oracle (tests/_vss_oracle.py) on the labelled cases of tests/_vss_cases.py; the C ABI's argument checks.

Limit of the check: the reference's VSS tests print no bytes and no Go toolchain is at hand, so no transcript of the Go
program is pinned.  The fixtures pin AES-GCM with additional data, RFC 5869 test case 1 pins the HKDF with an info
string, schnorr.Sign is held to the verification equation of RFC 8032, and the composition is the oracle's, written
from vss.go's and dh.go's text."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _vss_cases as VC
from tests import _vss_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "aes256gcm_aad.json")))["aes256gcm_aad"]


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libvssharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "vss_harness.cpp")])
    h = C.CDLL(out)
    sz, b, p = C.c_size_t, C.c_char_p, C.c_void_p
    h.vsh_gcm_seal_aad.argtypes = [b, b, b, C.c_int, b, sz, b]
    h.vsh_gcm_open_aad.argtypes = [b, b, b, C.c_int, b, sz, b]
    h.vsh_kdf.argtypes = [b, b, sz, b]
    h.vsh_schnorr_sign.argtypes = [sz, p, p, sz, p, p, p, p]
    h.vsh_vss_seal.argtypes = [sz, p, p, p, p, p, p, sz, sz, p, p, p, p, p, p]
    h.vsh_vss_open.argtypes = [sz, p, sz, p, p, sz, sz, p, p, p, p]
    h.vsh_deal_check2.argtypes = [sz, p, p, p, p, sz, sz, p, p, sz, p, p]
    for f in (h.vsh_gcm_seal_aad, h.vsh_kdf, h.vsh_schnorr_sign, h.vsh_vss_seal, h.vsh_vss_open, h.vsh_deal_check2):
        f.restype = None
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _arr(x, dtype=np.uint8):
    return np.frombuffer(x, dtype=dtype) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=dtype)


def _packed(msgs, lead: int = 0):
    """(exactly sized blob, offsets): `lead` stray bytes stand in front of the first element"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += np.uint64(lead)
    return _arr(b"\xa5" * lead + b"".join(msgs) or b"\0"), off


# the four entry points of the harness, with the shapes of kyber_amd.group.edwards25519's batch_* wrappers
def sign(h, k, x, msgs):
    k, x = _arr(k).reshape(-1, 32), _arr(x).reshape(-1, 32)
    n = k.shape[0]
    blob, off = _packed(msgs, 3)
    sigs, st = np.full((n, 64), 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    h.vsh_schnorr_sign(n, k.ctypes.data, x.ctypes.data, 32 if x.shape[0] == n else 0, blob.ctypes.data,
                       off.ctypes.data, sigs.ctypes.data, st.ctypes.data)
    assert not st.any()
    return [bytes(s) for s in sigs]


def seal(h, dh, k, priv, pub, vpubs, ctx, msgs, lead: int = 1, ctx_len: int = 32):
    dh, k, vpubs = (_arr(a).reshape(-1, 32) for a in (dh, k, vpubs))
    ctx = _arr(ctx).reshape(-1, ctx_len)
    n = dh.shape[0]
    blob, off = _packed(msgs, lead)
    total = int(off[-1])
    keys, sigs = np.full((n, 32), 0xEE, dtype=np.uint8), np.full((n, 64), 0xEE, dtype=np.uint8)
    out, st = np.full(total + 16 * n, 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    h.vsh_vss_seal(n, dh.ctypes.data, k.ctypes.data, _arr(priv).ctypes.data, _arr(pub).ctypes.data, vpubs.ctypes.data, ctx.ctypes.data,
                   ctx_len if ctx.shape[0] > 1 else 0, ctx_len, blob.ctypes.data, off.ctypes.data, keys.ctypes.data, sigs.ctypes.data, out.ctypes.data,
                   st.ctypes.data)
    assert bytes(out[:lead]) == b"\xee" * lead  # nothing in front of the first cipher
    ciphers = [bytes(out[int(off[i]) + 16 * i:int(off[i + 1]) + 16 * (i + 1)]) for i in range(n)]
    return [bytes(x) for x in keys], [bytes(x) for x in sigs], ciphers, st


def open_(h, privs, keys, ctx, ciphers, ctx_len: int = 32):
    privs, keys = (_arr(a).reshape(-1, 32) for a in (privs, keys))
    ctx = _arr(ctx).reshape(-1, ctx_len)
    n = keys.shape[0]
    blob, off = _packed(ciphers)
    out, st = np.full(max(int(off[-1]), 1) + 1, 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    h.vsh_vss_open(n, privs.ctypes.data, 32 if privs.shape[0] > 1 else 0, keys.ctypes.data, ctx.ctypes.data, ctx_len if ctx.shape[0] > 1 else 0, ctx_len,
                   blob.ctypes.data, off.ctypes.data, out.ctypes.data, st.ctypes.data)
    assert out[int(off[-1])] == 0xEE  # nothing written past the last slot
    return [bytes(out[int(off[i]):int(off[i + 1])]) for i in range(n)], st


def check2(h, poly, idx, f, g, m, t, commits, H):
    poly, idx = _arr(poly, np.uint32), _arr(idx, np.uint32)
    n = len(poly)
    f, g, commits, H = _arr(f), _arr(g), _arr(commits or b"\0"), _arr(H)
    ok, st = np.full(max(n, 1), 0xEE, dtype=np.uint8), np.full(max(m, 1), 0xEE, dtype=np.uint8)
    h.vsh_deal_check2(n, poly.ctypes.data, idx.ctypes.data, f.ctypes.data, g.ctypes.data, m, t, commits.ctypes.data, H.ctypes.data,
                      32 if len(H) > 32 else 0, ok.ctypes.data, st.ctypes.data)
    return list(ok[:n]), list(st[:m])


# ------------------------------------------------------------------------------------------------------ the yardsticks
def test_fixture_holds_the_specification_case_and_every_length():
    by_name = {c["name"]: c for c in GOLDEN}
    spec = by_name["gcm-spec test case 16"]
    assert len(bytes.fromhex(spec["aad"])) == 20 and spec["sealed"].endswith("76fc6ece0f4e1768cddf8853bb2d551b")
    assert spec["sealed"].startswith("522dc1f099567d07f47f37a32a84427d")
    from tests._ecies_oracle import LENGTHS

    for prefix, aad_len in (("random,", 32), ("random128,", 128)):
        rnd = [c for c in GOLDEN if c["name"].startswith(prefix)]
        assert sorted(len(bytes.fromhex(c["msg"])) for c in rnd) == sorted(LENGTHS)
        assert all(c["nonce"] == "00" * 12 and len(c["aad"]) == 2 * aad_len for c in rnd)


def test_python_oracle_matches_the_fixture_and_rfc5869():
    for c in GOLDEN:
        key, nonce, aad, msg, sealed = (bytes.fromhex(c[k]) for k in ("key", "nonce", "aad", "msg", "sealed"))
        assert VO.gcm_seal_aad(key, nonce, msg, aad) == sealed, c["name"]
        assert VO.gcm_open_aad(key, nonce, sealed, aad) == msg, c["name"]
        assert VO.gcm_open_aad(key, nonce, sealed[:-1] + bytes([sealed[-1] ^ 1]), aad) is None
        assert VO.gcm_open_aad(key, nonce, sealed, aad[:-1] + bytes([aad[-1] ^ 1])) is None
    # RFC 5869 appendix A.1: SHA-256, a salt and an info string
    okm = VO.hkdf_sha256(bytes([0x0B]) * 22, bytes(range(13)), bytes(range(0xF0, 0xFA)), 42)
    assert okm.hex() == "3cb25f25faacd57a90434f64d0362f2a2d2d0a90cf1a5a4c5db02d56ecc4c5bf34007208d5b887185865"
    # appendix A.3 through the same function: no salt, no info
    assert VO.hkdf_sha256(bytes([0x0B]) * 22, b"", b"", 42).hex() == (
        "8da4e775a563c18f715f802a063c5a31b8a11f5c5ee1879ec3454e5f3c738d2d9d201395faa4b61a96c8")


def test_gcm_with_additional_data_matches_the_fixture_at_every_length(harness):
    for c in GOLDEN:
        key, nonce, aad, msg, sealed = (bytes.fromhex(c[k]) for k in ("key", "nonce", "aad", "msg", "sealed"))
        if len(aad) % 16:
            continue  # the device function takes whole blocks: a context is 32 or 128 bytes
        out = C.create_string_buffer(len(msg) + 16)
        harness.vsh_gcm_seal_aad(key, nonce, aad, len(aad) // 16, msg, len(msg), out)
        assert out.raw == sealed, c["name"]
        back = C.create_string_buffer(b"\xff" * (len(msg) + 1), len(msg) + 1)
        assert harness.vsh_gcm_open_aad(key, nonce, aad, len(aad) // 16, sealed, len(msg), back) == 1, c["name"]
        assert back.raw == msg + b"\xff", c["name"]
        for bad_aad, bad_sealed in ((aad[:5] + bytes([aad[5] ^ 4]) + aad[6:], sealed), (aad, sealed[:-3] + bytes([sealed[-3] ^ 1]) + sealed[-2:])):
            assert harness.vsh_gcm_open_aad(key, nonce, bad_aad, len(aad) // 16, bad_sealed, len(msg), back) == 0
            assert back.raw == bytes(len(msg)) + b"\xff"


def test_key_derivation_is_one_expand_step_with_the_context(harness):
    for i in range(8):
        pre, ctx = O.mul_base(bytes([i + 1]) + bytes(31)), bytes(VC.scalars(b"kdf ctx %d" % i, 1, 0xFF)[0])
        out = C.create_string_buffer(32)
        harness.vsh_kdf(pre, ctx, 32, out)
        assert out.raw == VO.aead_key(pre, ctx)
        long = bytes(VC.scalars(b"kdf ctx128 %d" % i, 4, 0xFF).reshape(-1))  # rabin's 128 bytes: the message ends in a third block
        harness.vsh_kdf(pre, long, 128, out)
        assert out.raw == VO.aead_key(pre, long)


# -------------------------------------------------------------------------------------------------------- schnorr.Sign
def test_sign_matches_the_oracle_and_the_equation_holds(harness):
    k, x, m, want = VC.sign_pool()
    rows = list(range(len(VC.SIGN_LENGTHS) + 3)) + [VC.POOL - 3, VC.POOL - 2, VC.POOL - 1]
    got = sign(harness, k[rows], x[rows], [m[i] for i in rows])
    assert got == [want[i] for i in rows]
    for i in rows[:-2]:
        assert VO.schnorr_holds(O.mul_base(bytes(x[i])), m[i], want[i]), i
    for i in rows[-2:]:  # a key or a nonce at or above 2^255, where Point.Mul drops the top digit: bytes, but no signature
        assert not VO.schnorr_holds(O.mul_base(bytes(x[i])), m[i], want[i]), i
    # one signer for the batch
    got = sign(harness, k[:5], x[7], m[:5])
    assert got == [VO.schnorr_sign(bytes(k[i]), bytes(x[7]), m[i]) for i in range(5)]


# ----------------------------------------------------------------------------------------------------- seal and open
@pytest.mark.parametrize("per_element_ctx", [False, True])
def test_seal_matches_the_oracle_with_rejects_planted(harness, per_element_ctx):
    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(per_element_ctx)
    for lo, hi in ((0, 2 * len(VC.LENGTHS)), (VC.POOL - 65, VC.POOL)):
        c = ctx[lo:hi] if per_element_ctx else ctx
        keys, sigs, ciphers, st = seal(harness, dh[lo:hi], k[lo:hi], priv, pub, vpubs[lo:hi], c, m[lo:hi], lead=1 + lo % 2)
        for j, i in enumerate(range(lo, hi)):
            if want[i] is None:
                assert st[j] == _lib.ST_BAD_POINT and (keys[j], sigs[j], ciphers[j]) == (bytes(32), bytes(64), bytes(len(m[i]) + 16)), i
            else:
                assert st[j] == 0 and (keys[j], sigs[j], ciphers[j]) == want[i], i
                assert VO.schnorr_holds(pub, keys[j], sigs[j])


@pytest.mark.parametrize("per_element_ctx", [False, True])
def test_open_round_trips_and_rejects_in_the_reference_order(harness, per_element_ctx):
    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(per_element_ctx)
    good = [i for i in range(3, 3 + len(VC.LENGTHS)) if want[i] is not None and i not in VC.SPECIAL]
    # a receiver each
    c = ctx[good] if per_element_ctx else ctx
    back, st = open_(harness, vpriv[good], b"".join(want[i][0] for i in good), c, [want[i][2] for i in good])
    assert not st.any() and back == [m[i] + bytes(16) for i in good]
    # one receiver, every tamper: the rows of the case table under element 5's key and context
    i = 5
    cx = bytes(ctx[i] if per_element_ctx else ctx[0])
    sealed = [VO.seal(bytes(dh[j]), bytes(k[j]), priv, pub, bytes(vpubs[i]), cx, m[j]) for j in good]
    rows = VC.open_cases(bytes(vpriv[i]), cx, sealed)
    back, st = open_(harness, vpriv[i], b"".join(r[0] for r in rows), cx, [r[1] for r in rows])
    seen = set()
    for j, (key, cipher, label) in enumerate(rows):
        msg, code = VO.open_(bytes(vpriv[i]), key, cx, cipher)
        assert st[j] == code and back[j] == (msg or b"") + bytes(len(cipher) - len(msg or b"")), (j, label)
        seen.add((label, code))
    assert {("good", 0), ("tag bit", 10), ("cipher bit", 10), ("short", 9), ("undecodable key", 1), ("another key", 10)} <= seen
    # a flipped context bit fails every element
    flipped = bytes([cx[0] ^ 1]) + cx[1:]
    back, st = open_(harness, vpriv[i], b"".join(s[0] for s in sealed), flipped, [s[2] for s in sealed])
    assert list(st) == [_lib.ST_ECIES_AUTH] * len(sealed) and all(b == bytes(len(b)) for b in back)


@pytest.mark.parametrize("per_element_ctx", [False, True])
def test_seal_and_open_under_rabins_128_byte_context(harness, per_element_ctx):
    dh, k, priv, pub, vpriv, vpubs, _, m, _ = VC.seal_pool(False)
    rows = list(range(13, 13 + len(VC.LENGTHS)))  # (every length once, no planted key among them)
    assert not set(rows) & set(VC.SPECIAL)
    ctx = VC.scalars(b"vss ctx128", 4 * (len(rows) if per_element_ctx else 1), 0xFF).reshape(-1, 128)
    want = [VO.seal(bytes(dh[i]), bytes(k[i]), priv, pub, bytes(vpubs[i]), bytes(ctx[j if per_element_ctx else 0]), m[i]) for j, i in enumerate(rows)]
    keys, sigs, ciphers, st = seal(harness, dh[rows], k[rows], priv, pub, vpubs[rows], ctx, [m[i] for i in rows], lead=3, ctx_len=128)
    assert not st.any() and list(zip(keys, sigs, ciphers)) == want
    back, st = open_(harness, vpriv[rows], b"".join(keys), ctx, ciphers, ctx_len=128)
    assert not st.any() and back == [m[i] + bytes(16) for i in rows]
    flipped = ctx.copy()
    flipped[:, 127] ^= 1  # the last byte of the context: the third block of the HMAC, the eighth of the additional data
    back, st = open_(harness, vpriv[rows], b"".join(keys), flipped, ciphers, ctx_len=128)
    assert list(st) == [_lib.ST_ECIES_AUTH] * len(rows) and all(b == bytes(len(b)) for b in back)


# ------------------------------------------------------------------------------------------------- Rabin's share check
@pytest.mark.parametrize("per_poly_h", [False, True])
def test_deal_check2_on_the_share_table(harness, per_poly_h):
    poly, idx, f, g, m, t, commits, H, want_ok, want_st, labels = VC.check2_table(per_poly_h)
    ok, st = check2(harness, poly, idx, f, g, m, t, commits, H)
    bad = {0, 4, 6, 11} if per_poly_h else {0, 6, 11}  # first, middle and last place (tests/_vss_cases.py)
    assert st == want_st == [1 if k in bad else 0 for k in range(m)]
    assert ok == want_ok
    for k, o, label in zip(poly, ok, labels):
        if label in ("right", "both + l") and not want_st[k] and not (per_poly_h and k in (2, 7)):
            assert o == 1, (k, label)  # (where H has a torsion component, reducing g mod l moves g H: the oracle decides)
        if label in ("forged f", "forged g") and not (per_poly_h and k in (1, 3) and label == "forged g"):
            assert o == 0, (k, label)  # (g does not matter where H is the identity)
    if not per_poly_h:  # ONE H for the batch that does not decode marks every polynomial
        ok, st = check2(harness, poly[:8], idx[:8], f[:256], g[:256], m, t, commits, DC.UNDECODABLE)
        assert ok == [0] * 8 and st == [1] * m
    # a check that names a polynomial the table does not hold
    assert check2(harness, [m], [0], f[:32], g[:32], m, t, commits, H)[0] == [0]


def test_deal_check2_at_every_threshold(harness):
    for t in range(18):
        rows, commits, H, want = VC.check2_threshold(t)
        n = len(rows)
        ok, st = check2(harness, [0] * n, [r[0] for r in rows], b"".join(r[1] for r in rows), b"".join(r[2] for r in rows), 1, t, commits, H)
        assert ok == want == [1, 0, 0] * 3 and st == [0], t


# ------------------------------------------------------------------------------------------------- the C ABI's checks
def test_argument_errors_and_empty_batches_never_touch_the_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert lib.kyb_ed25519_schnorr_sign(0, p, p, 32, p, p, p, p) == 0
    assert lib.kyb_ed25519_schnorr_sign_dev(0, p, p, 0, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_vss_seal(0, p, p, p, p, p, p, 0, 32, p, p, p, p, p, p) == 0
    assert lib.kyb_ed25519_vss_seal_dev(0, p, p, p, p, p, p, 128, 128, p, p, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_vss_open(0, p, 0, p, p, 32, 32, p, p, p, p) == 0
    assert lib.kyb_ed25519_vss_open_dev(0, p, 32, p, p, 0, 128, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_deal_check2(0, p, p, p, p, 0, 0, p, p, 0, p, p) == 0
    assert lib.kyb_ed25519_deal_check2_dev(0, p, p, p, p, 3, 2, p, p, 32, p, p, None) == 0
    off = (C.c_uint64 * 3)(0, 40, 8)  # decreasing
    po = C.addressof(off)
    one = (C.c_uint32 * 2)(0, 1)  # names polynomial 1 of a table of one
    bad = [
        ("kyb_ed25519_schnorr_sign", (2, p, p, 32, p, po, p, p)),
        ("kyb_ed25519_schnorr_sign", (2, p, p, 16, p, p, p, p)),
        ("kyb_ed25519_schnorr_sign", (2, None, p, 32, p, p, p, p)),
        ("kyb_ed25519_schnorr_sign_dev", (2, p, p, 33, p, p, p, p, None)),
        ("kyb_ed25519_schnorr_sign_dev", (2, p, p, 0, p, p, None, p, None)),
        ("kyb_ed25519_vss_seal", (2, p, p, p, p, p, p, 0, 32, p, po, p, p, p, p)),
        ("kyb_ed25519_vss_seal", (2, p, p, p, p, p, p, 8, 32, p, p, p, p, p, p)),
        ("kyb_ed25519_vss_seal", (2, p, p, p, p, p, p, 32, 128, p, p, p, p, p, p)),  # a stride that is not the length
        ("kyb_ed25519_vss_seal", (2, p, p, p, p, p, p, 0, 64, p, p, p, p, p, p)),  # a length neither package has
        ("kyb_ed25519_vss_seal", (2, p, p, None, p, p, p, 0, 32, p, p, p, p, p, p)),
        ("kyb_ed25519_vss_seal_dev", (2, p, p, p, p, p, p, 64, 32, p, p, p, p, p, p, None)),
        ("kyb_ed25519_vss_seal_dev", (2, p, p, p, p, p, p, 0, 128, p, p, p, None, p, p, None)),
        ("kyb_ed25519_vss_open", (2, p, 0, p, p, 0, 32, p, po, p, p)),
        ("kyb_ed25519_vss_open", (2, p, 8, p, p, 0, 32, p, p, p, p)),
        ("kyb_ed25519_vss_open", (2, p, 0, p, p, 31, 32, p, p, p, p)),
        ("kyb_ed25519_vss_open", (2, p, 0, p, p, 128, 32, p, p, p, p)),
        ("kyb_ed25519_vss_open", (2, p, 0, p, p, 0, 0, p, p, p, p)),
        ("kyb_ed25519_vss_open", (2, p, 32, p, p, 0, 32, p, p, None, p)),
        ("kyb_ed25519_vss_open_dev", (2, p, 64, p, p, 0, 32, p, p, p, p, None)),
        ("kyb_ed25519_deal_check2", (2, C.addressof(one), p, p, p, 1, 2, p, p, 0, p, p)),
        ("kyb_ed25519_deal_check2", (2, p, p, p, None, 1, 2, p, p, 0, p, p)),
        ("kyb_ed25519_deal_check2", (2, p, p, p, p, 1, 2, p, p, 16, p, p)),
        ("kyb_ed25519_deal_check2_dev", (2, p, p, p, p, 1, 2, p, None, 0, p, p, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, name
        assert name.encode() in lib.kyb_last_error()
    assert lib.kyb_ed25519_deal_check2(2, p, p, p, p, 1 << 40, 1 << 40, p, p, 0, p, p) == -4  # KYB_E_ALLOC: no such workspace
