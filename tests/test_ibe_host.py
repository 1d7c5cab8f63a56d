"""encrypt/ibe without a GPU: the oracle's Encrypt/Decrypt CCA in both orientations, the golden vector's verdict, the
C ABI's argument checks, and the per-lane hashing of kyber_amd/csrc/bls12381_ibe.cuh compiled for the CPU against
hashlib (tests/ibe_harness.cpp)."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess

import pytest

from oracle import bls12381 as O
from tests import _ibe_oracle as IBE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 16, 31, 32)


@pytest.mark.parametrize("on_g2", [False, True])
def test_oracle_round_trips_both_orientations(on_g2):
    ident = b"round 1234"
    master, private = IBE.keys(on_g2, 0x5EED1234 % O.R, ident)
    g = IBE.gid(on_g2, master, ident)
    rng = random.Random(7 + on_g2)
    for ln in LENGTHS:
        msg, sigma = bytes(rng.getrandbits(8) for _ in range(ln)), bytes(rng.getrandbits(8) for _ in range(ln))
        U, V, W = IBE.encrypt(on_g2, master, ident, msg, sigma, g=g)
        assert len(U) == (96 if on_g2 else 48) and len(V) == len(W) == ln
        assert IBE.decrypt(on_g2, private, U, V, W) == msg
        if ln:  # a flipped bit of W changes msg, so h3 and with it rP
            with pytest.raises(ValueError):
                IBE.decrypt(on_g2, private, U, V, bytes([W[0] ^ 1]) + W[1:])


def test_golden_vector_opens_but_fails_the_rp_check(golden_dir):
    """ibe_test.go:202-245's ciphertext: sigma and msg come out as deadbeef..., but its U predates today's h3, so the full
    DecryptCCAonG1 stops at the rP check -- on the engine that is status KYB_ST_IBE_CHECK, not a decode status."""
    v = json.load(open(os.path.join(golden_dir, "bls12381_ibe.json")))
    U, beacon = bytes.fromhex(v["U_g1"]), bytes.fromhex(v["beacon_g2"])
    V, W, want = bytes.fromhex(v["V"]), bytes.fromhex(v["W"]), bytes.fromhex(v["expected"])
    sigma, msg = IBE._ibe_decrypt(O.pair_bytes(U, beacon), V, W, IBE.TAGS)
    assert msg == want
    assert O.g1_compress(O.g1_mul(IBE.h3(sigma, msg), O.G1_GEN)) != U
    with pytest.raises(ValueError, match="rP check"):
        IBE.decrypt(False, beacon, U, V, W)


def test_header_cites_ibe_go():
    src = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    for cite in ("ibe.go:51-232", "ibe.go:234-281", "KYB_ST_IBE_CHECK 3", "KYB_ST_IBE_H3 4"):
        assert cite in src


_IBE = ("kyb_bls12381_ibe_encrypt_g1", "kyb_bls12381_ibe_encrypt_g2", "kyb_bls12381_ibe_decrypt_g1", "kyb_bls12381_ibe_decrypt_g2")


def _call(lib, name, n, msg_len=16, stride=None, null=False):
    """one call of an IBE entry point (host or _dev) with buffers large enough for n elements"""
    on_g2 = name.endswith(("g2", "g2_dev"))
    buf = C.create_string_buffer(b"\x01" * 8192)
    p = None if null else C.cast(buf, C.c_void_p)
    dev = name.endswith("_dev")
    tail = [0, None] if dev else [0]
    if "encrypt" in name:
        return getattr(lib, name)(n, p, buf, 4, b"dst", 3, buf, buf, msg_len, p, buf, buf, buf, *tail)
    ksz = 48 if on_g2 else 96
    return getattr(lib, name)(n, p, ksz if stride is None else stride, buf, buf, buf, msg_len, buf, buf, *tail)


@pytest.mark.parametrize("name", _IBE + tuple(x + "_dev" for x in _IBE))
def test_ibe_entry_points_check_arguments_without_a_device(name):
    from kyber_amd import _lib

    lib = _lib.load()
    assert _call(lib, name, 0) == 0
    assert _call(lib, name, 0, msg_len=32) == 0
    assert _call(lib, name, 4, msg_len=33) == -1
    assert name.encode() in lib.kyb_last_error()
    assert _call(lib, name, 0, msg_len=33) == -1  # too long is an error whatever n is
    assert _call(lib, name, 4, null=True) == -1
    assert name.encode() in lib.kyb_last_error()
    if "decrypt" in name:
        assert _call(lib, name, 4, stride=47) == -1
        assert name.encode() in lib.kyb_last_error()
        assert _call(lib, name, 0, stride=0) == 0



@pytest.mark.parametrize("name", ("kyb_bls12381_ibe_encrypt_g1", "kyb_bls12381_ibe_encrypt_g2"))
def test_ibe_encrypt_takes_a_dst_of_at_most_255_bytes(name):
    """expand_message_xmd takes DSTs of at most 255 bytes: 256 is KYB_E_ARG on the C ABI (host and _dev, whatever n is)
    and ValueError in the Python wrapper, before anything reaches a device"""
    from kyber_amd import _lib
    from kyber_amd.pairing import bls12381 as bls

    lib = _lib.load()
    buf = C.create_string_buffer(b"\x01" * 8192)
    for dev in (False, True):
        fn = getattr(lib, name + ("_dev" if dev else ""))
        tail = [0, None] if dev else [0]
        for n, dl, want in ((0, 255, 0), (0, 256, -1), (4, 256, -1), (4, 1000, -1)):
            assert fn(n, buf, buf, 4, buf, dl, buf, buf, 16, buf, buf, buf, buf, *tail) == want, (dev, n, dl)
            if want:
                assert name.encode() in lib.kyb_last_error() and b"dst" in lib.kyb_last_error()
        assert fn(4, buf, buf, 4, None, 3, buf, buf, 16, buf, buf, buf, buf, *tail) == -1  # a length without a DST
    enc = bls.batch_ibe_encrypt_g2 if name.endswith("g2") else bls.batch_ibe_encrypt_g1
    master = bls.G2_BASE if name.endswith("g2") else bls.G1_BASE
    with pytest.raises(ValueError, match="DST"):
        enc(master, b"id", [b"m" * 8], sigmas=[b"s" * 8], dst=bytes(256))


def test_oracle_opens_drand_rounds_with_drand_keys_and_dsts(golden_dir):
    """drand's beacons are IBE private keys: sig_on_g1 (keys on G2, G1 signatures hashed under the G2 DST, identity
    sha256(BE64(round))) opens EncryptCCAonG2 to pk_g2 under that DST and not under the default G1 DST; sig_on_g2
    (chained: identity sha256(prev_sig || BE64(round))) opens EncryptCCAonG1 to pk_g1"""
    v = json.load(open(os.path.join(golden_dir, "bls12381_drand.json")))
    msg, sigma = b"drand round opens" + bytes(15), hashlib.sha256(b"sigma").digest()
    a = v["sig_on_g1"]
    pk, sig = bytes.fromhex(a["pk_g2"]), bytes.fromhex(a["sig_g1"])
    ident = hashlib.sha256(a["round"].to_bytes(8, "big")).digest()
    dst = v["dst_g2"].encode()
    assert IBE.decrypt(True, sig, *IBE.encrypt(True, pk, ident, msg, sigma, dst=dst)) == msg
    with pytest.raises(ValueError, match="rP check"):
        IBE.decrypt(True, sig, *IBE.encrypt(True, pk, ident, msg, sigma))
    b = v["sig_on_g2"]
    pk, sig = bytes.fromhex(b["pk_g1"]), bytes.fromhex(b["sig_g2"])
    ident = hashlib.sha256(bytes.fromhex(b["prev_sig"]) + b["round"].to_bytes(8, "big")).digest()
    assert v["dst_g2"].encode() == IBE.DOMAIN_G2
    assert IBE.decrypt(False, sig, *IBE.encrypt(False, pk, ident, msg[:17], sigma[:17])) == msg[:17]


# --------------------------------------------------------------------------- the hashing header on the CPU
_harness = None


def _lib():
    global _harness
    if _harness is None:
        out = os.path.join(ROOT, "tests", "_build", "libibeharness.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "ibe_harness.cpp")])
        _harness = C.CDLL(out)
    return _harness


def _h3_ref(sigma: bytes, msg: bytes):
    buf = hashlib.sha256(b"IBE-H3" + sigma + msg).digest()
    for i in range(1, 65535):
        h = bytearray(hashlib.sha256(i.to_bytes(2, "little") + buf).digest())
        h[0] >>= 1
        if int.from_bytes(h, "big") < O.R:
            return bytes(h), i
    raise AssertionError("rejection sampling failure")


def test_hashing_header_matches_hashlib():
    lib = _lib()
    rng = random.Random(2024)
    out = C.create_string_buffer(32)
    tries = {}
    for t in range(3000):
        ln = t % 33
        sigma, msg = rng.randbytes(ln), rng.randbytes(ln)
        gt = rng.randbytes(576)
        lib.ibe_h2(gt, out)
        assert out.raw == hashlib.sha256(b"IBE-H2" + gt).digest()
        lib.ibe_h4(sigma, ln, out)
        assert out.raw == hashlib.sha256(b"IBE-H4" + sigma).digest(), ln
        assert lib.ibe_h3(sigma, msg, ln, out) == 0
        r, i = _h3_ref(sigma, msg)
        assert out.raw == r, (ln, i)
        tries[i] = tries.get(i, 0) + 1
        lib.ibe_xor(msg.ljust(32, b"\0"), gt[:32], ln, out)
        assert out.raw == bytes(a ^ b for a, b in zip(msg, gt)) + bytes(32 - ln)
    assert tries.get(2, 0) > 100  # about 9 % of the first tries are rejected


def test_hashing_header_h3_beyond_the_second_try():
    """inputs whose first two or three candidates are all at least the order"""
    lib = _lib()
    out = C.create_string_buffer(32)
    found = {2: 0, 3: 0}
    k = 0
    while min(found.values()) < 3 and k < 200000:
        sigma = msg = k.to_bytes(4, "big")
        k += 1
        r, i = _h3_ref(sigma, msg)
        if i in found:
            found[i] += 1
            assert lib.ibe_h3(sigma, msg, 4, out) == 0 and out.raw == r, (k, i)
    assert min(found.values()) >= 3
