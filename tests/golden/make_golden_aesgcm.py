#!/usr/bin/env python3
"""Writes tests/golden/aes256gcm.json: AES-256-GCM (12-byte nonce, no additional data) outputs of the build machine's
OpenSSL (libcrypto.so.3 through ctypes' EVP calls), which pin the pure-Python AES-GCM of tests/_ecies_oracle.py and the
device header kyber_amd/csrc/aes256gcm.cuh.  Cases: the GCM specification's 256-bit test cases 13 and 14 (zero key and
nonce; empty plaintext, one zero block) with their published outputs asserted here, and a seeded random key, nonce and
plaintext at every length of _ecies_oracle.LENGTHS.  Also HKDF-SHA256 of RFC 5869 test case 3, asserted against the RFC.
The tests read only the JSON; nothing calls libcrypto at test time.

  python tests/golden/make_golden_aesgcm.py"""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._ecies_oracle import LENGTHS, hkdf_sha256  # noqa: E402

lib = C.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
lib.EVP_aes_256_gcm.restype = C.c_void_p
lib.EVP_EncryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
lib.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
lib.EVP_EncryptFinal_ex.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
lib.EVP_CIPHER_CTX_ctrl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def seal(key: bytes, nonce: bytes, msg: bytes) -> bytes:
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        assert lib.EVP_EncryptInit_ex(ctx, lib.EVP_aes_256_gcm(), None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, 12, None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        out, n = C.create_string_buffer(len(msg) + 32), C.c_int(0)
        ct = b""
        if msg:
            assert lib.EVP_EncryptUpdate(ctx, out, C.byref(n), msg, len(msg)) == 1
            ct = out.raw[:n.value]
        assert lib.EVP_EncryptFinal_ex(ctx, out, C.byref(n)) == 1
        ct += out.raw[:n.value]
        tag = C.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        return ct + tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def main():
    cases = []
    spec = [("gcm-spec test case 13", b"", "530f8afbc74536b9a963b4f1c4cb738b"),
            ("gcm-spec test case 14", bytes(16), "cea7403d4d606b6e074ec5d3baf39d18d0d1c8a799996bf0265b98b5d48ab919")]
    for name, msg, want in spec:
        got = seal(bytes(32), bytes(12), msg)
        assert got.hex() == want, (name, got.hex())
        cases.append({"name": name, "key": bytes(32).hex(), "nonce": bytes(12).hex(), "msg": msg.hex(), "sealed": got.hex()})
    for ln in LENGTHS:
        stream = hashlib.shake_256(b"aes256gcm golden %d" % ln).digest(44 + ln)
        key, nonce, msg = stream[:32], stream[32:44], stream[44:]
        cases.append({"name": "random, %d bytes" % ln, "key": key.hex(), "nonce": nonce.hex(), "msg": msg.hex(),
                      "sealed": seal(key, nonce, msg).hex()})
    okm = "8da4e775a563c18f715f802a063c5a31b8a11f5c5ee1879ec3454e5f3c738d2d9d201395faa4b61a96c8"
    assert hkdf_sha256(bytes([0x0B]) * 22, 42).hex() == okm
    doc = {"source": "OpenSSL libcrypto EVP_aes_256_gcm, 12-byte nonce, no additional data; sealed = ciphertext || tag",
           "aes256gcm": cases,
           "hkdf_sha256": [{"name": "RFC 5869 test case 3", "ikm": (bytes([0x0B]) * 22).hex(), "length": 42, "okm": okm}]}
    with open(os.path.join(HERE, "aes256gcm.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
