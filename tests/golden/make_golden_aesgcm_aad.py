#!/usr/bin/env python3
"""Writes tests/golden/aes256gcm_aad.json: AES-256-GCM with additional data, outputs of the build machine's OpenSSL
(libcrypto through ctypes' EVP calls, as tests/golden/make_golden_aesgcm.py), which pin the GCM of tests/_vss_oracle.py
and gcm_seal_aad / gcm_open_aad of kyber_amd/csrc/aes256gcm.cuh.  Cases: the GCM specification's 256-bit test case 16
(60 bytes of plaintext, 20 of additional data; its published tag is asserted here) and, at every plaintext length of
_ecies_oracle.LENGTHS, a seeded random key and plaintext under the all-zero nonce with 32 bytes of additional data and again with
128: the shapes of share/vss/pedersen's and share/vss/rabin's deals.  The tests read only the JSON; nothing calls libcrypto at test time.

  python tests/golden/make_golden_aesgcm_aad.py"""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._ecies_oracle import LENGTHS  # noqa: E402

lib = C.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
lib.EVP_aes_256_gcm.restype = C.c_void_p
lib.EVP_EncryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
lib.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
lib.EVP_EncryptFinal_ex.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
lib.EVP_CIPHER_CTX_ctrl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def seal(key: bytes, nonce: bytes, msg: bytes, aad: bytes) -> bytes:
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        assert lib.EVP_EncryptInit_ex(ctx, lib.EVP_aes_256_gcm(), None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, 12, None) == 1
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        out, n = C.create_string_buffer(len(msg) + 32), C.c_int(0)
        if aad:  # additional data: an update with no output buffer
            assert lib.EVP_EncryptUpdate(ctx, None, C.byref(n), aad, len(aad)) == 1
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
    key = bytes.fromhex("feffe9928665731c6d6a8f9467308308" * 2)
    nonce = bytes.fromhex("cafebabefacedbaddecaf888")
    msg = bytes.fromhex("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a72"
                        "1c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b39")
    aad = bytes.fromhex("feedfacedeadbeeffeedfacedeadbeefabaddad2")
    got = seal(key, nonce, msg, aad)
    assert got[-16:].hex() == "76fc6ece0f4e1768cddf8853bb2d551b", got.hex()
    cases = [{"name": "gcm-spec test case 16", "key": key.hex(), "nonce": nonce.hex(), "aad": aad.hex(), "msg": msg.hex(),
              "sealed": got.hex()}]
    for ln in LENGTHS:
        stream = hashlib.shake_256(b"aes256gcm aad golden %d" % ln).digest(64 + ln)
        key, aad, msg = stream[:32], stream[32:64], stream[64:]
        cases.append({"name": "random, zero nonce, %d bytes" % ln, "key": key.hex(), "nonce": bytes(12).hex(), "aad": aad.hex(),
                      "msg": msg.hex(), "sealed": seal(key, bytes(12), msg, aad).hex()})
    for ln in LENGTHS:  # share/vss/rabin's shape: the context is 128 bytes of the suite's XOF
        stream = hashlib.shake_256(b"aes256gcm aad128 golden %d" % ln).digest(160 + ln)
        key, aad, msg = stream[:32], stream[32:160], stream[160:]
        cases.append({"name": "random128, zero nonce, %d bytes" % ln, "key": key.hex(), "nonce": bytes(12).hex(), "aad": aad.hex(),
                      "msg": msg.hex(), "sealed": seal(key, bytes(12), msg, aad).hex()})
    doc = {"source": "OpenSSL libcrypto EVP_aes_256_gcm, 12-byte nonce, with additional data; sealed = ciphertext || tag",
           "aes256gcm_aad": cases}
    with open(os.path.join(HERE, "aes256gcm_aad.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
