"""Host-side mirror of ``encrypt/ibe`` (ibe.go:51-232): the Boneh-Franklin CCA identity-based encryption that drand's
timelock encryption (tlock) runs on, on BLS12-381 with the suite hash SHA-256, over the engine's fused batch calls
(kyb_bls12381_ibe_encrypt_g1/g2, kyb_bls12381_ibe_decrypt_g1/g2).

OnG1 (master key and U on G1, identities and private keys on G2): drand's "chained" / "unchained" networks.
OnG2 (master key and U on G2, identities and private keys on G1): drand quicknet, the current tlock network.

The single-ciphertext functions raise ValueError where the reference returns an error.  The batch forms take messages
of mixed lengths and issue one engine call per length; a decrypt of a malformed ciphertext (len(V) != len(W), or W
longer than 32 bytes) yields None with status ST_MALFORMED without reaching the device.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..pairing import bls12381 as _bls

ST_OK, ST_BAD_POINT, ST_NOT_IN_SUBGROUP, ST_IBE_CHECK, ST_IBE_H3 = 0, 1, 2, 3, 4  # include/kyber_hip.h
ST_MALFORMED = 255  # Python side only: the reference's "ciphertext too long" / "XorSigma is of invalid length"
_ERRORS = {ST_BAD_POINT: "point does not unmarshal", ST_NOT_IN_SUBGROUP: "point not in the prime-order subgroup",
           ST_IBE_CHECK: "invalid proof: rP check failed", ST_IBE_H3: "rejection sampling failure",
           ST_MALFORMED: "ciphertext too long or XorSigma of invalid length"}


@dataclass(frozen=True)
class Ciphertext:
    """encrypt/ibe Ciphertext (ibe.go:20-27): U on the master key's group, V = sigma ^ H2(Gid^r), W = msg ^ H4(sigma)."""
    U: bytes
    V: bytes
    W: bytes


def _encrypt_batch(on_g2: bool, master: bytes, ident: bytes, msgs, sigmas, dst):
    enc = _bls.batch_ibe_encrypt_g2 if on_g2 else _bls.batch_ibe_encrypt_g1
    dst = dst if dst is not None else (_bls.DOMAIN_G1 if on_g2 else _bls.DOMAIN_G2)
    msgs = [bytes(m) for m in msgs]
    if any(len(m) > 32 for m in msgs):
        raise ValueError("plaintext too long for the hash function provided")
    out = [None] * len(msgs)
    by_len = {}
    for i, m in enumerate(msgs):
        by_len.setdefault(len(m), []).append(i)
    for ln, idx in by_len.items():
        sg = None if sigmas is None else [bytes(sigmas[i]) for i in idx]
        U, V, W, st = enc(bytes(master), bytes(ident), np.frombuffer(b"".join(msgs[i] for i in idx), dtype=np.uint8).reshape(len(idx), ln),
                          sigmas=sg, dst=dst)
        if np.asarray(st).any():
            raise ValueError(_ERRORS.get(int(np.asarray(st).max()), "encryption failed"))
        for k, i in enumerate(idx):
            out[i] = Ciphertext(bytes(U[k]), bytes(V[k]), bytes(W[k]))
    return out


def _decrypt_batch(on_g2: bool, privates, cts):
    """(msgs, status): msgs[i] is None where status[i] != 0.  privates: one key (bytes) for every ciphertext or one each."""
    dec = _bls.batch_ibe_decrypt_g2 if on_g2 else _bls.batch_ibe_decrypt_g1
    usz = 96 if on_g2 else 48
    shared = isinstance(privates, (bytes, bytearray))
    n = len(cts)
    msgs, status = [None] * n, np.zeros(n, dtype=np.uint8)
    by_len = {}
    for i, c in enumerate(cts):
        if len(c.W) > 32 or len(c.V) != len(c.W):
            status[i] = ST_MALFORMED
        elif len(c.U) != usz:
            status[i] = ST_BAD_POINT
        else:
            by_len.setdefault(len(c.W), []).append(i)
    for ln, idx in by_len.items():
        keys = bytes(privates) if shared else [bytes(privates[i]) for i in idx]
        m, st = dec(keys, [cts[i].U for i in idx], np.frombuffer(b"".join(cts[i].V for i in idx), dtype=np.uint8).reshape(len(idx), ln),
                    np.frombuffer(b"".join(cts[i].W for i in idx), dtype=np.uint8).reshape(len(idx), ln))
        for k, i in enumerate(idx):
            status[i] = st[k]
            if not st[k]:
                msgs[i] = bytes(m[k])
    return msgs, status


def batch_encrypt_cca_on_g1(master: bytes, ident: bytes, msgs, sigmas=None, dst: bytes = None):
    """EncryptCCAonG1 (ibe.go:51-98) of many messages to one identity: a list of Ciphertext"""
    return _encrypt_batch(False, master, ident, msgs, sigmas, dst)


def batch_encrypt_cca_on_g2(master: bytes, ident: bytes, msgs, sigmas=None, dst: bytes = None):
    """EncryptCCAonG2 (ibe.go:137-185)"""
    return _encrypt_batch(True, master, ident, msgs, sigmas, dst)


def batch_decrypt_cca_on_g1(privates, cts):
    """DecryptCCAonG1 (ibe.go:100-135) of many ciphertexts: (messages or None, status)"""
    return _decrypt_batch(False, privates, cts)


def batch_decrypt_cca_on_g2(privates, cts):
    """DecryptCCAonG2 (ibe.go:187-232)"""
    return _decrypt_batch(True, privates, cts)


def encrypt_cca_on_g1(master: bytes, ident: bytes, msg: bytes, dst: bytes = None) -> Ciphertext:
    return batch_encrypt_cca_on_g1(master, ident, [msg], dst=dst)[0]


def encrypt_cca_on_g2(master: bytes, ident: bytes, msg: bytes, dst: bytes = None) -> Ciphertext:
    return batch_encrypt_cca_on_g2(master, ident, [msg], dst=dst)[0]


def _one(res) -> bytes:
    (m,), st = res
    if st[0]:
        raise ValueError(_ERRORS.get(int(st[0]), "decryption failed"))
    return m


def decrypt_cca_on_g1(private: bytes, c: Ciphertext) -> bytes:
    return _one(batch_decrypt_cca_on_g1(bytes(private), [c]))


def decrypt_cca_on_g2(private: bytes, c: Ciphertext) -> bytes:
    return _one(batch_decrypt_cca_on_g2(bytes(private), [c]))
