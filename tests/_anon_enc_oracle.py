"""CPU ORACLE (test infrastructure) -- the reference's sign/anon Encrypt / Decrypt (enc.go) restated sequentially in
Python integers on oracle/ed25519.py and the host BLAKE2Xb (kyber_amd/util/blake2xb.py).  The checker of the anon
encryption tests, never the thing shipped.

What the restatement keeps of enc.go:
  * key.Pair.Gen calls the suite's NewKey (curve.go:51-76): 32 stream bytes, SHA-512, clamped, stored UNREDUCED; X = x B
    and, in Encrypt, every x Y_i use those bytes (geScalarMult's value, oracle mul / mul_base);
  * the master secret xb = Private.MarshalBinary() is x REDUCED mod l; the slots carry xb and XOF(xb) is the message stream;
  * Decrypt unmarshals xb as a scalar (32 bytes copied, no reduction, no range check) and multiplies by THOSE bytes, so a
    ring member with a torsion component makes Decrypt reject what Encrypt made;
  * the raw first 32 bytes of the ciphertext go back into the regenerated header: a non-canonical X that decodes is not
    rejected for that alone; x B = X is compared on canonical bytes (point.go:81-95);
  * the order of Decrypt's checks (enc.go:55-101, 175-190) is the precedence of the status values.
A ring member that does not decode has no counterpart in the reference (its Set holds decoded points): the engine's rule
is KYB_ST_BAD_POINT -- in an open behind the checks that do not touch the ring (the two lengths and X), in front of the
two that do -- and the oracle states the same.
"""
from __future__ import annotations

import hashlib

from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests._anon_oracle import canon_bytes, point_pick, scalar_pick

L = O.L
MAC = 16
ST_OK, ST_BAD_POINT, ST_SHORT, ST_INVALID, ST_MAC = 0, 1, 11, 12, 13
ERR = {ST_BAD_POINT: "invalid Ed25519 curve point", ST_SHORT: "ciphertext too short", ST_INVALID: "invalid ciphertext",
       ST_MAC: "invalid ciphertext: failed MAC check"}


# Products somebody computed before, (scalar bytes, point bytes or None for the base) -> encoding: the large batches of
# tests/_anon_enc_cases.py fill it from the oracle's C restatement (tests/_oracle_c.py), which tests hold to oracle/ed25519.py
PRODUCTS: dict = {}


def _mul(a: bytes, P: bytes):
    return PRODUCTS.get((a, P)) or O.mul(a, P)


def _mul_base(a: bytes) -> bytes:
    return PRODUCTS.get((a, None)) or O.mul_base(a)


def new_key(stream) -> bytes:
    """Curve.NewKey (curve.go:62-76): random.Bytes(32), SHA-512, clamp; the 32 bytes as stored, unreduced"""
    d = bytearray(hashlib.sha512(stream.XORKeyStream(bytes(32))).digest()[:32])
    d[0] &= 0xF8
    d[31] &= 0x7F
    d[31] |= 0x40
    return bytes(d)


def reduced(x: bytes) -> bytes:
    """Scalar.MarshalBinary: the value mod l"""
    return (int.from_bytes(x, "little") % L).to_bytes(32, "little")


def xor(a: bytes, b: bytes) -> bytes:
    return bytes(p ^ q for p, q in zip(a, b))


def slot(x: bytes, Y: bytes, xb: bytes):
    """one header slot (enc.go:17-25): xb XOR XOF(MarshalBinary(x Y))[0:32]; None when Y does not decode"""
    S = _mul(x, Y)
    return None if S is None else blake2xb.New(S).XORKeyStream(xb)


def body(xb: bytes, message: bytes) -> bytes:
    """ctx || mac (enc.go:127-145)"""
    ctx = blake2xb.New(xb).XORKeyStream(message)
    return ctx + blake2xb.New(ctx).Read(MAC)


def seal(message: bytes, keys, x: bytes):
    """(ciphertext, status) of kyb_ed25519_anon_seal for one message under the ephemeral scalar bytes x: an all-zero
    slot and KYB_ST_BAD_POINT where a ring member does not decode"""
    xb = reduced(x)
    slots = [slot(x, Y, xb) for Y in keys]
    if any(s is None for s in slots):
        return bytes(48 + 32 * len(keys) + len(message)), ST_BAD_POINT
    return _mul_base(x) + b"".join(slots) + body(xb, message), ST_OK


def encrypt(message: bytes, keys, rand) -> bytes:
    """Encrypt (enc.go:123-148) with suite.RandomStream() = rand"""
    ct, st = seal(message, keys, new_key(rand))
    assert st == ST_OK
    return ct


def open_(ct: bytes, keys, mine: int, priv: bytes):
    """(plaintext or None, status) of Decrypt (enc.go:165-192) in the order of its checks"""
    ring = len(keys)
    if not 0 <= mine < ring:
        raise ValueError("private-key index out of range")
    if len(ct) < 32:
        return None, ST_SHORT
    Xb = ct[:32]
    if O.decode(Xb) is None:
        return None, ST_BAD_POINT
    hdrlen = 32 + 32 * ring
    if len(ct) < hdrlen:
        return None, ST_SHORT
    if any(O.decode(Y) is None for Y in keys):  # (the engine's rule: before the ring is touched)
        return None, ST_BAD_POINT
    xb = blake2xb.New(_mul(priv, Xb)).XORKeyStream(ct[32 + 32 * mine:64 + 32 * mine])
    if _mul_base(xb) != canon_bytes(Xb):
        return None, ST_INVALID
    if Xb + b"".join(slot(xb, Y, xb) for Y in keys) != ct[:hdrlen]:
        return None, ST_INVALID
    if len(ct) < hdrlen + MAC:
        return None, ST_SHORT
    ctx, mac = ct[hdrlen:len(ct) - MAC], ct[len(ct) - MAC:]
    if blake2xb.New(ctx).Read(MAC) != mac:
        return None, ST_MAC
    return blake2xb.New(xb).XORKeyStream(ctx), ST_OK


def decrypt(ct: bytes, keys, mine: int, priv: bytes) -> bytes:
    msg, st = open_(ct, keys, mine, priv)
    if st:
        raise ValueError(ERR[st])
    return msg


GOLDEN_MESSAGE = b"Hello World!"


def golden_keys(name: str):
    """(keys, mine, x, rand) of one example of enc_test.go: its key generation replayed under blake2xb.New(nil), rand
    left where the example's Encrypt finds it"""
    r = blake2xb.New(b"")
    if name == "ExampleEncrypt_one":
        x = scalar_pick(r)
        return [O.mul_base(x)], 0, x, r
    assert name == "ExampleEncrypt_anonSet"
    keys = [point_pick(r) for _ in range(3)]
    x = scalar_pick(r)
    keys[1] = O.mul_base(x)
    return keys, 1, x, r


# ------------------------------------------------------------------------------------------------- labelled cases
def _rng_bytes(tag: str, n: int) -> bytes:
    return blake2xb.New(b"anon-enc-cases/" + tag.encode()).Read(n)


def keypair(tag: str):
    x = reduced(_rng_bytes("key/" + tag, 32))
    return x, O.mul_base(x)


def torsion_point() -> bytes:
    """a point of order 8: l times the first curve point that leaves one"""
    y = 2
    while True:
        pt = O.decode(y.to_bytes(32, "little"))
        if pt is not None:
            t = O.mul_int(L, pt)
            if t != O.IDENTITY and O.mul_int(4, t) != O.IDENTITY:
                return O.encode(t)
        y += 1


def undecodable() -> bytes:
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


# An ephemeral scalar whose X = x B is the identity (x = l, unreduced: xb = 0): the one X with non-canonical encodings
# that still decode to it -- the sign bit set on x = 0, and y + p -- so a ciphertext that stays VALID with either.
X_IS_L = L.to_bytes(32, "little")
IDENTITY_NONCANONICAL = (bytes([1]) + bytes(30) + bytes([0x80]), (2**255 - 18).to_bytes(32, "little"))
