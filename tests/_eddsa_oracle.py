"""sign/eddsa's key expansion and Sign (curve.go:51-60, eddsa.go:43-142) restated with hashlib and Python integers; the
point comes from oracle/ed25519.py.  No GPU, no engine: the checker of kyb_ed25519_eddsa_expand and
kyb_ed25519_eddsa_sign, never the thing shipped.  Also the lines of the reference's sign.input that the tests share."""
import functools
import hashlib
import json
import os

import numpy as np

from oracle import ed25519 as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def expand(seed: bytes):
    """(secret, prefix, pub): the clamped, UNREDUCED first half of SHA-512(seed), its second half, secret B"""
    d = bytearray(hashlib.sha512(seed).digest())
    d[0] &= 0xF8
    d[31] &= 0x7F
    d[31] |= 0x40
    secret = bytes(d[:32])
    return secret, bytes(d[32:]), O.mul_base(secret)


def nonce(prefix: bytes, msg: bytes) -> int:
    return int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % O.L


def challenge(R: bytes, pub: bytes, msg: bytes) -> int:
    return int.from_bytes(hashlib.sha512(R + pub + msg).digest(), "little") % O.L


def sign(secret: bytes, prefix: bytes, pub: bytes, msg: bytes) -> bytes:
    """R || S; pub is hashed as its bytes stand"""
    r = nonce(prefix, msg)
    R = O.mul_base(r.to_bytes(32, "little"))
    S = (r + challenge(R, pub, msg) * int.from_bytes(secret, "little")) % O.L
    return R + S.to_bytes(32, "little")


# ---------------------------------------------------------------------------------------------------- shared vectors
@functools.lru_cache(maxsize=None)
def sign_input():
    """(seeds (1024, 32), kat (1024, 6, 32) with columns a, A, r, R, h, S, msgs [1024], sigs [1024]); message i is i
    bytes long"""
    from tests._cosi_cases import sign_input_roster

    seeds = np.load(os.path.join(GOLDEN, "eddsa_sign_input_seeds.npy"))
    kat = np.load(os.path.join(GOLDEN, "ed25519_sign_input.npy"))
    _, msgs, sigs = sign_input_roster()
    assert seeds.shape == (1024, 32) and seeds.dtype == np.uint8
    return seeds, kat, msgs, sigs


@functools.lru_cache(maxsize=None)
def sign_input_keys():
    """(secrets, prefixes, pubs), 1024 x 32 each: the oracle's expansion of every line's seed, computed once"""
    seeds = sign_input()[0]
    parts = [expand(bytes(s)) for s in seeds]
    return tuple(np.frombuffer(b"".join(p[k] for p in parts), dtype=np.uint8).reshape(-1, 32).copy() for k in range(3))


def rfc8032():
    """[(seed, pub, msg, sig)] of RFC 8032 section 7.1 (eddsa_test.go:24-51)"""
    rows = json.load(open(os.path.join(GOLDEN, "ed25519_misc.json")))["rfc8032"]
    return [tuple(bytes.fromhex(c[k]) for k in ("seed", "pub", "msg", "sig")) for c in rows]


# message lengths at which either hash changes its block count or its padding's place: the issue's list, and every
# length with (32 + len) mod 128 or (64 + len) mod 128 in {111, 112, 127, 0}
LISTED = (0, 1, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 175, 176, 191, 192, 207, 208, 239, 240, 1023)
BOUNDARY = tuple(sorted(set(LISTED) | {n for n in range(1024) for head in (32, 64) if (head + n) % 128 in (111, 112, 127, 0)}))
