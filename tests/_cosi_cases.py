"""The labelled table of the sign/cosi tests: rosters, masks and signatures, built once and used by the CPU tests (the
lane programs compiled for the host, the callers over the oracle) and by the GPU tests.  Every row's verdict and bytes
come from tests/_cosi_oracle.py; nothing here is taken from the code under test.

Rosters: m in SIZES covers every group edge of both table widths (4 and 8 keys) and every count of stray bits in the
last mask byte.  From m = 3 on a roster holds, at fixed slots, the identity, a point of order 8, a key plus torsion, one
key twice, P next to -P, the identity encoded with y = p + 1 (y >= p) and the identity as "-0"; roster "bad5" holds a
key with no x.
Masks: empty, full, every single bit, floor(m / 2) and floor(m / 2) + 1 keys (the two sides of the complement rule),
sparse and dense rows in turn (one wave holds both polarities), stray bits set above m, random.
Signatures: honest ones; r + l and r + 15 l (accepted); the four encodings of the identity as V with a signature made
for v = 0 (accepted, each hashed as given); one mask bit flipped, r altered, the message altered, V no curve point
(rejected); message lengths at the SHA-512 padding edges of a 64 + len byte input.

A key of unknown discrete logarithm can only be a torsion point here, and a torsion component T of the aggregate key
drops out of r B - k A exactly when 8 | k: honest signatures over such masks draw v (or, where v is fixed, extend the
message) until that holds."""
from __future__ import annotations

import functools
import hashlib
import os
import random
from collections import namedtuple

import numpy as np

from oracle import ed25519 as O
from tests import _cosi_oracle as CO

SIZES = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257)
MSG_LENS = (0, 47, 48, 63, 64, 65, 191, 192)  # SHA-512 padding edges of V || A || msg
MESSAGE = b"Hello World Cosi"

Key = namedtuple("Key", "enc a torsion")  # a: the discrete logarithm of the key's prime-order part
Row = namedtuple("Row", "label mask msg sig")  # mask: (m + 7) >> 3 bytes; sig: V || r


def _h(*parts) -> int:
    return int.from_bytes(hashlib.sha512(b"|".join(str(p).encode() for p in parts)).digest(), "little")


@functools.lru_cache(maxsize=None)
def plain_key(j: int) -> Key:
    a = _h("cosi-key", j) % O.L
    return Key(O.encode(CO.mul_base_int(a)), a, False)


@functools.lru_cache(maxsize=None)
def order8():
    """a point of order 8: the torsion part [l]Q of the first decodable y whose torsion part has full order"""
    y = 2
    while True:
        q = O.decode(y.to_bytes(32, "little"))
        if q is not None:
            t = O.mul_int(O.L, q)
            if O.mul_int(4, t) != O.IDENTITY:
                return t
        y += 1


def not_a_point() -> bytes:
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


IDENTITY_ENCODINGS = (  # 01.., the same with the sign bit, p + 1, that with the sign bit
    (1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little"),
    (O.P + 1).to_bytes(32, "little"), ((O.P + 1) | 1 << 255).to_bytes(32, "little"))


@functools.lru_cache(maxsize=None)
def roster(m: int):
    """the m keys of roster m: plain keys with the special ones at fixed slots, as far as m reaches"""
    keys = [plain_key(j) for j in range(m)]
    special = {
        1: Key(IDENTITY_ENCODINGS[0], 0, False),
        2: Key(O.encode(order8()), 0, True),
        3: Key(O.encode(CO.padd(O.decode(plain_key(3).enc), order8())), plain_key(3).a, True),
        4: plain_key(0),
        6: Key(O.encode(O.neg(O.decode(plain_key(5).enc))), O.L - plain_key(5).a, False),
        7: Key(IDENTITY_ENCODINGS[2], 0, False),
        8: Key(IDENTITY_ENCODINGS[1], 0, False),
    }
    for slot, k in special.items():
        if slot < m:
            keys[slot] = k
    return tuple(keys)


def bad_roster():
    keys = list(roster(5))
    keys[2] = Key(not_a_point(), 0, False)
    return tuple(keys)


def publics(keys):
    return [k.enc for k in keys]


def mask_of(m: int, bits) -> bytes:
    b = bytearray(CO.mask_len(m))
    for j in bits:
        b[j >> 3] |= 1 << (j & 7)
    return bytes(b)


def honest(keys, mask: bytes, msg: bytes, tag, v=None, Vb=None):
    """(msg, V || r) that verifies under (keys, mask).  v None: drawn until a torsion part of the aggregate key drops
    out; v given (with Vb, the encoding of v B to hash): the message grows by a counter byte string instead."""
    on = CO.enabled(mask, len(keys))
    a_sum = sum(keys[j].a for j in on) % O.L
    tors = any(keys[j].torsion for j in on)
    A, _ = CO.aggregate(publics(keys), mask)
    v0 = _h("cosi-v", tag) % O.L if v is None else v
    Vp = O._ext(CO.mul_base_int(v0)) if Vb is None else None
    for t in range(1000):
        vv = (v0 + t) % O.L if v is None else v
        if Vb is None:  # (v0 + t) B, one addition further each time
            V = O.encode(O._aff(Vp))
            Vp = O._ext_add(Vp, O._ext(O.B))
        else:
            V = Vb
        m2 = msg if v is None or t == 0 else msg + b"#%d" % t
        k = CO.challenge_int(V, A, m2)
        if tors and k % 8:
            continue
        return m2, V + ((vv + k * a_sum) % O.L).to_bytes(32, "little")
    raise AssertionError("no challenge divisible by 8")


def masks_of(m: int):
    """[(label, mask bytes)] of roster size m"""
    rng = random.Random(1000 + m)
    out = [("empty", mask_of(m, [])), ("full", mask_of(m, range(m)))]
    out += [("single", mask_of(m, [j])) for j in range(m)]
    out += [("half", mask_of(m, rng.sample(range(m), m // 2))), ("half+1", mask_of(m, rng.sample(range(m), m // 2 + 1)))]
    for t in range(4):  # sparse and dense in turn
        few = rng.sample(range(m), min(m, 1 + t % 2))
        out.append(("sparse", mask_of(m, few)) if t % 2 == 0 else ("dense", mask_of(m, set(range(m)) - set(few))))
    if m & 7:  # stray bits above m in the last byte, over a sparse and over a dense mask
        for label, bits in (("stray", rng.sample(range(m), (m + 2) // 3)), ("stray-full", range(m))):
            b = bytearray(mask_of(m, bits))
            b[-1] |= (0xFF << (m & 7)) & 0xFF
            out.append((label, bytes(b)))
    out += [("random", mask_of(m, [j for j in range(m) if rng.random() < 0.5])) for _ in range(3)]
    return out


@functools.lru_cache(maxsize=None)
def rows(name):
    """the rows of roster `name`: a size of SIZES, or "bad5" """
    if name == "bad5":
        keys = bad_roster()
        good = roster(5)
        return tuple(Row("undecodable-key/" + label, mask, *honest(good, mask, MESSAGE, ("bad", i)))
                     for i, (label, mask) in enumerate(masks_of(5)[:12]))
    m = int(name)
    keys = roster(m)
    out = []
    for i, (label, mask) in enumerate(masks_of(m)):
        out.append(Row("honest/" + label, mask, *honest(keys, mask, MESSAGE, (m, i))))
    rng = random.Random(2000 + m)
    base_mask = mask_of(m, rng.sample(range(m), (m + 1) // 2))
    msg, sig = honest(keys, base_mask, MESSAGE, (m, "base"))
    r = int.from_bytes(sig[32:], "little")
    for label, rr in (("r+l", r + O.L), ("r+15l", r + 15 * O.L)):
        assert rr < 1 << 256
        out.append(Row(label, base_mask, msg, sig[:32] + rr.to_bytes(32, "little")))
    for e, Vb in enumerate(IDENTITY_ENCODINGS):
        out.append(Row("identity-V/%d" % e, base_mask, *honest(keys, base_mask, MESSAGE, None, v=0, Vb=Vb)))
    flip = bytearray(base_mask)
    flip[0] ^= 1
    out.append(Row("mask-bit-flipped", bytes(flip), msg, sig))
    out.append(Row("r-altered", base_mask, msg, sig[:32] + ((r + 1) % O.L).to_bytes(32, "little")))
    out.append(Row("msg-altered", base_mask, msg + b"!", sig))
    out.append(Row("V-not-a-point", base_mask, msg, not_a_point() + sig[32:]))
    for ln in MSG_LENS:
        body = bytes((7 * ln + t) & 0xFF for t in range(ln))
        out.append(Row("msg-len/%d" % ln, base_mask, *honest(keys, base_mask, body, (m, "len", ln))))
        out.append(Row("msg-len-altered/%d" % ln, base_mask, out[-1].msg, out[-1].sig[:32] + sig[32:]))
    return tuple(out)


def keys_of(name):
    return bad_roster() if name == "bad5" else roster(int(name))


NAMES = tuple(str(m) for m in SIZES) + ("bad5",)


@functools.lru_cache(maxsize=None)
def expected(name):
    """[(ok, agg, count, status)] of rows(name), from the oracle, computed once"""
    pub = publics(keys_of(name))
    return tuple(CO.abi_cosi_verify(pub, r.msg, r.sig, r.mask) for r in rows(name))


def take(name, n: int):
    """n rows of the table, the table's rows repeated in turn, with their expectations"""
    rs, ex = rows(name), expected(name)
    return [rs[i % len(rs)] for i in range(n)], [ex[i % len(rs)] for i in range(n)]


def pack_masks(rs, m: int, stride: int) -> np.ndarray:
    """(n, stride) bytes: each row's mask, the slack beyond it set to ones (nobody may read it)"""
    L = CO.mask_len(m)
    a = np.full((len(rs), stride), 0xFF, dtype=np.uint8)
    for i, r in enumerate(rs):
        a[i, :L] = np.frombuffer(r.mask, dtype=np.uint8)
    return a


def pack_sigs(rs) -> np.ndarray:
    return np.frombuffer(b"".join(r.sig for r in rs), dtype=np.uint8).reshape(len(rs), 64).copy()


def pack_roster(name) -> np.ndarray:
    return np.frombuffer(b"".join(publics(keys_of(name))), dtype=np.uint8).reshape(-1, 32).copy()


# ------------------------------------------------------------------------------------------------ the EdDSA pins
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def sign_input_roster():
    """(pubs [1024], msgs [1024], sigs [1024]) of the reference's sign.input: keys and signatures of all 1024 lines from
    ed25519_sign_input.npy (columns: a, A, r, R, h, S), the messages of lines 0..383 and 384..1023 from the two message
    fixtures (tests/golden/make_golden_ed25519_verify.py, make_golden_cosi.py)"""
    kat = np.load(os.path.join(GOLDEN, "ed25519_sign_input.npy"))
    msgs = []
    for f in ("ed25519_sign_input_msgs.npz", "ed25519_sign_input_msgs_tail.npz"):
        z = np.load(os.path.join(GOLDEN, f))
        off, blob = z["off"], z["msgs"].tobytes()
        msgs += [blob[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    assert len(msgs) == len(kat) == 1024 and all(len(m) == i for i, m in enumerate(msgs))
    return ([kat[i, 1].tobytes() for i in range(1024)], msgs, [kat[i, 3].tobytes() + kat[i, 5].tobytes() for i in range(1024)])


# ------------------------------------------------------------------------------------------------ the reference's scenarios
def scenario(n: int, f: int, seed: int = 0):
    """testCoSi(n, f) (cosi_test.go:69-158) with seeded scalars: (privates, publics, message, signature, threshold or None)"""
    kp = [plain_key(100 + seed * 16 + i) for i in range(n)]
    privates, pubs = [k.a for k in kp], [k.enc for k in kp]
    signers = list(range(n - f))
    sig = CO.cosign(privates, pubs, signers, MESSAGE, [_h("scenario", n, f, seed, i) % O.L for i in signers])
    return privates, pubs, MESSAGE, sig, (None if f == 0 else n - f)


SCENARIOS = ((2, 0), (5, 0), (5, 2), (5, 4))
