"""The labelled table of kyb_ed25519_lincomb cases, shared by tests/test_proof_host.py (the lane program on the CPU) and
tests/test_gpu_lincomb.py (the kernels), and the oracle's statement of the call.

A batch is (name, shared, rows): `shared` the ks encodings the batch shares (the bytes of a nil term are junk on
purpose: they must not be read); a row is (label, scalars, own, kind) with ko + ks scalars, ko own encodings and the
kind of `expect` the row is checked with (EXPECT_KINDS).  value() is the sum as the reference computes it term by term:
Mul under the flag for own and shared points (oracle.ed25519.mul: unreduced scalars and the >= 2^255 behaviour
included), geScalarMultBase's value for a nil term whatever the flag (point.go:243)."""
import functools
import random

from oracle import ed25519 as O
from tests import _ed_verify_oracle as V

L = O.L
ST_BAD_POINT = 1
IDENT = O.encode(O.IDENTITY)
BASE = O.encode(O.B)
SPECIAL = (L, L + 1, 2**255 - 1, 2**255, 2**256 - 1)
EXPECT_KINDS = ("equal", "noncanonical", "sign", "off curve")
FULL_GRID = {(1, 2, 0), (1, 2, 1), (1, 2, 2), (1, 2, 3), (2, 2, 1), (4, 4, 5)}  # (ko, ks, nil_mask): every special scalar in every slot


def sc(v: int) -> bytes:
    return (v % L).to_bytes(32, "little")


def raw(v: int) -> bytes:
    return (v % 2**256).to_bytes(32, "little")


_mul_cached = functools.lru_cache(maxsize=None)(O.mul)
_mul_base = functools.lru_cache(maxsize=None)(O.mul_base)


def _mul(s: bytes, pt: bytes, vartime: bool):
    return _mul_cached(s, pt, vartime and s[31] >= 0x80)  # below 2^255 both flag values multiply by the scalar itself


def value(ko, ks, nil_mask, shared, scalars, own, vartime):
    """the 32 bytes of the sum, or None where an own point or a shared point that is used does not decode"""
    acc, bad = O.IDENTITY, False
    for j in range(ko + ks):
        s = bytes(scalars[j])
        if j < ko:
            t = _mul(s, bytes(own[j]), vartime)
        elif nil_mask >> (j - ko) & 1:
            t = _mul_base(s)
        else:
            t = _mul(s, bytes(shared[j - ko]), vartime)
        if t is None:
            bad = True
        else:
            acc = O.add(acc, O.decode(t))
    return None if bad else O.encode(acc)


def verdict(v, expect):
    """(ok, status) of one element whose sum is v (None: a point did not decode) against expect's 32 bytes"""
    if v is None:
        return 0, ST_BAD_POINT
    t = O.decode(bytes(expect))
    return int(t is not None and O.encode(t) == v), 0


def _off_curve(rng) -> bytes:
    while True:
        e = rng.getrandbits(255).to_bytes(32, "little")
        if O.decode(e) is None:
            return e


OFF_CURVE = _off_curve(random.Random(62))


def noncanonical(enc: bytes):
    """another encoding of the same point, or None when it has one encoding only: y + p where that fits 255 bits, and
    the other sign where x = 0"""
    n = int.from_bytes(enc, "little")
    sign, y = n >> 255, n & (2**255 - 1)
    x = O.decode(enc)[0]
    if y + O.P < 2**255:
        return (y + O.P | sign << 255).to_bytes(32, "little")
    if x == 0:
        return (y | (sign ^ 1) << 255).to_bytes(32, "little")
    return None


def kind_checked(kind: str, v) -> str:
    """what a row of this kind checks when its sum is v: a point with one encoding only (nearly every point: y + p must
    fit 255 bits, or x be 0) has no non-canonical expect, and the row is an "equal" row"""
    return "equal" if kind == "noncanonical" and v is not None and noncanonical(v) is None else kind


def expect_bytes(kind: str, v):
    """the expect column of a row whose sum is v, for kind_checked(kind, v).  "sign" flips bit 255, which names another
    point unless x = 0"""
    kind = kind_checked(kind, v)
    if v is None:
        return IDENT
    if kind == "equal":
        return v
    if kind == "noncanonical":
        return noncanonical(v)
    if kind == "sign":
        return v[:31] + bytes([v[31] ^ 0x80])
    assert kind == "off curve"
    return OFF_CURVE


def _small_order():
    small = [bytes.fromhex(h) for h in V._misc()["small_order"]]
    order8 = [s for s in small if O.mul_int(4, O.decode(s)) != O.IDENTITY]
    order4 = [s for s in small if O.mul_int(2, O.decode(s)) != O.IDENTITY and O.mul_int(4, O.decode(s)) == O.IDENTITY]
    assert order8 and order4
    return order8, order4


@functools.lru_cache(maxsize=None)
def batches(ko: int, ks: int, nil_mask: int):
    """[(name, shared, rows)] for one shape"""
    K = ko + ks
    rng = random.Random(1000 * ko + 100 * ks + nil_mask)
    order8, order4 = _small_order()
    junk = bytes([0xA5]) * 31 + bytes([0x7F])  # what a nil slot holds: no curve point, y above p
    nil = lambda j: bool(nil_mask >> j & 1)
    pt = lambda: O.encode(O.mul_int(rng.getrandbits(250) + 1, O.B))
    scs = lambda: [sc(rng.getrandbits(256)) for _ in range(K)]
    owns = lambda: [pt() for _ in range(ko)]
    kinds = iter(EXPECT_KINDS * 1000)
    shared = [junk if nil(j) else pt() for j in range(ks)]
    rows = [(f"random {i}", scs(), owns(), next(kinds)) for i in range(4)]
    rows.append(("zero scalars", [raw(0)] * K, owns(), "noncanonical"))  # the identity, expected as y + p
    for j in range(K):
        s = scs()
        s[j] = raw(0)
        rows.append((f"scalar {j} zero", s, owns(), next(kinds)))
    # the special scalars: each in every slot for the shapes of FULL_GRID, else each once, the slots taken in turn
    slots = [(v, j) for v in SPECIAL for j in range(K)] if (ko, ks, nil_mask) in FULL_GRID else \
        [(v, (i + nil_mask) % K) for i, v in enumerate(SPECIAL)]
    for v, j in slots:
        s = scs()
        s[j] = raw(v)
        rows.append((f"scalar {j} = {v:#x}", s, owns(), "equal"))
    rows.append(("every scalar 2^256 - 1", [raw(-1)] * K, owns(), "equal"))
    for j in range(ko):  # exceptional own points, slot by slot
        for label, p in (("identity", IDENT), ("identity as y + p", noncanonical(IDENT)), ("order 8", order8[j % len(order8)]),
                         ("order 4 as y = p", noncanonical(order4[0])), ("undecodable", OFF_CURVE)):
            o = owns()
            o[j] = p
            rows.append((f"own {j} {label}", scs(), o, next(kinds)))
    out = [("random bases", shared, rows)]
    for j in range(ks):  # exceptional shared points, slot by slot, a batch each
        if nil(j):
            continue
        for label, p in (("identity as y + p", noncanonical(IDENT)), ("order 8", order8[j % len(order8)]), ("undecodable", OFF_CURVE)):
            sh = list(shared)
            sh[j] = p
            out.append((f"shared {j} {label}", sh, [(f"shared {j} {label}", scs(), owns(), "equal"),
                                                    (f"shared {j} {label}, own 0 undecodable", scs(), [OFF_CURVE] * ko, "equal")]))
    # every term on the standard base: terms on the same point, and pairs of terms that cancel
    twin = [junk if nil(j) else BASE for j in range(ks)]
    rows = [("every term on one point", scs(), [BASE] * ko, "sign")]
    if K >= 2:
        for a, b in sorted({(0, K - 1), (0, 1), (K - 2, K - 1)}):
            s = [raw(0)] * K
            v = rng.getrandbits(250) + 1
            s[a], s[b] = sc(v), sc(-v)
            rows.append((f"terms {a} and {b} cancel", s, [BASE] * ko, "noncanonical"))
            s = scs()
            s[b] = sc(-sum(int.from_bytes(x, "little") for i, x in enumerate(s) if i != b))
            rows.append((f"all terms cancel through {b}", s, [BASE] * ko, "noncanonical"))
    out.append(("one point", twin, rows))
    return out


def shapes():
    """(ko, ks, nil_mask): every shape with 1 <= ko + ks, every nil mask where ks <= 2, three masks above"""
    out = []
    for ko in range(5):
        for ks in range(5):
            if ko + ks == 0:
                continue
            masks = range(1 << ks) if ks <= 2 else (0, 5 & ((1 << ks) - 1), (1 << ks) - 1)
            out += [(ko, ks, m) for m in masks]
    return out
