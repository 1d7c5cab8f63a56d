"""CPU ORACLE (test infrastructure) -- the reference's sign/anon (sig.go) restated on oracle/ed25519.py and the host
BLAKE2Xb (kyber_amd/util/blake2xb.py).  The checker of the ring-signature tests, never the thing shipped.

Every product is composed from the oracle's mul_base, mul and add, so scalars are the wire bytes with the reference's
behaviour at and above 2^255: s G is geScalarMultBase's value whatever `vartime` says, the other products follow it.
"""
from __future__ import annotations

from kyber_amd.util import blake2xb
from oracle import ed25519 as O

L = O.L
IDENTITY_ENC = O.encode(O.IDENTITY)


def canon(enc: bytes):
    """MarshalBinary(UnmarshalBinary(enc)), None when enc does not decode"""
    pt = O.decode(enc)
    return None if pt is None else O.encode(pt)


def canon_bytes(enc: bytes) -> bytes:
    """the bytes MarshalBinary would write, from the wire bytes alone (defined for encodings that do not decode too)"""
    v = int.from_bytes(enc, "little")
    sign, y = v >> 255, (v & ((1 << 255) - 1)) % O.P
    if y in (1, O.P - 1):
        sign = 0
    return (y | (sign << 255)).to_bytes(32, "little")


def point_pick(stream) -> bytes:
    """Point.Pick = Embed(nil, rand), point.go:132-182: 32 stream bytes, FromBytes, times 8, retried on failure or identity"""
    while True:
        pt = O.decode(stream.XORKeyStream(bytes(32)))
        if pt is None:
            continue
        q = O.mul_int(8, pt)
        if q != O.IDENTITY:
            return O.encode(q)


def scalar_pick(stream) -> bytes:
    return blake2xb.pick(stream.Read)


def link_base(scope: bytes) -> bytes:
    return point_pick(blake2xb.New(scope))


def padd(a: bytes, b: bytes) -> bytes:
    return O.encode(O.add(O.decode(a), O.decode(b)))


def h1(message: bytes, scope, tag, PG: bytes, PH) -> bytes:
    """signH1(signH1pre(...), PG, PH), sig.go:23-43.  tag: the bytes MarshalBinary writes for it"""
    x = blake2xb.New(message)
    if scope is not None:
        x.Write(scope)
        x.Write(tag)
    x.Write(PG)
    if PH is not None:
        x.Write(PH)
    return scalar_pick(x)


def step(message, scope, base, tagc, key: bytes, s: bytes, c: bytes, vartime=False):
    """one ring position (sig.go:232-236); None when the key does not decode"""
    cx = O.mul(c, key, vartime)
    if cx is None:
        return None
    PG = padd(O.mul_base(s), cx)
    PH = None
    if scope is not None:
        PH = padd(O.mul(s, base, vartime), O.mul(c, tagc, vartime))
    return h1(message, scope, tagc, PG, PH)


def chain(message, keys, scope, sig: bytes, start=0, steps=None, vartime=False):
    """(c_zero, c_out, ok, status) of kyb_ed25519_ring_chain for one signature: status 1 and zero challenges when the
    tag or a visited key does not decode"""
    ring = len(keys)
    steps = ring if steps is None else steps
    c0 = sig[:32]
    s = [sig[32 * (1 + i):32 * (2 + i)] for i in range(ring)]
    base = tagc = None
    bad = False
    if scope is not None:
        base = link_base(scope)
        tagc = canon(sig[32 * (1 + ring):32 * (2 + ring)])
        if tagc is None:
            return bytes(32), bytes(32), 0, 1
    c, pos = c0, start
    czero = c0 if start == 0 else bytes(32)
    for _ in range(steps):
        c = step(message, scope, base, tagc, keys[pos], s[pos], c, vartime)
        if c is None:
            bad = True
            break
        pos = (pos + 1) % ring
        if pos == 0:
            czero = c
    if bad:
        return bytes(32), bytes(32), 0, 1
    return czero, c, int(c == c0), 0


def verify(message, keys, scope, sig: bytes, vartime=False):
    """Verify, sig.go:192-248: the tag (b"" when unlinkable) or None for an invalid signature"""
    ring = len(keys)
    if len(sig) < 32 * (ring + (2 if scope is not None else 1)):
        return None
    _, _, ok, st = chain(message, keys, scope, sig, vartime=vartime)
    if not ok:
        return None
    return b"" if scope is None else canon(sig[32 * (1 + ring):32 * (2 + ring)])


def sign(message, keys, scope, mine: int, x: bytes, rand) -> bytes:
    """Sign, sig.go:107-180, drawing u and the s_i from rand in the reference's order"""
    ring = len(keys)
    xi = int.from_bytes(x, "little") % L
    base = tag = None
    if scope is not None:
        base = link_base(scope)
        tag = O.mul(x, base)
    u = scalar_pick(rand)
    UB = O.mul_base(u)
    UL = O.mul(u, base) if scope is not None else None
    s = [None] * ring
    c = [None] * ring
    c[(mine + 1) % ring] = h1(message, scope, tag, UB, UL)
    i = (mine + 1) % ring
    while i != mine:
        s[i] = scalar_pick(rand)
        c[(i + 1) % ring] = step(message, scope, base, tag, keys[i], s[i], c[i])
        i = (i + 1) % ring
    s[mine] = ((int.from_bytes(u, "little") - xi * int.from_bytes(c[mine], "little")) % L).to_bytes(32, "little")
    return c[0] + b"".join(s) + (tag if scope is not None else b"")


GOLDEN_MESSAGE, GOLDEN_BAD_MESSAGE, GOLDEN_SCOPE = b"Hello World!", b"Goodbye world!", b"My Linkage Scope"


def golden_keys(name: str):
    """(keys, scope, mines, xs, rand) of one example of sig_test.go: its key generation replayed under blake2xb.New(nil),
    rand left where the example's first Sign finds it"""
    r = blake2xb.New(b"")
    if name == "ExampleSign_one":
        x = scalar_pick(r)
        return [O.mul_base(x)], None, [0], [x], r
    keys = [point_pick(r) for _ in range(3)]
    if name == "ExampleSign_anonSet":
        x = scalar_pick(r)
        keys[1] = O.mul_base(x)
        return keys, None, [1], [x], r
    assert name == "ExampleSign_linkable"
    x1, x2 = scalar_pick(r), scalar_pick(r)
    keys[1], keys[2] = O.mul_base(x1), O.mul_base(x2)
    return keys, GOLDEN_SCOPE, [1, 1, 2, 2], [x1, x1, x2, x2], r


GOLDEN_EXAMPLES = ("ExampleSign_one", "ExampleSign_anonSet", "ExampleSign_linkable")
