"""Labelled cases of sign/anon Encrypt / Decrypt for the host-harness and the GPU tests, each with the oracle's answer
(tests/_anon_enc_oracle.py), computed once per process and shared.

A batch is a dict: ring, sets (one list of ring keys, or one per element), x / msgs / sealed / seal_status for a seal;
cts / mine / privs / opened / open_status for an open; labels names each element.  `opened[i]` is the plaintext, or None
with a status; in that case the engine's slot must be all zero.
"""
from __future__ import annotations

import functools

from kyber_amd.util import blake2xb
from tests import _anon_enc_oracle as E

# the keystream's 64-byte node edges, the MAC's key edge at 64 and its 128-byte block edges behind it, the keyless root
LENGTHS = (0, 1, 12, 63, 64, 65, 127, 128, 129, 191, 192, 193, 320, 321)


def _stream(tag: str):
    return blake2xb.New(b"anon-enc-cases/" + tag.encode())


@functools.lru_cache(maxsize=None)
def members(ring: int, tag: str = "set"):
    """ring key pairs ((priv, pub), ...), every private key reduced"""
    return tuple(E.keypair("%s/%d/%d" % (tag, ring, k)) for k in range(ring))


def _msg(tag: str, n: int) -> bytes:
    return _stream("msg/" + tag).Read(n)


def _batch(ring, sets, xs, msgs, mine, privs, labels):
    """seal every message with the oracle, then open what it made"""
    shared = not isinstance(sets[0], (list, tuple))
    set_of = (lambda i: list(sets)) if shared else (lambda i: list(sets[i]))
    sealed, sst = zip(*(E.seal(m, set_of(i), xs[i]) for i, m in enumerate(msgs)))
    return _with_open(dict(ring=ring, sets=sets, x=list(xs), msgs=list(msgs), sealed=list(sealed), seal_status=list(sst), labels=list(labels)),
                      list(sealed), mine, privs)


def _with_open(b, cts, mine, privs):
    shared = not isinstance(b["sets"][0], (list, tuple))
    one = not isinstance(privs, (list, tuple))
    res = [E.open_(ct, list(b["sets"]) if shared else list(b["sets"][i]), mine[i], privs if one else privs[i]) for i, ct in enumerate(cts)]
    b.update(cts=list(cts), mine=list(mine), privs=privs, opened=[r[0] for r in res], open_status=[r[1] for r in res])
    return b


@functools.lru_cache(maxsize=None)
def lengths_batch():
    """every message length, one shared set of three, receivers at first, middle and last position in turn"""
    ring = 3
    mem = members(ring)
    r = _stream("lengths")
    xs = [E.new_key(r) for _ in LENGTHS]
    mine = [i % ring for i in range(len(LENGTHS))]
    return _batch(ring, [p for _, p in mem], xs, [_msg("len%d" % n, n) for n in LENGTHS], mine, [mem[m][0] for m in mine],
                  ["len %d" % n for n in LENGTHS])


@functools.lru_cache(maxsize=None)
def shape_batch(n: int, ring: int, per_element: bool, one_receiver: bool):
    """n messages of a few short lengths for a ring; per_element: every element its own set (the same members rotated,
    so that the tables differ per lane); one_receiver: member 0's key opens everything (priv stride 0), else the
    receivers take first, middle and last position in turn"""
    mem = members(ring, "shape")
    pubs = [p for _, p in mem]
    r = _stream("shape/%d/%d" % (n, ring))
    xs = [E.new_key(r) for _ in range(n)]
    if n >= 64 and not per_element:
        _precompute(xs, pubs, [p for p, _ in mem])
    msgs = [_msg("s%d" % i, (0, 5, 33, 70)[i % 4]) for i in range(n)]
    if one_receiver:
        mine = [0] * n
    else:
        mine = [(0, ring // 2, ring - 1)[i % 3] for i in range(n)]
    if per_element:
        sets = [pubs[i % ring:] + pubs[:i % ring] for i in range(n)]
        who = [(mine[i] + i) % ring for i in range(n)]  # the member standing at mine[i] of the rotated set
    else:
        sets, who = pubs, mine
    privs = mem[0][0] if one_receiver and not per_element else [mem[w][0] for w in who]
    return _batch(ring, sets, xs, msgs, mine, privs, ["%d/%d" % (i, n) for i in range(n)])


def _precompute(xs, pubs, privs):
    """a large valid batch's products from the C restatement into the oracle's cache: x B and x Y for the seal; for the
    open priv X, xb B and xb Y with xb = x mod l.  One in 37 is recomputed by oracle/ed25519.py."""
    import numpy as np

    from tests import _oracle_c as OC

    arr = lambda bs: np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(len(bs), 32).copy()
    X = [bytes(v) for v in OC.ed_mul_base(arr(xs))]
    xbs = [E.reduced(x) for x in xs]
    pairs = [(x, Y) for x in xs for Y in pubs] + [(xb, Y) for xb in xbs for Y in pubs] + [(p, Xi) for Xi in X for p in privs]
    out, st = OC.ed_mul(arr([a for a, _ in pairs]), arr([P for _, P in pairs]))
    assert not np.asarray(st).any()
    for (a, P), v in zip(pairs, out):
        E.PRODUCTS[(a, P)] = bytes(v)
    for x, xb, Xi, XBi in zip(xs, xbs, X, OC.ed_mul_base(arr(xbs))):
        E.PRODUCTS[(x, None)], E.PRODUCTS[(xb, None)] = Xi, bytes(XBi)
    for k, (a, P) in enumerate(list(E.PRODUCTS)):
        if k % 37 == 0:
            assert E.PRODUCTS[(a, P)] == (E.O.mul_base(a) if P is None else E.O.mul(a, P))


def _flip(ct: bytes, byte: int, bit: int = 0) -> bytes:
    b = bytearray(ct)
    b[byte] ^= 1 << bit
    return bytes(b)


def _flip_X(ct: bytes, decodes: bool) -> bytes:
    """ct with one bit of X flipped so that X still decodes / no longer decodes"""
    for bit in range(8 * 32 - 1):
        c = _flip(ct, bit // 8, bit % 8)
        if (E.O.decode(c[:32]) is not None) == decodes:
            return c
    raise AssertionError


@functools.lru_cache(maxsize=None)
def rejects_batch():
    """Decrypt's rejects, one per element between valid neighbours, every element with a set of its own (ring 3) so that
    the cases that need a special set stand in the same batch"""
    ring = 3
    mem = members(ring, "rej")
    K = [p for _, p in mem]
    hdr = 32 + 32 * ring
    r = _stream("rejects")
    msg = _msg("rej", 40)
    base, st = E.seal(msg, K, E.new_key(r))
    empty, st2 = E.seal(b"", K, E.new_key(r))
    assert st == 0 and st2 == 0
    T, U = E.torsion_point(), E.undecodable()
    KT, KU = [K[0], T, K[2]], [K[0], U, K[2]]
    tors, st3 = E.seal(msg, KT, E.new_key(r))
    assert st3 == 0
    ident, st4 = E.seal(msg, K, E.X_IS_L)
    assert st4 == 0
    mine, priv = 1, mem[1][0]
    cases = [
        ("X flipped, decodes", _flip_X(base, True), K, mine, priv),
        ("X flipped, no point", _flip_X(base, False), K, mine, priv),
        ("slot mine flipped", _flip(base, 32 + 32 * mine + 7, 3), K, mine, priv),
        ("another slot flipped", _flip(base, 32 + 32 * 2 + 9, 5), K, mine, priv),
        ("body flipped", _flip(base, hdr + 11, 1), K, mine, priv),
        ("mac flipped", _flip(base, len(base) - 1, 7), K, mine, priv),
        ("wrong mine", base, K, 2, priv),
        ("wrong private key", base, K, mine, mem[0][0]),
        ("cut 31", empty[:31], K, mine, priv),
        ("cut 32", empty[:32], K, mine, priv),
        ("cut hdr-1", empty[:hdr - 1], K, mine, priv),
        ("cut hdr", empty[:hdr], K, mine, priv),
        ("cut hdr+15", empty[:hdr + 15], K, mine, priv),
        ("cut hdr+16: a valid empty message", empty[:hdr + 16], K, mine, priv),
        ("message cut to hdr+16", base[:hdr + 16], K, mine, priv),
        ("short, X no point, 31", U[:31], K, mine, priv),
        ("short, X no point, 32", U + b"", K, mine, priv),
        ("short, X no point, hdr-1", U + base[32:hdr - 1], K, mine, priv),
        ("X = identity", ident, K, mine, priv),
        ("X = identity, sign bit set", E.IDENTITY_NONCANONICAL[0] + ident[32:], K, mine, priv),
        ("X = identity as y + p", E.IDENTITY_NONCANONICAL[1] + ident[32:], K, mine, priv),
        ("torsion member under a clamped x", tors, KT, 0, mem[0][0]),
        ("member is no point", base, KU, 0, mem[0][0]),
        ("member is no point, short X-only", base[:32], KU, 0, mem[0][0]),
    ]
    labels, cts, sets, mines, privs = [], [], [], [], []
    for c in cases:  # a valid neighbour in front of every case, and one behind the last
        for label, ct, keys, m, p in (("valid", base, K, mine, priv), c):
            labels.append(label); cts.append(ct); sets.append(list(keys)); mines.append(m); privs.append(p)
    labels.append("valid"); cts.append(base); sets.append(list(K)); mines.append(mine); privs.append(priv)
    b = _with_open(dict(ring=ring, sets=sets, labels=labels), cts, mines, privs)
    # what every label must give, stated here and not read off the oracle
    want = {"valid": 0, "X flipped, no point": 1, "slot mine flipped": 12, "another slot flipped": 12, "body flipped": 13, "mac flipped": 13,
            "wrong mine": 12, "wrong private key": 12, "cut 31": 11, "cut 32": 11, "cut hdr-1": 11, "cut hdr": 11, "cut hdr+15": 11,
            "cut hdr+16: a valid empty message": 0, "message cut to hdr+16": 13, "short, X no point, 31": 11, "short, X no point, 32": 1,
            "short, X no point, hdr-1": 1, "X = identity": 0, "X = identity, sign bit set": 0, "X = identity as y + p": 0,
            "torsion member under a clamped x": 12, "member is no point": 1, "member is no point, short X-only": 11,
            "X flipped, decodes": 12}
    for label, stt in zip(labels, b["open_status"]):
        assert want[label] == stt, (label, stt)
    return b


@functools.lru_cache(maxsize=None)
def seal_edge_batch():
    """seal's own edges, per-element sets of three: a member that is no point (an all-zero slot between valid ones), a
    torsion member, x given unreduced (x + l and a 256-bit x: the products use those bytes, the slots carry x mod l)"""
    ring = 3
    mem = members(ring, "rej")
    K = [p for _, p in mem]
    r = _stream("seal-edges")
    x0 = E.new_key(r)
    xs = [x0, E.new_key(r), E.new_key(r), (int.from_bytes(x0, "little") % E.L + E.L).to_bytes(32, "little"), bytes([0xF3]) * 32, E.X_IS_L]
    sets = [K, [K[0], E.undecodable(), K[2]], [E.torsion_point(), K[1], K[2]], K, K, K]
    msgs = [_msg("e%d" % i, 17 + i) for i in range(len(xs))]
    labels = ["valid", "member is no point", "torsion member", "x + l", "x of 256 bits", "x = l"]
    sealed, sst = zip(*(E.seal(m, s, x) for m, s, x in zip(msgs, sets, xs)))
    assert list(sst) == [0, 1, 0, 0, 0, 0]
    return dict(ring=ring, sets=[list(s) for s in sets], x=xs, msgs=msgs, sealed=list(sealed), seal_status=list(sst), labels=labels)


def shared_bad_set():
    """(ring, keys, x, msgs, cts): one set for the batch with a member that is no point -- every element is refused"""
    mem = members(3, "rej")
    K = [mem[0][1], E.undecodable(), mem[2][1]]
    good = [p for _, p in mem]
    r = _stream("shared-bad")
    xs = [E.new_key(r) for _ in range(3)]
    msgs = [b"", b"abc", _msg("sb", 70)]
    cts = [E.seal(m, good, x)[0] for m, x in zip(msgs, xs)]
    return 3, K, xs, msgs, cts, mem
