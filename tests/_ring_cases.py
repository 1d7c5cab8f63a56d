"""The table of ring-signature rows shared by tests/test_ring_host.py (the lane program on the CPU) and
tests/test_gpu_anon.py (the kernels): for every ring size in RINGS, unlinkable and linkable, one valid signature and its
labelled alterations.  Rows are made with the sign/anon oracle from a fixed stream; the oracle also gives every
expectation, so a row's label says what was done to it, never what must come out."""
from __future__ import annotations

import functools
from collections import namedtuple

from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests import _anon_oracle as A

RINGS = (1, 2, 3, 5)
SCOPE = b"ring cases scope"
LABELS = ("valid", "c0 altered", "s altered", "message altered", "scope altered", "tag altered", "key altered", "s + l",
          "s + 8 l", "s + 15 l", "c0 + l", "c0 + 8 l", "c0 + 15 l", "c0 = 0", "key undecodable", "tag undecodable", "key small order",
          "identity intermediate")
LINKABLE_ONLY = ("scope altered", "tag altered", "tag undecodable")

Row = namedtuple("Row", "label ring linkable message keys sig")  # verified under SCOPE when linkable


def _undecodable() -> bytes:
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


UNDECODABLE = _undecodable()
IDENTITY = O.encode(O.IDENTITY)
ORDER8 = bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a")  # const.go weakKeys


class _ZeroAt:
    """a stream whose k-th Read returns zeros (Scalar.Pick then picks 0), every other one the wrapped stream's bytes"""

    def __init__(self, inner, k):
        self.inner, self.k, self.i = inner, k, 0

    def Read(self, n):
        self.i += 1
        return bytes(n) if self.i == self.k else self.inner.Read(n)


def _put(sig: bytes, slot: int, v: bytes) -> bytes:
    return sig[:32 * slot] + v + sig[32 * slot + 32:]


def _add_l(v: bytes, k: int) -> bytes:
    return (int.from_bytes(v, "little") + k * O.L).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def base_keys(ring: int, linkable: bool):
    """(keys, mine, x): the anonymity set every row of (ring, linkable) starts from"""
    r = blake2xb.New(b"ring cases %d %d" % (ring, linkable))
    keys = [A.point_pick(r) for _ in range(ring)]
    mine = ring // 2
    x = A.scalar_pick(r)
    keys[mine] = O.mul_base(x)
    return tuple(keys), mine, x


@functools.lru_cache(maxsize=None)
def rows():
    out = []
    for ring in RINGS:
        for linkable in (False, True):
            keys, mine, x = base_keys(ring, linkable)
            keys = list(keys)
            scope = SCOPE if linkable else None
            r = blake2xb.New(b"ring rows %d %d" % (ring, linkable))
            msg = b"message of ring %d" % ring + b"." * (60 * (ring % 3))  # 17, 77 and 137 bytes: key only, key + data
            sig = A.sign(msg, keys, scope, mine, x, r)
            j = (mine + 1) % ring  # a position other than the signer's where the ring has one
            add = lambda label, m=msg, k=keys, s=sig: out.append(Row(label, ring, linkable, m, tuple(k), s))
            add("valid")
            add("c0 altered", s=_put(sig, 0, bytes([sig[0] ^ 1]) + sig[1:32]))
            add("s altered", s=_put(sig, 1 + j, bytes([sig[32 * (1 + j)] ^ 1]) + sig[32 * (1 + j) + 1:32 * (2 + j)]))
            add("message altered", m=msg + b"!")
            add("key altered", k=keys[:j] + [A.point_pick(r)] + keys[j + 1:])
            sj = sig[32 * (1 + j):32 * (2 + j)]
            add("s + l", s=_put(sig, 1 + j, _add_l(sj, 1)))
            add("s + 8 l", s=_put(sig, 1 + j, _add_l(sj, 8)))
            add("s + 15 l", s=_put(sig, 1 + j, _add_l(sj, 15)))
            add("c0 + l", s=_put(sig, 0, _add_l(sig[:32], 1)))
            add("c0 + 8 l", s=_put(sig, 0, _add_l(sig[:32], 8)))  # at and above 2^255: the top digit the recodings split on
            add("c0 + 15 l", s=_put(sig, 0, _add_l(sig[:32], 15)))
            add("c0 = 0", s=_put(sig, 0, bytes(32)))
            add("key undecodable", k=keys[:j] + [UNDECODABLE] + keys[j + 1:])
            add("key small order", k=keys[:j] + [ORDER8] + keys[j + 1:])
            if linkable:
                add("scope altered", s=A.sign(msg, keys, SCOPE + b"'", mine, x, r))
                add("tag altered", s=_put(sig, 1 + ring, O.mul_base(A.scalar_pick(r))))
                add("tag undecodable", s=_put(sig, 1 + ring, UNDECODABLE))
            if ring > 1:  # a valid signature whose position j has s_j = 0 and the identity as its key: PG is the identity
                ik = keys[:j] + [IDENTITY] + keys[j + 1:]
                add("identity intermediate", k=ik, s=A.sign(msg, ik, scope, mine, x, _ZeroAt(r, 2)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(vartime: bool):
    """the oracle's (c_zero, c_out, ok, status) of every row, Verify's chain"""
    return tuple(A.chain(r.message, list(r.keys), SCOPE if r.linkable else None, r.sig, vartime=vartime) for r in rows())


def groups():
    """{(ring, linkable): [row indices]}"""
    g = {}
    for i, r in enumerate(rows()):
        g.setdefault((r.ring, r.linkable), []).append(i)
    return g


def shared_groups():
    """{(ring, linkable, keys): [row indices]}: the rows that can share one ring in a call (key_stride = 0)"""
    g = {}
    for i, r in enumerate(rows()):
        g.setdefault((r.ring, r.linkable, r.keys), []).append(i)
    return g
