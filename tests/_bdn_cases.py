"""The labelled table behind tests/test_bdn_host.py and tests/test_gpu_bdn.py: rosters and masks for every (suite,
group) pair of tests/_bdn_oracle.py, with what the oracle expects of kyb_<suite>_bdn_terms_<g> and
kyb_<suite>_mask_aggregate_<g> over them.  Everything is computed once per process and cached.

Rosters, by name:
  m1 .. m17     m in SIZES distinct keys: every group edge of both table widths (4 | 5, 8 | 9, a partial last group)
  equal         two equal keys among five (an addition that must double)
  opposite      P next to -P (a table entry at infinity)
  identity      the identity among four keys
  undecodable   one key with x >= p among five: every coefficient and term is zero, the status names the key
  xplusp        bn256 only: a key given as x + p, which UnmarshalBinary reduces: same coefficients and terms as m3
  offsub        BLS12-381 G1 only: a curve point off the subgroup among three keys; rejected unless vouched for
Masks, by label, for a roster of m keys: empty, full (stray bits set), half (m // 2 bits: the largest count that is
not flipped), half+1 (the smallest that is), stray (one bit and every bit at or above m), and three patterns."""
import functools

import numpy as np

from tests import _bdn_oracle as O

SIZES = (1, 3, 4, 5, 8, 9, 17)
COMMON = tuple(f"m{m}" for m in SIZES) + ("equal", "opposite", "identity", "undecodable")


def names(G):
    extra = ("xplusp",) if G.name.startswith("bn256") else ("offsub",) if G.name == "bls12381_g1" else ()
    return COMMON + extra


@functools.lru_cache(maxsize=None)
def _key(gname, k):
    return O.BY_NAME[gname].key(k)


def _scalar(j):
    return 0x9E3779B97F4A7C15 * (j + 2) + 12345


def _bad_key(G):
    """x >= p under valid flag bits (BLS12-381), a point off the curve (the BN suites): KYB_ST_BAD_POINT"""
    if G.suite == "bls12381":
        return bytes([0x9F]) + b"\xff" * (G.POINT - 1)
    return b"".join((1).to_bytes(32, "big") for _ in range(G.POINT // 32))


@functools.lru_cache(maxsize=None)
def roster(gname, name):
    G = O.BY_NAME[gname]
    key = lambda j: _key(gname, _scalar(j))
    if name[0] == "m" and name[1:].isdigit():
        return tuple(key(j) for j in range(int(name[1:])))
    if name == "equal":
        return (key(0), key(1), key(0), key(2), key(3))
    if name == "opposite":
        p = G.decode(key(1))[1]
        return (key(0), key(1), G.marshal(G.neg(p)), key(2), key(3))
    if name == "identity":
        return (key(0), G.marshal(None), key(1), key(2))
    if name == "undecodable":
        return (key(0), key(1), key(2), _bad_key(G), key(4))
    if name == "xplusp":  # the first coordinate of key 1 plus p: below 2^256, and reduced on decode
        from oracle import bn256 as ON
        k = key(1)
        return (key(0), (int.from_bytes(k[:32], "big") + ON.P).to_bytes(32, "big") + k[32:], key(2))
    if name == "offsub":
        return (key(0), O.bls_g1_off_subgroup(), key(2))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def terms(gname, name, flags=0):
    """(coefs, terms, status) the oracle expects of bdn_terms"""
    return _terms(gname, name, flags)[:3]


@functools.lru_cache(maxsize=None)
def _terms(gname, name, flags):
    """... and the terms as the oracle's points, which `expected` sums as they are: they need no second UnmarshalBinary"""
    G = O.BY_NAME[gname]
    dec = O.decode_all(G, roster(gname, name), flags)
    if any(st for st, _ in dec):
        return tuple(O.new_mask(G, roster(gname, name), flags)) + (None,)
    return O.new_mask_points(G, dec)


@functools.lru_cache(maxsize=None)
def points(gname, name, flags=0):
    """what mask_aggregate sums in this table: the roster's terms, or the roster itself where it has none"""
    coefs, tm, status = terms(gname, name, flags)
    return tuple(tm) if not any(status) else roster(gname, name)


@functools.lru_cache(maxsize=None)
def masks(m):
    """[(label, mask of (m + 7) >> 3 bytes)]"""
    L = O.mask_len(m)

    def of(bits, stray=False):
        b = bytearray(L)
        for j in bits:
            b[j >> 3] |= 1 << (j & 7)
        if stray:
            for j in range(m, 8 * L):
                b[j >> 3] |= 1 << (j & 7)
        return bytes(b)

    rng = np.random.default_rng(m)
    rows = [("empty", of([])), ("full", b"\xff" * L), ("half", of(range(m // 2))), ("half+1", of(range(m - m // 2 - 1, m))),
            ("stray", of([0], stray=True))]
    for k in range(3):
        rows.append((f"pattern{k}", of([j for j in range(m) if rng.integers(0, 2)], stray=bool(k & 1))))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def expected(gname, name, flags=0):
    """[(out, count, status)] per mask of masks(m) over points(gname, name)"""
    G = O.BY_NAME[gname]
    pts = points(gname, name, flags)
    made = _terms(gname, name, flags)[3]
    dec = O.decode_all(G, pts, flags) if made is None else [(O.ST_OK, p) for p in made]
    return tuple(O.aggregate(G, pts, mk, flags, dec) for _, mk in masks(len(pts)))


def pack(rows, width):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()


def pack_masks(ms, m, stride):
    """the masks at `stride`, the last one ending the buffer"""
    L = O.mask_len(m)
    flat = np.full((len(ms) - 1) * stride + L, 0xA5, dtype=np.uint8)
    for i, mk in enumerate(ms):
        flat[i * stride:i * stride + L] = np.frombuffer(mk, dtype=np.uint8)
    return flat
