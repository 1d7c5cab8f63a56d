"""sign/bdn restated sequentially in Python integers (test infrastructure): bdn.go and mask.go line by line over
oracle/bn256.py, oracle/bls12381.py and oracle/bn254.py -- hashPointToR, NewMask's terms, AggregatePublicKeys and
AggregateSignatures -- plus the value of the two C entry points kyb_<suite>_bdn_terms_<g> and
kyb_<suite>_mask_aggregate_<g> as include/kyber_hip.h states it (statuses, the zero outputs of a rejected roster, stray
mask bits).  Pinned by the bytes the reference prints for bn256 (tests/golden/bn256.json: bdn_coefs, bdn_agg_key,
bdn_fixture_agg_sig_mask101, bdn_fixture_agg_key_mask101) in tests/test_bdn_host.py."""
import functools

from kyber_amd.util.blake2xs import blake2xs
from oracle import bls12381 as OB, bn254 as ON4, bn256 as ON

ST_OK, ST_BAD_POINT, ST_NOT_IN_SUBGROUP = 0, 1, 2  # include/kyber_hip.h
F_TRUSTED = 0x100


class Group:
    """One (suite, group) pair: `which` is tests/bdn_harness.cpp's index, `sym` the C ABI's suite and group names."""

    def __init__(self, which, suite, g, point, order, gen, add, mul, neg, marshal, decode):
        self.which, self.suite, self.g, self.POINT, self.ORDER, self.GEN = which, suite, g, point, order, gen
        self.add, self.mul, self.neg, self.marshal, self._decode = add, mul, neg, marshal, decode
        self.name = f"{suite}_{g}"

    def decode(self, buf, trusted=False):
        """(status, point): UnmarshalBinary's verdict in the C ABI's codes"""
        return self._decode(bytes(buf), trusted)

    def key(self, k):
        return self.marshal(self.mul(k % self.ORDER, self.GEN))


def _bls_decode(decompress, in_subgroup):
    def dec(buf, trusted):
        try:
            p = decompress(buf, False)
        except OB.DecodeError:
            return ST_BAD_POINT, None
        if not trusted and p is not None and not in_subgroup(p):
            return ST_NOT_IN_SUBGROUP, None
        return ST_OK, p
    return dec


def _bn_decode(unmarshal, err):
    def dec(buf, trusted):
        try:
            return ST_OK, unmarshal(buf)
        except err:
            return ST_BAD_POINT, None
    return dec


def _bn254_g2_decode(buf, trusted):
    """oracle/bn254.py g2_unmarshal with its documented fast subgroup criterion (the 254-bit ladder per key is what makes
    the table slow; tests/test_oracle_bn254.py holds the two criteria equal)"""
    try:
        v = [ON4._coord(buf[32 * i:32 * i + 32]) for i in range(4)]
    except ON4.DecodeError:
        return ST_BAD_POINT, None
    x, y = (v[1], v[0]), (v[3], v[2])
    if x == ON4.F2_ZERO and y == ON4.F2_ZERO:
        return ST_OK, None
    if not ON4.g2_on_curve((x, y)) or not ON4.g2_in_subgroup_fast((x, y)):
        return ST_BAD_POINT, None
    return ST_OK, (x, y)


GROUPS = [
    Group(0, "bls12381", "g1", 48, OB.R, OB.G1_GEN, OB.g1_add, OB.g1_mul, OB.g1_neg, OB.g1_compress, _bls_decode(OB.g1_decompress, OB.g1_in_subgroup)),
    Group(1, "bls12381", "g2", 96, OB.R, OB.G2_GEN, OB.g2_add, OB.g2_mul, OB.g2_neg, OB.g2_compress, _bls_decode(OB.g2_decompress, OB.g2_in_subgroup)),
    Group(2, "bn256", "g1", 64, ON.ORDER, ON.G1_GEN, ON.g1_add, ON.g1_mul, ON.g1_neg, ON.g1_marshal, _bn_decode(ON.g1_unmarshal, ON.DecodeError)),
    Group(3, "bn256", "g2", 128, ON.ORDER, ON.G2_GEN, ON.g2_add, ON.g2_mul, ON.g2_neg, ON.g2_marshal, _bn_decode(ON.g2_unmarshal, ON.DecodeError)),
    Group(4, "bn254", "g1", 64, ON4.ORDER, ON4.G1_GEN, ON4.g1_add, ON4.g1_mul, ON4.g1_neg, ON4.g1_marshal, _bn_decode(ON4.g1_unmarshal, ON4.DecodeError)),
    Group(5, "bn254", "g2", 128, ON4.ORDER, ON4.G2_GEN, ON4.g2_add, ON4.g2_mul, ON4.g2_neg, ON4.g2_marshal, _bn254_g2_decode),
]
BY_NAME = {G.name: G for G in GROUPS}


def mask_len(m):
    return (m + 7) >> 3


def hash_point_to_r(canon):
    """bdn.go:29-63 over MarshalBinary's bytes: (coefficients as integers, their 16 stream bytes each)"""
    out = blake2xs(b"".join(canon), 16 * len(canon))
    raw = [out[16 * i:16 * i + 16] for i in range(len(canon))]
    return [int.from_bytes(r, "little") for r in raw], raw


def new_mask(G, roster, flags=0):
    """kyb_<suite>_bdn_terms_<g>: (coefs, terms, status) -- mask.go:51-61, Mul(c, P) then Add(., P)"""
    dec = [G.decode(k, bool(flags & F_TRUSTED)) for k in roster]
    status = [st for st, _ in dec]
    if any(status):
        return [bytes(16)] * len(roster), [bytes(G.POINT)] * len(roster), status
    return new_mask_points(G, dec)[:3]


def new_mask_points(G, dec):
    """(coefs, terms, status, the terms as points) of a roster that decoded, from what decode_all gave for it"""
    coefs, raw = hash_point_to_r([G.marshal(p) for _, p in dec])
    pts = [G.add(G.mul(c, p), p) for c, (_, p) in zip(coefs, dec)]
    return raw, [G.marshal(p) for p in pts], [ST_OK] * len(dec), pts


def enabled(mask, m):
    return [j for j in range(m) if mask[j >> 3] >> (j & 7) & 1]


def decode_all(G, points, flags=0):
    """[(status, point)] of a list of encodings: UnmarshalBinary once per point"""
    return [G.decode(p, bool(flags & F_TRUSTED)) for p in points]


def aggregate(G, points, mask, flags=0, dec=None):
    """one element of kyb_<suite>_mask_aggregate_<g>: (out, count, status) -- bdn.go:166-181 over `points` (dec: what
    decode_all gave for them, where a caller has many masks over the same points)"""
    m = len(points)
    on = enabled(mask, m)
    dec = decode_all(G, points, flags) if dec is None else dec
    bad = [st for st, _ in dec if st]
    if bad:
        return bytes(G.POINT), len(on), bad[0]
    acc = None
    for j in on:
        acc = G.add(acc, dec[j][1])
    return G.marshal(acc), len(on), ST_OK


def aggregate_signatures(S, sigs, coefs, mask, m):
    """bdn.go:126-161 on the signature group S: the loop's errors in the loop's order"""
    acc, sigs = None, list(sigs)
    for j in range(m):
        if not mask[j >> 3] >> (j & 7) & 1:
            continue
        if not sigs:
            raise ValueError("length of signatures and public keys must match")
        st, p = S.decode(sigs.pop(0))
        if st:
            raise ValueError("invalid signature")
        acc = S.add(acc, S.add(S.mul(coefs[j], p), p))
    if sigs:
        raise ValueError("length of signatures and public keys must match")
    return S.marshal(acc)


def plan(n, m, fill=65536):
    """kyb_bdn_plan restated: the width by the count of additions, the slices by the lanes that fill the device"""
    def additions(g):
        full, rem = divmod(m, g)
        nb = full + (1 if rem else 0)
        return full * ((1 << g) - g - 1) + ((1 << rem) - rem - 1 if rem else 0) + nb + n * nb
    g = 8 if additions(8) < additions(4) else 4
    return g, min((m + g - 1) // g, (fill + n - 1) // n)


@functools.lru_cache(maxsize=None)
def bls_g1_off_subgroup():
    """a compressed BLS12-381 G1 encoding of a curve point outside the r-torsion (the cofactor is 76 bits: the first
    x with a square x^3 + 4 is one)"""
    x = 1
    while True:
        y = OB.fp_sqrt((x * x * x + 4) % OB.P)
        if y is not None and not OB.g1_in_subgroup((x, y)):
            return OB.g1_compress((x, y))
        x += 1
