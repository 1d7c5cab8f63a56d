"""The batched Point.Add cases the host-harness tests and the GPU tests share: for each of the seven groups a table of
(a, b, expected out, expected status, label) rows, built on the oracles alone (no GPU, no engine).

Operand points are mostly links of chains of oracle additions, P_{i+1} = P_i + D, so a few thousand pairs cost seconds
(an oracle scalar multiplication costs some 400 additions).  Every expectation is

    status = status(a) if status(a) != 0 else status(b)      out = encode(decode(a) + decode(b)), or zero bytes

with decode / + / encode the oracle's.  What Add decodes is what the kernels' g*_add_wire decode: BLS12-381 applies every
rule of UnmarshalBinary, subgroup included (status 2); BN G2 operands are checked against the twist only -- on bn254 too,
whose UnmarshalBinary also checks the subgroup -- so a twist point outside the subgroup is an accepted operand; bn256
reduces a coordinate >= p (point.go:218-221) where bn254 rejects it (gfp.go:101-118).

Sizes: FILLER generic rows per table next to the labelled ones (a table is 280-470 rows; the seven build in a few
seconds: tests/test_add_cases.py prints the time); chain(name, n) makes the n generic rows of the batch-size tests."""
import functools
import json
import os
import random
from collections import Counter, namedtuple

import numpy as np

from oracle import bls12381 as OB, bn254 as ON4, bn256 as ON, ed25519 as OE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILLER = 192
Table = namedtuple("Table", "a b out status labels")  # (n, w) uint8 x 3, (n,) uint8, n labels

WEIERSTRASS_VALID = ["generic", "double", "cancel", "neg-plus-pos", "inf-plus-p", "p-plus-inf", "inf-plus-inf", "p-plus-2p",
                     "2p-plus-p", "same-x-negated-y", "same-y-other-x"]
BLS_REJECTS = ["no-compression-bit", "inf-with-sort-flag", "inf-with-x", "x-ge-p", "x-no-point", "off-subgroup"]
BN_REJECTS = ["off-curve", "half-zero"]
BN_G2_OFF = ["off-subgroup:member-plus-nonmember", "off-subgroup:nonmember-plus-member", "off-subgroup:nonmember-plus-negative",
             "off-subgroup:nonmember-doubled", "off-subgroup:nonmember-plus-inf"]
ED_LABELS = ["generic", "torsion-table", "torsion-plus-prime", "prime-plus-torsion", "cancel", "double", "noncanonical-a",
             "noncanonical-b", "noncanonical-both", "x-zero-result", "reject-a", "reject-b", "reject-both"]


def _slots(kinds):
    return ["reject-%s:%s" % (s, k) for k in kinds for s in ("a", "b", "both")]


class Group:
    """One group: its wire width and the oracle's decode / add / neg / encode.  decode(buf) -> (status, point); points
    made by the oracle's own additions are remembered with status 0 (multiples of the generator: nothing to re-check)."""

    def __init__(self, name, width, enc, dec, add, neg, mul, gen, order, inf, field_p=None, strict=False, fp2=False):
        self.name, self.width, self._enc, self._dec = name, width, enc, dec
        self.add, self.neg, self.mul, self.gen, self.order, self.inf = add, neg, mul, gen, order, inf
        self.p, self.strict, self.fp2 = field_p, strict, fp2
        self.memo = {}

    def enc(self, pt):
        b = self._enc(pt)
        self.memo.setdefault(b, (0, pt))
        return b

    def decode(self, buf):
        buf = bytes(buf)
        if buf not in self.memo:
            self.memo[buf] = self._dec(buf)
        return self.memo[buf]

    def expect(self, a, b):
        (sa, pa), (sb, pb) = self.decode(a), self.decode(b)
        st = sa if sa else sb
        return (st, bytes(self.width)) if st else (0, self._enc(self.add(pa, pb)))


def _bls_dec(decompress, in_subgroup):
    def dec(buf):
        try:
            pt = decompress(buf, subgroup_check=False)
        except OB.DecodeError:
            return 1, None
        return (0, pt) if pt is None or in_subgroup(pt) else (2, None)
    return dec


def _bn_dec(unmarshal, err):
    def dec(buf):
        try:
            return 0, unmarshal(buf)
        except err:
            return 1, None
    return dec


def _bn254_g2_on_twist(buf):
    """pointG2.UnmarshalBinary of bn254 without its subgroup half: what Add's operands are held to"""
    v = [ON4._coord(buf[32 * i:32 * i + 32]) for i in range(4)]
    x, y = (v[1], v[0]), (v[3], v[2])
    if x == (0, 0) and y == (0, 0):
        return None
    if not ON4.g2_on_curve((x, y)):
        raise ON4.DecodeError("bn254.G2: malformed point")
    return (x, y)


def _ed_dec(buf):
    pt = OE.decode(buf)
    return (1, None) if pt is None else (0, pt)


@functools.lru_cache(None)
def group(name):
    if name == "ed25519":
        return Group(name, 32, OE.encode, _ed_dec, OE.add, OE.neg, OE.mul_int, OE.B, OE.L, OE.IDENTITY)
    if name == "bls12381-g1":
        return Group(name, 48, OB.g1_compress, _bls_dec(OB.g1_decompress, OB.g1_in_subgroup), OB.g1_add, OB.g1_neg, OB.g1_mul,
                     OB.G1_GEN, OB.R, None, OB.P)
    if name == "bls12381-g2":
        return Group(name, 96, OB.g2_compress, _bls_dec(OB.g2_decompress, OB.g2_in_subgroup), OB.g2_add, OB.g2_neg, OB.g2_mul,
                     OB.G2_GEN, OB.R, None, OB.P, fp2=True)
    suite, g = name.split("-")
    M = {"bn256": ON, "bn254": ON4}[suite]
    strict = suite == "bn254"
    if g == "g1":
        return Group(name, 64, M.g1_marshal, _bn_dec(M.g1_unmarshal, M.DecodeError), M.g1_add, M.g1_neg, M.g1_mul, M.G1_GEN,
                     M.ORDER, None, M.P, strict)
    un = _bn254_g2_on_twist if strict else M.g2_unmarshal
    return Group(name, 128, M.g2_marshal, _bn_dec(un, M.DecodeError), M.g2_add, M.g2_neg, M.g2_mul, M.G2_GEN, M.ORDER, None,
                 M.P, strict, fp2=True)


GROUPS = ("ed25519", "bls12381-g1", "bls12381-g2", "bn256-g1", "bn256-g2", "bn254-g1", "bn254-g2")


def required_labels(name):
    if name == "ed25519":
        return list(ED_LABELS)
    if name.startswith("bls"):
        return WEIERSTRASS_VALID + ["cancel-by-sort-flag"] + _slots(BLS_REJECTS)
    out = WEIERSTRASS_VALID + _slots(BN_REJECTS) + ["coord-ge-p-a", "coord-ge-p-b", "coord-ge-p-both"]
    return out + (BN_G2_OFF if name.endswith("g2") else [])


def _chain(G, rng, n):
    """n points P_0 + i D, both random multiples of the generator"""
    p, d = G.mul(rng.randrange(1, G.order), G.gen), G.mul(rng.randrange(1, G.order), G.gen)
    out = []
    for _ in range(n):
        out.append(p)
        p = G.add(p, d)
    return out


class _Rows:
    def __init__(self, G):
        self.G, self.a, self.b, self.out, self.st, self.labels = G, [], [], [], [], []

    def put(self, a, b, label):
        st, out = self.G.expect(a, b)
        assert len(a) == len(b) == len(out) == self.G.width
        self.a.append(bytes(a)); self.b.append(bytes(b)); self.out.append(out); self.st.append(st); self.labels.append(label)

    def table(self):
        w = self.G.width
        arr = lambda rows: np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), w).copy()
        return Table(arr(self.a), arr(self.b), arr(self.out), np.array(self.st, dtype=np.uint8), list(self.labels))


def _cube_root_of_unity(p):
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    return pow(g, (p - 1) // 3, p)


def _reject_rows(R, kinds, good, rng):
    """every bad operand in slot a alone, in slot b alone, and in both next to a bad operand of ANOTHER kind (and, where
    there is one, of another status), both ways round: which operand's status comes back is visible"""
    names = list(kinds)
    for i, k in enumerate(names):
        for bad in kinds[k]:
            R.put(bad, rng.choice(good), "reject-a:" + k)
            R.put(rng.choice(good), bad, "reject-b:" + k)
        others = [names[(i + 1) % len(names)], names[(i + len(names) // 2) % len(names)], names[-1], names[0]]
        for o in dict.fromkeys(x for x in others if x != k):
            R.put(kinds[k][0], kinds[o][-1], "reject-both:" + k)
            R.put(kinds[o][-1], kinds[k][0], "reject-both:" + o)


def _on_curve_x(G, M, rng, want_point=True):
    """a random x with (want_point) or without a point of the curve / twist above it, and that point's y"""
    bls = G.name.startswith("bls")
    while True:
        if G.fp2:
            x = (rng.randrange(G.p), rng.randrange(G.p))
            y = M.f2_sqrt(M.f2_add(M.f2_mul(M.f2_sqr(x), x), M._Fp2.b if bls else M.TWIST_B))
        else:
            x = rng.randrange(G.p)
            y = M.fp_sqrt(x * x * x + (4 if bls else 3))
        if (y is not None) == want_point:
            return x, y


def _weierstrass_valid(R, G, rng, pts, qts):
    e = G.enc
    inf = e(None)
    beta = _cube_root_of_unity(G.p)
    for i in range(FILLER):
        R.put(e(pts[i]), e(qts[i]), "generic")
    for i in range(0, 12, 2):
        p, q = pts[FILLER + i], qts[FILLER + i]
        p2 = G.add(p, p)
        R.put(e(p), e(p), "double")
        R.put(e(p), e(G.neg(p)), "cancel")
        R.put(e(G.neg(q)), e(q), "neg-plus-pos")
        R.put(inf, e(p), "inf-plus-p")
        R.put(e(q), inf, "p-plus-inf")
        R.put(e(p), e(p2), "p-plus-2p")
        R.put(e(p2), e(p), "2p-plus-p")
        # the same x met again with y negated in the coordinates (not through the oracle's neg)
        x, y = q
        ny = tuple(-c % G.p for c in y) if G.fp2 else -y % G.p
        R.put(e(q), e((x, ny)), "same-x-negated-y")
        # (beta x, y) is on the curve too (j = 0) and in the subgroup (an endomorphism image): equal y, other x -- the
        # difference of the y's vanishes where that of the x's does not
        bx = tuple(c * beta % G.p for c in x) if G.fp2 else x * beta % G.p
        R.put(e(q), e((bx, y)), "same-y-other-x")
        R.put(e((bx, y)), e(q), "same-y-other-x")
    R.put(inf, inf, "inf-plus-inf")


def _bls_table(G, seed):
    rng = random.Random("add/%s/%d" % (G.name, seed))
    R = _Rows(G)
    pts, qts = _chain(G, rng, FILLER + 12), _chain(G, rng, FILLER + 12)
    _weierstrass_valid(R, G, rng, pts, qts)
    w, half = G.width, 48
    inf = G.enc(None)
    good = [G.enc(p) for p in pts[:16]] + [inf]
    for p in pts[FILLER:FILLER + 6]:  # -P written by flipping the sort flag of the same bytes
        b = G.enc(p)
        R.put(b, bytes([b[0] ^ 0x20]) + b[1:], "cancel-by-sort-flag")
        assert R.out[-1] == inf == bytes([0xC0]) + bytes(w - 1) and R.st[-1] == 0
    g0 = G.enc(pts[3])
    xn, _ = _on_curve_x(G, OB, rng, want_point=False)
    xs = [xn[1], xn[0]] if G.fp2 else [xn]
    no_point = bytearray(b"".join(v.to_bytes(48, "big") for v in xs))
    no_point[0] |= 0x80
    while True:  # a point of the curve outside the subgroup (the cofactor is large: the first one found)
        x, y = _on_curve_x(G, OB, rng)
        if G.decode(G._enc((x, y)))[0] == 2:
            break
    off = [G._enc((x, y)), G._enc(G.neg((x, y)))]
    pb = OB.P.to_bytes(48, "big")
    ge_p = [bytes([pb[0] | 0x80]) + pb[1:] + bytes(w - half), bytes([0x9F]) + b"\xff" * 47 + bytes(w - half)]
    if G.fp2:  # the second half (x.c0) >= p under a first half that is fine
        ge_p.append(g0[:half] + pb)
    kinds = {
        "no-compression-bit": [bytes([g0[0] & 0x7F]) + g0[1:], bytes(w)],
        "inf-with-sort-flag": [bytes([0xE0]) + bytes(w - 1)],
        "inf-with-x": [bytes([0xC0]) + bytes(w - 2) + b"\x01", bytes([0xC0]) + g0[1:]],
        "x-ge-p": ge_p,
        "x-no-point": [bytes(no_point), bytes([no_point[0] | 0x20]) + bytes(no_point[1:])],
        "off-subgroup": off,
    }
    for k, v in kinds.items():
        for bad in v:
            assert G.decode(bad)[0] == (2 if k == "off-subgroup" else 1), (G.name, k)
    _reject_rows(R, kinds, good, rng)
    t = R.table()
    ok = t.status == 0
    for arr in (t.a[ok], t.b[ok], t.out[ok]):  # both values of the sort flag, in operands and in results
        finite = arr[(arr[:, 0] & 0x40) == 0]
        assert {0, 0x20} == set(np.unique(finite[:, 0] & 0x20)), G.name
    both = [(s, l) for s, l in zip(t.status, t.labels) if l.startswith("reject-both")]
    assert {1, 2} == {int(s) for s, _ in both}, "precedence needs both statuses among the doubly bad rows"
    return t


def _bn_table(G, seed):
    M = ON4 if G.strict else ON
    rng = random.Random("add/%s/%d" % (G.name, seed))
    R = _Rows(G)
    pts, qts = _chain(G, rng, FILLER + 12), _chain(G, rng, FILLER + 12)
    _weierstrass_valid(R, G, rng, pts, qts)
    w, e = G.width, G.enc
    nc = w // 32
    good = [e(p) for p in pts[:16]] + [bytes(w)]
    be = lambda v: v.to_bytes(32, "big")
    g0 = e(pts[5])
    # a coordinate written as c + p (where that fits 256 bits): bn256 reduces it, bn254 rejects it -- the oracle says which
    plus_p = []
    for p in [G.gen] + pts:
        b = e(p)
        cand = [k for k in range(nc) if int.from_bytes(b[32 * k:32 * k + 32], "big") + G.p < 1 << 256]
        for k in cand:
            if sum(1 for _, kk in plus_p if kk == k) < 2:
                c = int.from_bytes(b[32 * k:32 * k + 32], "big")
                plus_p.append((b[:32 * k] + be(c + G.p) + b[32 * k + 32:], k))
        if len(plus_p) == 2 * nc:
            break
    assert {k for _, k in plus_p} == set(range(nc)), "every coordinate slot written as c + p"
    for i, (bad, _) in enumerate(plus_p):
        R.put(bad, good[i], "coord-ge-p-a")
        R.put(good[i], bad, "coord-ge-p-b")
        R.put(bad, plus_p[(i + 1) % len(plus_p)][0], "coord-ge-p-both")
        assert G.decode(bad)[0] == (1 if G.strict else 0), G.name
    five = be(5)
    kinds = {
        "off-curve": [bytes(32) * (nc - 1) + five, five * nc, g0[:w - 32] + be((int.from_bytes(g0[w - 32:], "big") + 1) % G.p)],
        "half-zero": [bytes(w // 2) + g0[w // 2:], g0[:w // 2] + bytes(w // 2)],
    }
    if G.strict:  # (on bn254 c + p is one more kind of rejected operand)
        kinds["coord-ge-p"] = [plus_p[0][0]]
    for k, v in kinds.items():
        for bad in v:
            assert G.decode(bad)[0] == 1, (G.name, k)
    _reject_rows(R, kinds, good, rng)
    if G.fp2:  # twist points outside the order-n subgroup: accepted, summed on the twist
        offs = []
        while len(offs) < 3:
            x, y = _on_curve_x(G, M, rng)
            if M.g2_mul(M.ORDER, (x, y)) is not None:
                offs.append((x, y))
        for i, q in enumerate(offs):
            assert G.decode(G._enc(q))[0] == 0
            R.put(e(pts[i]), e(q), "off-subgroup:member-plus-nonmember")
            R.put(e(q), e(qts[i]), "off-subgroup:nonmember-plus-member")
            R.put(e(q), e(G.neg(q)), "off-subgroup:nonmember-plus-negative")
            R.put(e(q), e(q), "off-subgroup:nonmember-doubled")
            R.put(e(q), bytes(w), "off-subgroup:nonmember-plus-inf")
            R.put(e(q), e(offs[(i + 1) % 3]), "off-subgroup:nonmember-plus-member")
    return R.table()


def torsion_points():
    """the eight points of small order: the encodings of tests/golden/ed25519_misc.json, their negatives, the identity"""
    small = [bytes.fromhex(h) for h in json.load(open(os.path.join(GOLDEN, "ed25519_misc.json")))["small_order"]]
    pts = [OE.decode(s) for s in small]
    pts = list(dict.fromkeys([OE.IDENTITY] + pts + [OE.neg(p) for p in pts]))
    assert len(pts) == 8 and all(OE.mul_int(8, p) == OE.IDENTITY for p in pts)
    return pts


def small_y_points():
    """curve points with 2 <= y < 19: y + p still fits 255 bits"""
    le = lambda v: v.to_bytes(32, "little")
    return [le(y) for y in range(2, 19) if OE.decode(le(y)) is not None]


def ed_noncanonical():
    """encodings the decoder accepts that MarshalBinary never writes: y + p for small y with either sign, p + 1 (the
    identity) without and with bit 255, p (y = 0) and p - 1 | sign, "-0" = the identity with bit 255, all bits set
    (y = 2^255 - 1 = 18 mod p: a point)"""
    le = lambda v: v.to_bytes(32, "little")
    out = []
    for s in small_y_points():
        y = int.from_bytes(s, "little")
        out += [le(y + OE.P), le(y + OE.P | 1 << 255)]
    out += [le(OE.P + 1), le(OE.P + 1 | 1 << 255), le(1 | 1 << 255), le(OE.P), le(OE.P | 1 << 255), le(OE.P - 1 | 1 << 255),
            b"\xff" * 32]
    out = [s for s in out if OE.decode(s) is not None]
    assert all(OE.encode(OE.decode(s)) != s for s in out) and len(out) >= 8
    return out


def ed_non_points():
    """well-formed 32-byte strings with no x: y = 2 (the rejected operand of the older tests), the next such y's, bit 255 set"""
    le = lambda v: v.to_bytes(32, "little")
    ys = [y for y in range(2, 40) if OE.decode(le(y)) is None][:3]
    out = [le(y) for y in ys] + [le(ys[0] | 1 << 255), le(ys[1] + OE.P)]
    assert ys[0] == 2 and all(OE.decode(s) is None for s in out)
    return out


def _ed_table(G, seed):
    rng = random.Random("add/%s/%d" % (G.name, seed))
    R = _Rows(G)
    e = G.enc
    pts, qts = _chain(G, rng, FILLER + 12), _chain(G, rng, FILLER + 12)
    for i in range(FILLER):
        R.put(e(pts[i]), e(qts[i]), "generic")
    tors = torsion_points()
    ident = bytes([1]) + bytes(31)
    for s in tors:
        for t in tors:
            R.put(e(s), e(t), "torsion-table")
    for i, t in enumerate(tors):
        R.put(e(t), e(pts[i]), "torsion-plus-prime")
        R.put(e(qts[i]), e(t), "prime-plus-torsion")
    order2 = next(t for t in tors if t != OE.IDENTITY and OE.add(t, t) == OE.IDENTITY)
    for i in range(6):
        p = pts[FILLER + i]
        R.put(e(p), e(G.neg(p)), "cancel")
        assert R.out[-1] == ident
        R.put(e(p), e(p), "double")
        R.put(e(p), e(G.neg(p)), "x-zero-result")
        R.put(e(p), e(G.add(order2, G.neg(p))), "x-zero-result")  # P + (T2 - P) = (0, -1)
    for t in tors:
        R.put(e(t), e(G.neg(t)), "x-zero-result")
        if OE.add(OE.add(t, t), OE.add(t, t)) == OE.IDENTITY:
            R.put(e(t), e(t), "x-zero-result")  # order 1, 2, 4: the double is (0, +-1)
    nc = ed_noncanonical()
    for i, s in enumerate(nc):
        R.put(s, e(pts[i]), "noncanonical-a")
        R.put(e(qts[i]), s, "noncanonical-b")
        R.put(s, nc[(i + 1) % len(nc)], "noncanonical-both")
        R.put(s, s, "noncanonical-both")
        R.put(s, e(tors[i % 8]), "noncanonical-a")
    bad = ed_non_points()
    for i, s in enumerate(bad):
        R.put(s, e(pts[i]), "reject-a")
        R.put(e(pts[i]), s, "reject-b")
        R.put(s, bad[(i + 1) % len(bad)], "reject-both")
        R.put(s, nc[i], "reject-a")
        R.put(e(tors[i]), s, "reject-b")
    t = R.table()
    for i, l in enumerate(t.labels):
        if l == "x-zero-result":
            assert OE.decode(bytes(t.out[i]))[0] == 0, i
        if l.startswith("reject"):
            assert t.status[i] == 1 and not t.out[i].any()
    return t


@functools.lru_cache(None)
def table(name, seed=1):
    """Table(a, b, out, status, labels) of one group; every required label present"""
    G = group(name)
    t = _ed_table(G, seed) if name == "ed25519" else (_bls_table(G, seed) if name.startswith("bls") else _bn_table(G, seed))
    census = Counter(t.labels)
    missing = [l for l in required_labels(name) if not census[l]]
    assert not missing, (name, missing)
    n = len(t.labels)
    assert t.a.shape == t.b.shape == t.out.shape == (n, G.width) and t.status.shape == (n,)
    bad = t.status != 0
    assert not t.out[bad].any()
    return t


@functools.lru_cache(None)
def chain(name, n, seed=7):
    """(a, b, out): n generic rows a_i = P_0 + i D, b_i = Q_0 + i E and their oracle sums, the last rows P+P, P+(-P) and
    inf+P / identity+P so that the ragged tail of a batch holds exceptional operands too"""
    G = group(name)
    rng = random.Random("chain/%s/%d/%d" % (name, n, seed))
    pts, qts = _chain(G, rng, n), _chain(G, rng, n)
    for k, j in enumerate(range(max(0, n - 3), n)):
        qts[j] = [pts[j], G.neg(pts[j]), G.inf][k % 3]
    R = _Rows(G)
    for p, q in zip(pts, qts):
        R.put(G.enc(p), G.enc(q), "chain")
    t = R.table()
    assert not t.status.any()
    return t.a, t.b, t.out


def tiled(t, copies, seed=5):
    """the table `copies` times over, shuffled: rejected and infinite rows beside valid ones in every wave"""
    idx = np.tile(np.arange(len(t.labels)), copies)
    np.random.default_rng(seed).shuffle(idx)
    return Table(t.a[idx], t.b[idx], t.out[idx], t.status[idx], [t.labels[i] for i in idx])


def one_per_label(t):
    """row indices: the first row of every label (the subset the sanitizer pass runs)"""
    seen = {}
    for i, l in enumerate(t.labels):
        seen.setdefault(l, i)
    return sorted(seen.values())
