"""The labelled table of kyb_ed25519_theta_check cases, shared by tests/test_shuffle_host.py (the lane program on the
CPU) and tests/test_gpu_shuffle.py (the kernels): batches of rows, one (U, W) per batch as in the call.  A row is
(label, a, A, b, B, T, must): must = 1 / 0 for a row that passes / fails for a known reason under both flag values,
None where the verdict is the oracle's alone (a scalar at or above 2^255 multiplies differently under KYB_F_VARTIME).
expect() is the oracle's statement of the call: thver over Xhat = A + U, Yhat = B + W (simple.go:178-183, 225-242) with
Neg(b) the scalar -b mod l."""
import random

from oracle import ed25519 as O
from tests import _ed_verify_oracle as V

L = O.L
ST_BAD_POINT = 1
IDENT = O.encode(O.IDENTITY)


def sc(v: int) -> bytes:
    return (v % L).to_bytes(32, "little")


def raw(v: int) -> bytes:
    return (v % 2**256).to_bytes(32, "little")


def _pt(k: int) -> bytes:
    return O.encode(O.mul_int(k, O.B))


def _add(a: bytes, b) -> bytes:
    return a if b is None else O.encode(O.add(O.decode(a), O.decode(b)))


def _neg(a: bytes) -> bytes:
    return O.encode(O.neg(O.decode(a)))


def lhs(a, A, U, b, B, W, vartime: bool, point_negation: bool = False):
    """encode(a (A + U) + Neg(b) (B + W)), None where a point does not decode.  point_negation: -(b (B + W)) instead,
    which is NOT what the reference computes (scalar.go:119-128) and differs where B + W has a torsion component"""
    if any(O.decode(bytes(p)) is None for p in (A, B) + tuple(x for x in (U, W) if x is not None)):
        return None
    xh, yh = _add(bytes(A), U), _add(bytes(B), W)
    p = O.decode(O.mul(bytes(a), xh, vartime))
    if point_negation:
        q = O.neg(O.decode(O.mul(bytes(b), yh, vartime)))
    else:
        q = O.decode(O.mul(sc(-int.from_bytes(bytes(b), "little")), yh, vartime))
    return O.encode(O.add(p, q))


def expect(a, A, U, b, B, W, T, vartime: bool, point_negation: bool = False):
    """(ok, status) of one element"""
    v = lhs(a, A, U, b, B, W, vartime, point_negation)
    if v is None:
        return 0, ST_BAD_POINT
    t = O.decode(bytes(T))
    return int(t is not None and O.encode(t) == v), 0


def _off_curve(rng) -> bytes:
    while True:
        e = rng.getrandbits(255).to_bytes(32, "little")
        if O.decode(e) is None:
            return e


def batches():
    """[(name, U, W, rows)]"""
    rng = random.Random(20)
    small = [bytes.fromhex(h) for h in V._misc()["small_order"]]
    order8 = [s for s in small if O.mul_int(4, O.decode(s)) != O.IDENTITY]
    order4 = [s for s in small if O.mul_int(2, O.decode(s)) != O.IDENTITY and O.mul_int(4, O.decode(s)) == O.IDENTITY]
    assert order8 and order4
    U, W = _pt(rng.getrandbits(250)), _pt(rng.getrandbits(250))
    bad = _off_curve(rng)

    def rnd():
        return sc(rng.getrandbits(256)), _pt(rng.getrandbits(250) + 1), sc(rng.getrandbits(256)), _pt(rng.getrandbits(250) + 1)

    def flip(x: bytes, bit: int = 3) -> bytes:
        return bytes([x[0] ^ (1 << bit)]) + x[1:]

    out = []
    for name, u, w in (("U and W", U, W), ("U alone", U, None), ("W alone", None, W), ("neither", None, None)):
        rows = []
        for i in range(3):
            a, A, b, B = rnd()
            rows.append((f"valid {i}", a, A, b, B, lhs(a, A, u, b, B, w, False), 1))
        a, A, b, B = rnd()
        T = lhs(a, A, u, b, B, w, False)
        rows += [("a tampered", sc(int.from_bytes(a, "little") + 1), A, b, B, T, 0),
                 ("b tampered", a, A, sc(int.from_bytes(b, "little") + 1), B, T, 0),
                 ("A tampered", a, _add(A, _pt(1)), b, B, T, 0),
                 ("B tampered", a, A, b, _add(B, _pt(1)), T, 0),
                 ("T tampered", a, A, b, B, _add(T, _pt(1)), 0),
                 ("T off the curve", a, A, b, B, bad, 0),
                 ("A undecodable", a, bad, b, B, T, 0),
                 ("B undecodable", a, A, b, bad, T, 0)]
        # unreduced scalars, for a and for b; T is the constant-time value, so the row passes without KYB_F_VARTIME
        for k, v in enumerate((L, L + 5, 2**255, 2**255 + 7, 2**256 - 1)):
            rows.append((f"a = scalar {k}", raw(v), A, b, B, lhs(raw(v), A, u, b, B, w, False), None))
            rows.append((f"a = scalar {k}, vartime value", raw(v), A, b, B, lhs(raw(v), A, u, b, B, w, True), None))
            rows.append((f"b = scalar {k}", a, A, raw(v), B, lhs(a, A, u, raw(v), B, w, False), 1))
        # torsion: the verdict follows Neg(b) as a scalar; T by point negation is another point
        for t8 in (order8[0], order4[0]):
            At, Bt = _add(A, t8), _add(B, t8)
            rows.append(("torsion in A and B", a, At, b, Bt, lhs(a, At, u, b, Bt, w, False), 1))
            rows.append(("torsion, T by point negation", a, At, b, Bt, lhs(a, At, u, b, Bt, w, False, point_negation=True), 0))
        rows.append(("small-order A and B", a, order8[0], b, order8[-1], lhs(a, order8[0], u, b, order8[-1], w, False), 1))
        out.append((name, u, w, rows))
    # the shared point tampered or undecodable
    a, A, b, B = rnd()
    T = lhs(a, A, U, b, B, W, False)
    out.append(("U tampered", _add(U, _pt(1)), W, [("U tampered", a, A, b, B, T, 0)]))
    out.append(("W tampered", U, _add(W, _pt(1)), [("W tampered", a, A, b, B, T, 0)]))
    out.append(("U undecodable", bad, W, [("U undecodable", a, A, b, B, T, 0)]))
    out.append(("W undecodable", U, bad, [("W undecodable", a, A, b, B, T, 0), ("and A too", a, bad, b, B, T, 0)]))
    # Xhat or Yhat the identity: U = -A, W = -B
    out.append(("Xhat identity", _neg(A), W, [("Xhat identity", a, A, b, B, lhs(a, A, _neg(A), b, B, W, False), 1),
                                               ("Xhat identity, T tampered", a, A, b, B, T, 0)]))
    out.append(("Yhat identity", U, _neg(B), [("Yhat identity", a, A, b, B, lhs(a, A, U, b, B, _neg(B), False), 1)]))
    out.append(("both identity", _neg(A), _neg(B), [("the identity", a, A, b, B, IDENT, 1),
                                                    ("as y + p", a, A, b, B, (O.P + 1).to_bytes(32, "little"), 1),
                                                    ("as -0", a, A, b, B, IDENT[:31] + bytes([0x80]), 1),
                                                    ("as y + p and -0", a, A, b, B, (O.P + 1 | 1 << 255).to_bytes(32, "little"), 1)]))
    # a point of order 4 (y = 0) as the value: T as y + p = p, under either sign of x
    q4 = order4[0]
    one = raw(1)
    sign = q4[31] & 0x80
    out.append(("order 4", None, None, [("y = 0", one, q4, raw(0), A, q4, 1),
                                        ("y = 0 as p", one, q4, raw(0), A, (O.P | sign << 248).to_bytes(32, "little"), 1),
                                        ("y = 0 as p, other sign", one, q4, raw(0), A, (O.P | (sign ^ 0x80) << 248).to_bytes(32, "little"), 0)]))
    return out
