"""The DLEQ proofs the host-harness test and the GPU test share: rows of (G, H, xG, xH, C, R, VG, VH), each 32 bytes,
built on the oracle (no GPU, no engine)."""
import random

import numpy as np

from oracle import ed25519 as O
from tests import _ed_verify_oracle as V
from tests import _pvss_oracle as PO

FIELDS = ("G", "H", "xG", "xH", "C", "R", "VG", "VH")
POINT_SLOTS = (0, 1, 2, 3, 6, 7)
EDGE_SCALARS = [0, 1, O.L, O.L - 1, 2**255, 2**256 - 1]  # the scalar edge list of tests/test_gpu_ed25519.py
IDENT = O.encode(O.IDENTITY)


def _b(v: int) -> bytes:
    return v.to_bytes(32, "little")


def valid_proof(rng, fs=False):
    """a proof that verifies; fs: its challenge is the Fiat-Shamir one (dleq.go:57-79), else a random scalar"""
    rp = lambda: O.encode(O.mul_int(rng.getrandbits(252) + 1, O.B))
    G, H = rp(), rp()
    x, v = rng.getrandbits(252) % O.L, rng.getrandbits(252) % O.L
    xG, xH, vG, vH = (O.encode(O.mul_int(k, O.decode(p))) for k, p in ((x, G), (x, H), (v, G), (v, H)))
    c = PO.dleq_challenge(xG, xH, vG, vH) if fs else _b(rng.getrandbits(252) % O.L)
    return [G, H, xG, xH, c, PO.sc(v - PO.le(c) * x), vG, vH]


def small_y_point():
    """a curve point with 2 <= y < 19: its y + p still fits 255 bits"""
    for y in range(2, 19):
        if O.decode(_b(y)) is not None:
            return _b(y)
    raise AssertionError("no curve point with a small y")


def cases(seed=3, nvalid=12, fs=False):
    """(rows, labels): valid proofs, every field tampered, an undecodable encoding in every point slot, non-canonical
    but equal commitments, unreduced scalars, the scalar edge list"""
    rng = random.Random(seed)
    rows, labels = [], []

    def put(row, label):
        rows.append([bytes(f) for f in row])
        labels.append(label)

    for _ in range(nvalid):
        put(valid_proof(rng, fs), "valid")
    for k, name in enumerate(FIELDS):  # one bit of one field
        row = valid_proof(rng, fs)
        row[k] = bytes([row[k][0] ^ 1]) + row[k][1:]
        put(row, "tampered-" + name)
        row = valid_proof(rng, fs)
        row[k] = row[k][:17] + bytes([row[k][17] ^ 0x20]) + row[k][18:]
        put(row, "tampered-" + name)
    bad = V._not_on_curve()
    for k in POINT_SLOTS:
        row = valid_proof(rng, fs)
        row[k] = bad
        put(row, "undecodable-" + FIELDS[k])
    # vG = y + p: G has a small y, x = 0, r = 1, so a = G and the commitment can be written non-canonically
    P0 = small_y_point()
    H = O.encode(O.mul_int(rng.getrandbits(250) + 1, O.B))
    c = _b(rng.getrandbits(250))
    put([P0, H, IDENT, IDENT, c, _b(1), _b(PO.le(P0) + O.P), H], "vG-plus-p")
    put([H, P0, IDENT, IDENT, c, _b(1), H, _b(PO.le(P0) + O.P)], "vH-plus-p")
    put([P0, H, IDENT, IDENT, c, _b(1), _b(PO.le(P0) + O.P + 1), H], "vG-plus-p-wrong")
    # a = identity (r = 0, xG = identity) and vG = the identity with the sign bit set ("-0")
    neg0 = _b(1 | 1 << 255)
    G2 = O.encode(O.mul_int(rng.getrandbits(250) + 1, O.B))
    put([G2, H, IDENT, IDENT, c, _b(0), neg0, IDENT], "vG-minus-zero")
    put([G2, H, IDENT, IDENT, c, _b(0), IDENT, _b(O.P - 1 | 1 << 255)], "vH-wrong-x0-point")
    put([G2, H, IDENT, IDENT, c, _b(0), _b(O.P + 1 | 1 << 255), neg0], "both-minus-zero-noncanonical")
    # unreduced scalars: c + l and r + l are other byte strings (and, as challenges, other challenges)
    for k, name in ((4, "C"), (5, "R")):
        row = valid_proof(rng, fs)
        row[k] = _b(PO.le(row[k]) + O.L)
        put(row, name + "-plus-l")
    # the scalar edge list against itself, the commitments set to what the equations give
    for vartime_points in (False,):
        for cs in EDGE_SCALARS:
            for rs in EDGE_SCALARS:
                row = valid_proof(rng, False)
                row[4], row[5] = _b(cs), _b(rs)
                put(row, "edge-scalars")
    return rows, labels


def commitments_from_equations(row, vartime):
    """the row with VG, VH replaced by r G + c xG and r H + c xH under the given flag: valid by construction"""
    G, H, xG, xH, C, R = row[:6]
    a = O.add(O.decode(O.mul(R, G, vartime)), O.decode(O.mul(C, xG, vartime)))
    b = O.add(O.decode(O.mul(R, H, vartime)), O.decode(O.mul(C, xH, vartime)))
    return row[:6] + [O.encode(a), O.encode(b)]


def pack(rows):
    """eight (n, 32) uint8 arrays"""
    n = len(rows)
    return [np.frombuffer(b"".join(r[k] for r in rows), dtype=np.uint8).reshape(n, 32).copy() for k in range(8)]


def oracle_ok(rows, vartime=False):
    return np.array([PO.dleq_verify(*r, vartime=vartime) for r in rows], dtype=bool)


def challenge_inputs(n, seed=9):
    """n x (xG, xH, vG, vH) for the challenge kernel: random byte strings (the challenge is defined on every input),
    with non-canonical encodings -- y + p, both signs of x = 0 -- sprinkled in"""
    rng = random.Random(seed)
    special = [_b(1), _b(1 | 1 << 255), _b(O.P - 1), _b(O.P - 1 | 1 << 255), _b(O.P), _b(O.P + 1), _b(O.P + 1 | 1 << 255),
               _b(2**255 - 1), _b(2**256 - 1), _b(0), _b(1 << 255), _b(O.P + 7), _b(O.P - 2)]
    out = []
    for i in range(n):
        row = [rng.getrandbits(256).to_bytes(32, "little") for _ in range(4)]
        if i % 5 == 0:
            row[rng.randrange(4)] = special[(i // 5) % len(special)]
        out.append(row)
    return out
