"""Scalars and points that reach every way the two Ed25519 walks can start (ed25519_dev.cuh: ge_scalarmult_w4_p1p1 from
its top digit's table entry, ed_comb_walk from position 0's row), shared by tests/test_ed25519_walk_start_host.py and
tests/test_gpu_ed25519_walk_start.py."""
import hashlib

from oracle import ed25519 as O

ELL = O.L


def scalars():
    """every top digit 0 .. 8 of the window walk, every position-0 digit -8 .. 8 of the comb with nothing else set, the
    group order's neighbours and the edges of the two scalar semantics, as 32 little-endian bytes"""
    v = [0, 1, 8]
    v += [16**63 * k for k in range(1, 9)]                  # top digit k, every other digit zero
    v += [16**63 * k + 0x7654321 for k in range(0, 9)]      # top digit k over low digits that add
    v += [16**62 * 9 + 16**63 * k for k in (0, 3, 7)]        # a carry into the top digit: k + 1
    v += [ELL - 1, ELL, 2**252 - 1, 2**252 + 1, 2**255 - 1, 2**255, 2**256 - 1]
    v += list(range(2, 8))                                  # comb position 0 alone: digit d ...
    v += [2**256 - d for d in range(1, 9)]                  # ... and -d (constant structure: the top digit is dropped)
    v += [2**64 - 1, 2**64 - 3, 2**128 + 5, 16**17 * 8]      # short scalars: KYB_F_VARTIME starts below digit 63
    v += [int("8" * 64, 16), int("7" * 64, 16)]
    out, seen = [], set()
    for x in v:
        if x not in seen:
            seen.add(x)
            out.append(x.to_bytes(32, "little"))
    return out


def points():
    """the base, the identity, a point of order 2, 4 and 8 (two of those), and twenty points derived from SHAKE-256"""
    pts = [O.encode(O.B), O.encode(O.IDENTITY), (O.P - 1).to_bytes(32, "little"), bytes(32),
           bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05"),
           bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a")]
    for order, enc in zip((2, 4, 8, 8), pts[2:]):
        pt = O.decode(enc)
        assert O.mul_int(order, pt) == O.IDENTITY and O.mul_int(order // 2, pt) != O.IDENTITY
    i = 0
    while len(pts) < 26:
        enc = hashlib.shake_256(b"ed-walk-start %d" % i).digest(32)
        i += 1
        if O.decode(enc) is not None:
            pts.append(enc)
    return pts


def top_digit(s: bytes) -> int:
    """digit 63 of the constant-structure recoding (a digit above 8 is dropped there)"""
    return O.recode_radix16(s)[63]
