"""Cases shared by the ECIES / deal-check tests on the CPU (tests/test_ecies_host.py: the lane programs compiled for the
host) and on the GPU (tests/test_gpu_ecies.py, tests/test_gpu_deal_check.py): the special encodings, the share table of
a deal check and its expected verdicts from the big-integer oracle."""
import hashlib

from oracle import ed25519 as O

L = O.L
IDENTITY = O.encode(O.IDENTITY)
# a point of order 8 (its y is one of the two the reference's weakKeys list holds for that order)
ORDER8 = bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a")
# y = p + 1 = 1 mod p: the identity written with a non-canonical y, which FromBytes accepts (ge.go:110-150)
NONCANONICAL = (O.P + 1).to_bytes(32, "little")


def _undecodable() -> bytes:
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


UNDECODABLE = _undecodable()
assert O.decode(ORDER8) is not None and O.mul_int(8, O.decode(ORDER8)) == O.IDENTITY and O.mul_int(4, O.decode(ORDER8)) != O.IDENTITY
assert O.decode(NONCANONICAL) == O.IDENTITY

# the indices of every deal-check test (x = index + 1: 2^32 - 1 evaluates at 2^32, a 33-bit x)
INDICES = (0, 1, 2, 254, 255, 2**16 - 1, 2**31, 2**32 - 2, 2**32 - 1)


def scalar(seed: bytes) -> int:
    return int.from_bytes(hashlib.sha512(seed).digest(), "little") % L


def le(x: int) -> bytes:
    return x.to_bytes(32, "little")


def eval_scalar(coeffs, idx: int) -> int:
    """PriPoly.Eval (share/poly.go:85-93) at x = idx + 1"""
    x, v = idx + 1, 0
    for c in reversed(coeffs):
        v = (v * x + c) % L
    return v


def eval_commits(commits, idx: int):
    """PubPoly.Eval (share/poly.go:340-348) at x = idx + 1 on encoded commitments: the encoded point, or None when one
    does not decode"""
    pts = [O.decode(c) for c in commits]
    if any(p is None for p in pts):
        return None
    x, v = idx + 1, O.IDENTITY
    for p in reversed(pts):
        v = O.add(O.mul_int(x, v), p)
    return O.encode(v)


def expected_ok(share: bytes, commits, idx: int) -> int:
    """dkg.go:488-495: Equal(Mul(share, nil), Eval(idx).V), the share's 32 bytes never reduced"""
    v = eval_commits(commits, idx)
    return int(v is not None and O.mul_base(share) == v)


def share_table(coeffs, idx: int):
    """(label, share bytes) rows for a polynomial with these secret coefficients at this index: the right share, the
    right share + 1, + l (the same scalar mod l, so the same point), and two scalars at and above 2^255 whose value is
    mul_base's"""
    s = eval_scalar(coeffs, idx)
    rows = [("right", le(s)), ("right + 1", le((s + 1) % L)), ("right + l", le(s + L)),
            ("2^255 + right", le(s + 2**255)), ("all ones", b"\xff" * 32)]
    return rows
