"""sign/eddsa VerifyWithChecks (eddsa.go:143-229) restated in Python with reason codes, on oracle/ed25519.py, and the
vectors the verify tests share (no GPU, no engine): the checker of kyb_ed25519_verify, never the thing shipped."""
import hashlib
import json
import os

import numpy as np

from oracle import ed25519 as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# reasons, in the order the reference meets them
OK, LENGTH, S_NONCANONICAL, R_NONCANONICAL, R_NOT_A_POINT, R_SMALL_ORDER = "ok", "length", "s-noncanonical", "r-noncanonical", "r-not-a-point", "r-small-order"
A_NONCANONICAL, A_NOT_A_POINT, A_SMALL_ORDER, EQUATION = "a-noncanonical", "a-not-a-point", "a-small-order", "equation"
REASONS = (OK, LENGTH, S_NONCANONICAL, R_NONCANONICAL, R_NOT_A_POINT, R_SMALL_ORDER, A_NONCANONICAL, A_NOT_A_POINT,
           A_SMALL_ORDER, EQUATION)

ST_OK, ST_BAD_POINT, ST_SIG_NONCANONICAL, ST_SIG_SMALL_ORDER = 0, 1, 5, 6  # include/kyber_hip.h
_MASK = (1 << 255) - 1


def point_is_canonical(b: bytes) -> bool:  # point.go:296-323
    return (int.from_bytes(b, "little") & _MASK) < O.P


def has_small_order(pt) -> bool:  # point.go:262-294: the canonical encoding is one of weakKeys <=> [8]P is the identity
    return O.mul_int(8, pt) == O.IDENTITY


def _byte_checks(pub: bytes, sig: bytes, r_decode: bool):
    """the checks before the equation; r_decode = False leaves R's decoding out, as the engine does"""
    if int.from_bytes(sig[32:], "little") >= O.L:  # scalar.go:2308-2333
        return S_NONCANONICAL
    if not point_is_canonical(sig[:32]):
        return R_NONCANONICAL
    R = O.decode(sig[:32])
    if R is None:
        if r_decode:
            return R_NOT_A_POINT
    elif has_small_order(R):
        return R_SMALL_ORDER
    if not point_is_canonical(pub):
        return A_NONCANONICAL
    A = O.decode(pub)
    if A is None:
        return A_NOT_A_POINT
    if has_small_order(A):
        return A_SMALL_ORDER
    return None


def verify_with_checks(pub: bytes, msg: bytes, sig: bytes):
    """(ok, reason) of VerifyWithChecks(pub, msg, sig)"""
    if len(sig) != 64 or len(pub) != 32:  # (a public key of another length fails IsCanonical in the reference)
        return False, LENGTH
    why = _byte_checks(pub, sig, True)
    if why:
        return False, why
    R, A = O.decode(sig[:32]), O.decode(pub)
    h = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % O.L
    S = int.from_bytes(sig[32:], "little")
    good = O.encode(O.add(R, O.mul_int(h, A))) == O.encode(O.mul_int(S, O.B))
    return good, (OK if good else EQUATION)


def abi_status(pub: bytes, msg: bytes, sig: bytes) -> int:
    """status[i] of kyb_ed25519_verify as include/kyber_hip.h documents it: the reference's order of checks, R's own
    decoding left to the equation (status 0, ok 0)"""
    why = _byte_checks(pub, sig, False)
    return {None: ST_OK, S_NONCANONICAL: ST_SIG_NONCANONICAL, R_NONCANONICAL: ST_SIG_NONCANONICAL, A_NONCANONICAL: ST_SIG_NONCANONICAL,
            R_SMALL_ORDER: ST_SIG_SMALL_ORDER, A_SMALL_ORDER: ST_SIG_SMALL_ORDER, A_NOT_A_POINT: ST_BAD_POINT}[why]


# ------------------------------------------------------------------------------------------------- vectors
def sign_input():
    """[(pub, msg, sig)] of the 384 committed SUPERCOP rows, message lengths 0..383"""
    z = np.load(os.path.join(GOLDEN, "ed25519_sign_input_msgs.npz"))
    off, m = z["off"], z["msgs"].tobytes()
    return [(z["pub"][i].tobytes(), m[int(off[i]):int(off[i + 1])], z["sig"][i].tobytes()) for i in range(len(off) - 1)]


def _misc():
    return json.load(open(os.path.join(GOLDEN, "ed25519_misc.json")))


def wycheproof():
    """[(pub, msg, sig, valid)] of the 150 Wycheproof cases (signatures of any length)"""
    return [(bytes.fromhex(c["pk"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bool(c["valid"])) for c in _misc()["wycheproof"]]


def rfc8032():
    return [(bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"])) for c in _misc()["rfc8032"]]


def _not_on_curve():
    """a canonical y with no x: the smallest y >= 2 for which decoding fails"""
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


def synthetic_rejects():
    """[(pub, msg, sig)]: what Wycheproof lacks -- every failure on the public key, and the same encodings as R.
    The five small-order encodings and their sign-bit twins, y = p + k for 0 <= k < 19, a y not on the curve; each put
    in A's place and in R's place of a valid row (the rest of the row untouched)."""
    pub, msg, sig = sign_input()[33]
    small = [bytes.fromhex(h) for h in _misc()["small_order"]]
    small += [s[:31] + bytes([s[31] | 0x80]) for s in small]
    noncanon = [(O.P + k).to_bytes(32, "little") for k in range(19)]
    noncanon += [(O.P + k | 1 << 255).to_bytes(32, "little") for k in (0, 18)]
    off_curve = [_not_on_curve()]
    off_curve.append(off_curve[0][:31] + bytes([off_curve[0][31] | 0x80]))
    out = []
    for enc in small + noncanon + off_curve:
        out.append((enc, msg, sig))
        out.append((pub, msg, enc + sig[32:]))
    # both at once: the reference stops at R's check
    out.append((small[2], msg, noncanon[0] + sig[32:]))
    out.append((noncanon[3], msg, small[3] + sig[32:]))
    out.append((noncanon[3], msg, off_curve[0] + sig[32:]))  # R no point, A not canonical: the ABI reports A's status
    # S = l + S0 (the same residue, not canonical) and S = l - 1, l
    s0 = int.from_bytes(sig[32:], "little")
    for s in (s0 + O.L, O.L - 1, O.L, 2**256 - 1):
        out.append((pub, msg, sig[:32] + s.to_bytes(32, "little")))
    return out


def all_cases():
    """[(pub, msg, sig)] with 64-byte signatures and 32-byte keys: everything the engine can be handed"""
    cases = sign_input() + rfc8032() + synthetic_rejects()
    cases += [(p, m, s) for p, m, s, _ in wycheproof() if len(s) == 64 and len(p) == 32]
    return cases


def pack(cases):
    """(pubs (n, 32), msgs (bytes,), off (n + 1,) uint64, sigs (n, 64)) for the C ABI"""
    n = len(cases)
    pubs = np.frombuffer(b"".join(c[0] for c in cases), dtype=np.uint8).reshape(n, 32).copy()
    sigs = np.frombuffer(b"".join(c[2] for c in cases), dtype=np.uint8).reshape(n, 64).copy()
    blob = b"".join(c[1] for c in cases)
    msgs = np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(1, dtype=np.uint8)
    off = np.cumsum([0] + [len(c[1]) for c in cases]).astype(np.uint64)
    return pubs, msgs, off, sigs
