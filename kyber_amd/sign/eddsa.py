"""Host-side mirror of ``sign/eddsa`` verification (eddsa.go:143-229 VerifyWithChecks) over the engine: the
reference checks S*B == R + h*A with one fixed-base and one variable-base Point.Mul per signature; here a whole
batch is one engine call (edwards25519.batch_verify -> kyb_ed25519_verify: checks, SHA-512, one ladder and the comb in
one lane program).  Only the length checks stay on the host.  ``_batch_verify_composed`` is the path this replaced --
five launches and a Python loop with the byte-level checks (scalar.go:2308-2333, point.go:262-323) and SHA-512 on the
host -- kept as the second opinion of the tests and the baseline of tools/ed_verify_probe.py.

Signing is the package function for function (eddsa.go:31-142, 231-239): ``EdDSA``, ``NewEdDSA``, ``MarshalBinary``,
``UnmarshalBinary``, ``Sign``, and ``Verify`` / ``VerifyWithChecks`` in the reference's raising form with its error
strings.  A key is expanded by ONE kyb_ed25519_eddsa_expand (SHA-512 of the seed, the clamp and secret * B in one lane)
and a message signed by ONE kyb_ed25519_eddsa_sign (both hashes, R = r * B and S = r + h * a on the device); the batch
forms ``NewEdDSABatch``, ``UnmarshalBinaryBatch`` and ``SignBatch`` make the same two calls with n elements and equal
the loops over the single forms under the same stream."""
from __future__ import annotations

import hashlib

import numpy as np

from ..group import edwards25519 as ed

_P = 2**255 - 19
# group/edwards25519/const.go:1453-1473 weakKeys: the y-coordinates (sign bit cleared) of the small-order points
_SMALL_ORDER_Y = (
    0, 1, _P - 1,
    0x7A03AC9277FDC74EC6CC392CFA53202A0F67100D760B3CBA4FD84D3D706A17C7,
    0x05FC536D880238B13933C6D305ACDFD5F098EFF289F4C345B027B2C28F95E826,
)


def _scalar_is_canonical(sb: bytes) -> bool:  # scalar.go:2308-2333
    return int.from_bytes(sb, "little") < ed.ORDER


def _point_is_canonical(pb: bytes) -> bool:  # point.go:296-323: y < p (sign bit ignored)
    return (int.from_bytes(pb, "little") & ((1 << 255) - 1)) < _P


def _has_small_order(enc: bytes) -> bool:  # point.go:262-294 on the canonical encoding
    return (int.from_bytes(enc, "little") & ((1 << 255) - 1)) in _SMALL_ORDER_Y


def batch_verify_with_checks(pubs, msgs, sigs) -> np.ndarray:
    """ok[i] = (VerifyWithChecks(pubs[i], msgs[i], sigs[i]) == nil)."""
    n = len(sigs)
    ok = np.zeros(n, dtype=bool)
    idx = [i for i in range(n) if len(sigs[i]) == 64 and len(pubs[i]) == 32]  # eddsa.go:144-146; IsCanonical's length check
    if idx:
        good, _ = ed.batch_verify([bytes(pubs[i]) for i in idx], [bytes(msgs[i]) for i in idx], [bytes(sigs[i]) for i in idx],
                                  want_status=False)
        ok[idx] = good.astype(bool)
    return ok


def _batch_verify_composed(pubs, msgs, sigs) -> np.ndarray:
    """The same verdicts from the engine's separate calls (two decoding ladders, comb, ladder, add) and host checks."""
    n = len(sigs)
    ok = np.zeros(n, dtype=bool)
    idx = []
    for i in range(n):
        pub, sig = bytes(pubs[i]), bytes(sigs[i])
        if len(sig) != 64 or len(pub) != 32:
            continue
        if not _scalar_is_canonical(sig[32:]) or not _point_is_canonical(sig[:32]) or not _point_is_canonical(pub):
            continue
        idx.append(i)
    if not idx:
        return ok
    R = np.frombuffer(b"".join(bytes(sigs[i])[:32] for i in idx), dtype=np.uint8).reshape(-1, 32)
    S = np.frombuffer(b"".join(bytes(sigs[i])[32:] for i in idx), dtype=np.uint8).reshape(-1, 32)
    A = np.frombuffer(b"".join(bytes(pubs[i]) for i in idx), dtype=np.uint8).reshape(-1, 32)
    h = np.frombuffer(b"".join(
        (int.from_bytes(hashlib.sha512(bytes(sigs[i])[:32] + bytes(pubs[i]) + bytes(msgs[i])).digest(), "little")
         % ed.ORDER).to_bytes(32, "little") for i in idx), dtype=np.uint8).reshape(-1, 32)
    one = np.zeros_like(S)
    one[:, 0] = 1
    Rc, st_r = ed.batch_mul(one, R)  # UnmarshalBinary(R): canonical re-encoding + decodability
    Ac, st_a = ed.batch_mul(one, A)
    SB = ed.batch_mul_base(S)
    hA, _ = ed.batch_mul(h, A)
    RhA, st_s = ed.batch_add(R, hA)
    for k, i in enumerate(idx):
        if st_r[k] or st_a[k] or st_s[k]:
            continue
        if _has_small_order(bytes(Rc[k])) or _has_small_order(bytes(Ac[k])):
            continue
        ok[i] = bytes(RhA[k]) == bytes(SB[k])
    return ok


# ------------------------------------------------------------------------------------------------------------ signing
_suite = ed.Curve()  # eddsa.go:15: the package's group

ErrPKMarshalling = "error unmarshalling public key"  # eddsa.go:16-29
ErrPKInvalid = "invalid public key"
ErrPKSmallOrder = "public key has small order"
ErrPKNotCanonical = "public key is not canonical"
ErrEdDSAWrongLength = "wrong length for decoding EdDSA private"
ErrSignatureLength = "signature length invalid"
ErrSignatureNotCanonical = "signature is not canonical"
ErrSignatureRecNotEqual = "reconstructed S is not equal to signature"
ErrPointRSmallOrder = "point R has small order"
ErrPointRNotCanonical = "point R is not canonical"
ErrPointRInvalid = "point R invalid"
_ErrPointDecode = "invalid Ed25519 curve point"  # point.go:65-70, wrapped behind ErrPointRInvalid and ErrPKInvalid


class EdDSA:
    """eddsa.go:31-41: Secret (hashed and bit-tweaked, unreduced), Public, and the private seed and prefix."""

    __slots__ = ("Secret", "Public", "seed", "prefix")

    def __init__(self):
        self.Secret, self.Public, self.seed, self.prefix = None, None, None, None

    def _set(self, seed: bytes, secret, prefix, pub) -> "EdDSA":
        self.seed, self.prefix = bytes(seed), bytes(prefix)
        self.Secret, self.Public = ed.Scalar(bytes(secret)), ed.Point(bytes(pub))
        return self

    def MarshalBinary(self) -> bytes:
        """eddsa.go:61-73: SUPERCOP ref10's seed || Public"""
        return self.seed + self.Public.MarshalBinary()

    def UnmarshalBinary(self, buff: bytes) -> "EdDSA":
        """eddsa.go:75-88"""
        return _expand_into([self], [_seed_of(buff)])[0]

    def Sign(self, msg: bytes) -> bytes:
        """eddsa.go:90-142"""
        return SignBatch(self, [msg])[0]

    def __eq__(self, other):
        return isinstance(other, EdDSA) and (self.seed, self.prefix, self.Secret.v, self.Public.enc) == (
            other.seed, other.prefix, other.Secret.v, other.Public.enc)

    __hash__ = None


def _seed_of(buff) -> bytes:
    """the seed of a marshalled key, seed || Public (eddsa.go:77-83; Public is recomputed, not read)"""
    buff = bytes(buff)
    if len(buff) != 64:
        raise ValueError(f"error: {ErrEdDSAWrongLength}")
    return buff[:32]


def _expand_into(keys, seeds) -> list:
    """keys[i] from seeds[i]: ONE kyb_ed25519_eddsa_expand"""
    if seeds:
        secrets, prefixes, pubs = ed.batch_eddsa_expand(b"".join(seeds))
        for k, seed, a, p, A in zip(keys, seeds, secrets, prefixes, pubs):
            k._set(seed, a, p, A)
    return keys


def NewEdDSA(stream) -> EdDSA:
    """eddsa.go:43-59"""
    return NewEdDSABatch(stream, 1)[0]


def NewEdDSABatch(stream, n: int) -> list:
    """[NewEdDSA(stream) for _ in range(n)]: the n seeds are drawn in order, each as the suite's NewKeyAndSeed draws its
    own (curve.go:62-69), and expanded together."""
    if stream is None:
        raise ValueError("stream is required")
    seeds = [bytes(_suite.NewKeyAndSeed(stream)[1]) for _ in range(n)]
    return _expand_into([EdDSA() for _ in seeds], seeds)


def UnmarshalBinaryBatch(buffs) -> list:
    """[EdDSA().UnmarshalBinary(b) for b in buffs]; the length of every buffer is checked before any is expanded"""
    seeds = [_seed_of(b) for b in buffs]
    return _expand_into([EdDSA() for _ in seeds], seeds)


def SignBatch(keys, msgs) -> list:
    """[keys[i].Sign(msgs[i]) for i in range(n)] as ONE kyb_ed25519_eddsa_sign.  keys: one EdDSA that signs every message,
    or a list of n."""
    msgs = [bytes(m) for m in msgs]
    ks = [keys] if isinstance(keys, EdDSA) else list(keys)
    if not isinstance(keys, EdDSA) and len(ks) != len(msgs):
        raise ValueError("keys/msgs length mismatch")
    if not msgs:
        return []
    sigs, _ = ed.batch_eddsa_sign(b"".join(ed._sc(k.Secret).v for k in ks), b"".join(k.prefix for k in ks),
                                  b"".join(ed._pt(k.Public).MarshalBinary() for k in ks), msgs)
    return [bytes(s) for s in sigs]


def _point_decodes(pb: bytes) -> bool:
    """Point.UnmarshalBinary accepts the encoding (ge.go FromBytes): (y^2 - 1) / (d y^2 + 1) is a square.  Euler's
    criterion on Python integers; it runs only to name the error of a signature the engine has already rejected."""
    y = (int.from_bytes(pb, "little") & ((1 << 255) - 1)) % _P
    d = -121665 * pow(121666, _P - 2, _P) % _P
    x2 = (y * y - 1) * pow(d * y * y + 1, _P - 2, _P) % _P
    return x2 == 0 or pow(x2, (_P - 1) // 2, _P) == 1


def _rejection(pub: bytes, sig: bytes, status: int) -> str:
    """the error VerifyWithChecks returns for a 64-byte signature the engine rejected, in the reference's order
    (eddsa.go:162-227).  status: kyb_ed25519_verify's, which has A's decoding; R's own is left to the equation there."""
    R, S = sig[:32], sig[32:]
    if not _scalar_is_canonical(S):
        return f"error: {ErrSignatureNotCanonical}"
    if not _point_is_canonical(R):
        return f"error: {ErrPointRNotCanonical}"
    if not _point_decodes(R):
        return f"error: {ErrPointRInvalid}: {_ErrPointDecode}"
    if _has_small_order(R):
        return f"error: {ErrPointRSmallOrder}"
    if len(pub) != 32 or not _point_is_canonical(pub):
        return f"error: {ErrPKNotCanonical}"
    if status == ed._lib.ST_BAD_POINT:
        return f"error: {ErrPKInvalid}: {_ErrPointDecode}"
    if _has_small_order(pub):
        return f"error: {ErrPKSmallOrder}"
    return f"error: {ErrSignatureRecNotEqual}"


def VerifyWithChecks(pub: bytes, msg: bytes, sig: bytes) -> None:
    """eddsa.go:144-229: returns None for a valid signature and raises ValueError with the reference's error text
    otherwise.  One engine call (kyb_ed25519_verify); what a rejected signature is rejected for is read off its bytes."""
    pub, msg, sig = bytes(pub), bytes(msg), bytes(sig)
    if len(sig) != 64:
        raise ValueError(f"error: {ErrSignatureLength}: expect 64 but got {len(sig)}")
    status = 0
    if len(pub) == 32:  # (a key of another length fails IsCanonical, below)
        ok, st = ed.batch_verify([pub], [msg], [sig])
        if ok[0]:
            return
        status = int(st[0])
    raise ValueError(_rejection(pub, sig, status))


def Verify(public, msg: bytes, sig: bytes) -> None:
    """eddsa.go:231-239"""
    VerifyWithChecks(ed._pt(public).MarshalBinary(), msg, sig)
