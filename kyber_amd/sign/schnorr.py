"""Host-side mirror of ``sign/schnorr`` for the Ed25519 group: verification (schnorr.go:84-160 VerifyWithChecks) as the
engine's fused batch call, ``Sign`` (schnorr.go:56-82) as host scalar arithmetic around the engine's fixed-base
multiplication, ``SignBatch`` -- n ``Sign``s as ONE kyb_ed25519_schnorr_sign, points, hash and response on the device --
and the ``sign.Scheme`` (schnorr.go:31-51) that ``share/dkg``'s Config.Auth is.

On this curve it is the engine call of ``sign/eddsa``: the reference hashes ``R.MarshalTo || public.MarshalTo || msg``
(schnorr.go:171-183), and MarshalTo of a point that passed IsCanonical returns the bytes it was decoded from, so the
hash is over the same bytes R || A || msg; the checks are the same set in another order (a verdict does not depend on
which failing check is met first); the equation is S*B == R + h*A; and the Ed25519 point type is no
``kyber.SubGroupElement``, so the IsInCorrectGroup branch (schnorr.go:121-123) is never taken.
tests/test_gpu_ed_verify.py holds this module against the oracle's restatement on the reference's vectors.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import eddsa
from ..group import edwards25519 as ed


def batch_verify_with_checks(pubs, msgs, sigs) -> np.ndarray:
    """ok[i] = (schnorr.VerifyWithChecks(edwards25519, pubs[i], msgs[i], sigs[i]) == nil)."""
    return eddsa.batch_verify_with_checks(pubs, msgs, sigs)


def _hash(public: bytes, R: bytes, msg: bytes) -> ed.Scalar:
    """schnorr.go:171-183: SetBytes(SHA-512(R || public || msg))"""
    return ed.Scalar().SetBytes(hashlib.sha512(R + public + bytes(msg)).digest())


def Sign(suite, private, msg: bytes, rand=None) -> bytes:
    """schnorr.go:56-82: R || S with k = Scalar.Pick(rand), R = k B, S = k + x * H(R || x B || msg).  rand: what
    ``Scalar.Pick`` takes (the reference draws from the suite's RandomStream); the two fixed-base multiplications are one
    engine call under KYB_F_UNIFORM: both scalars are secrets."""
    k = suite.Scalar().Pick(rand)
    out = ed.batch_mul_base(ed._sc(k).v + ed._sc(private).v, uniform=True)
    R, public = bytes(out[0]), bytes(out[1])
    h = _hash(public, R, msg)
    S = suite.Scalar().Add(k, suite.Scalar().Mul(private, h))
    return R + S.MarshalBinary()


def SignBatch(suite, privates, msgs, rand=None) -> list:
    """[Sign(suite, privates[i], msgs[i], rand) for i in range(n)] as ONE engine call (kyb_ed25519_schnorr_sign): both
    fixed-base multiplications, the hash and S = k + x h on the device.  The nonces are drawn here, one Scalar.Pick per
    message in input order: what n sequential Signs draw from the same stream.  privates: one scalar per message, or ONE
    scalar that signs them all.  rand: one stream for the batch, or a list with one stream per message (signers that
    each draw from their own)."""
    msgs = [bytes(m) for m in msgs]
    one = not isinstance(privates, (list, tuple))
    if not one and len(privates) != len(msgs):
        raise ValueError("privates/msgs length mismatch")
    rands = list(rand) if isinstance(rand, (list, tuple)) else [rand] * len(msgs)
    if len(rands) != len(msgs):
        raise ValueError("rand/msgs length mismatch")
    ks = b"".join(ed._sc(suite.Scalar().Pick(r)).v for r in rands)
    if not msgs:
        return []
    x = ed._sc(privates).v if one else b"".join(ed._sc(p).v for p in privates)
    sigs, _ = ed.batch_schnorr_sign(ks, x, msgs)
    return [bytes(s) for s in sigs]


def Verify(suite, public, msg: bytes, sig: bytes) -> None:
    """schnorr.go:163-169: raises ValueError unless sig is a valid signature of msg under public."""
    if not batch_verify_with_checks([public.MarshalBinary()], [bytes(msg)], [bytes(sig)])[0]:
        raise ValueError("schnorr: invalid signature")


class Scheme:
    """sign.Scheme over sign/schnorr (schnorr.go:31-51).  rand: the stream Sign and NewKeyPair draw from."""

    def __init__(self, suite, rand=None):
        self.s, self.rand = suite, rand

    def NewKeyPair(self, rand=None):
        priv = self.s.Scalar().Pick(rand if rand is not None else self.rand)
        return priv, self.s.Point().Mul(priv, None)

    def Sign(self, private, msg: bytes) -> bytes:
        return Sign(self.s, private, msg, self.rand)

    def Verify(self, public, msg: bytes, sig: bytes) -> None:
        Verify(self.s, public, msg, sig)


def NewScheme(suite, rand=None) -> Scheme:
    return Scheme(suite, rand)
