"""Host-side mirror of ``util/key`` (key.go:22-49): a public/private key pair and its generation.

``Pair.Gen`` asks the suite for ``NewKey`` when it is a ``key.Generator`` -- the Ed25519 suite is one (curve.go:71-76:
32 stream bytes, SHA-512, clamped, stored unreduced) -- and otherwise picks a scalar from the stream; the public key is
``Mul(Private, nil)``.  The reference reads ``suite.RandomStream()``; here the caller hands the stream in, as
``sign/anon.Sign`` does.
"""
from __future__ import annotations


class Pair:
    __slots__ = ("Public", "Private")

    def __init__(self, Public=None, Private=None):
        self.Public, self.Private = Public, Private

    def Gen(self, suite, rand) -> "Pair":
        """key.go:41-49"""
        self.Private = suite.NewKey(rand) if hasattr(suite, "NewKey") else suite.Scalar().Pick(rand)
        self.Public = suite.Point().Mul(self.Private, None)
        return self


def NewKeyPair(suite, rand) -> Pair:
    """key.go:29-34"""
    return Pair().Gen(suite, rand)
