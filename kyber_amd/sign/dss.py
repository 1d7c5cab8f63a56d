"""Host-side mirror of ``sign/dss`` (dss.go), the distributed Schnorr signature of Stinson and Strobl, for the Ed25519
group, function for function, with the reference's error strings in their order.  The sequential functions compose the
standing calls (sign/schnorr Sign and Verify, ``PubPoly.Eval``, ``Point.Mul``); three batch functions are the engine's:

  ``PartialSigBatch(dsss)``       n ``PartialSig()`` of DSS objects that share signer, roster and long-term share as ONE
                                  kyb_ed25519_dss_partial: h, V, the session id, both hashes and the signature on the
                                  device; nonces are read from the stream as n sequential ``PartialSig`` read them.
  ``process_partial_sigs(pairs)`` ``dss.ProcessPartialSig(ps)`` for (dss, ps) pairs over one roster and one long-term key
                                  as ONE kyb_ed25519_dss_check, then the sequential rules -- duplicates, ``partials``,
                                  ``partialsIdx`` -- on the host in list order; one error-or-None per pair, what the loop
                                  returns.
  ``SignatureBatch(dsss)``        ``Signature()`` of each: ``recover_secret`` on the host (B t^2 scalar operations).

A threshold signer spends one random distributed key per signature, so a service that signs B messages runs B sessions:
each of its n participants issues B partial signatures and checks B (n - 1).  The long-term polynomial and the roster are
the same for every session, which is what the two calls share.

Errors are raised as ValueError with the reference's text; ``ErrInvalidSignatureIndex`` is the one it exports."""
from __future__ import annotations

import hashlib
import struct

from . import eddsa, schnorr
from .. import _lib
from ..group import edwards25519 as ed
from ..share import poly as share


class Suite:
    """dss.go:27-32: kyber.Group, kyber.HashFactory and kyber.Random -- what ``edwards25519.NewSuite()`` is; spelled out
    for callers that bring their own"""

    def Scalar(self): ...
    def Point(self): ...
    def Hash(self): ...
    def RandomStream(self): ...


class DistKeyShare:
    """dss.go:34-40, a duck type: ``PriShare()`` (a share.PriShare) and ``Commitments()`` (a list of points), as
    share/dkg/rabin's DistKeyShare has them"""

    def PriShare(self): ...
    def Commitments(self): ...


ErrInvalidSignatureIndex = ValueError("dss: partial signature with invalid index")


def _hash(suite):
    return suite.Hash() if hasattr(suite, "Hash") else hashlib.sha256()


class PartialSig:
    """dss.go:62-68"""

    def __init__(self, Partial, SessionID: bytes, Signature: bytes = b""):
        self.Partial, self.SessionID, self.Signature = Partial, SessionID, Signature

    def Hash(self, s=None) -> bytes:  # dss.go:221-226 over PriShare.Hash (share/poly.go:35-40)
        inner = _hash(s)
        inner.update(ed._sc(self.Partial.V).MarshalBinary() + struct.pack("<I", self.Partial.I))
        h = _hash(s)
        h.update(inner.digest() + bytes(self.SessionID))
        return h.digest()


def _commit_bytes(dks) -> list:
    return [ed._pt(p).MarshalBinary() for p in dks.Commitments()]


def sessionID(suite, a, b) -> bytes:  # dss.go:235-246
    h = _hash(suite)
    h.update(b"".join(_commit_bytes(a)) + b"".join(_commit_bytes(b)))
    return h.digest()


def findPub(participants, i: int):  # dss.go:228-233
    if i >= len(participants):
        return None, False
    return participants[i], True


class DSS:
    """dss.go:42-60"""

    def __init__(self, suite, secret, public, index, participants, long, random, msg, t, rand=None):
        self.suite, self.secret, self.public, self.index = suite, secret, public, index
        self.participants, self.T, self.long, self.random = participants, t, long, random
        self.longPoly = share.PubPoly(suite, suite.Point().Base(), long.Commitments())
        self.randomPoly = share.PubPoly(suite, suite.Point().Base(), random.Commitments())
        self.msg, self.partials, self.partialsIdx, self.signed = bytes(msg), [], {}, False
        self.sessionID = sessionID(suite, long, random)
        self.rand = rand  # what schnorr.Sign draws its nonce from (the reference: the suite's RandomStream)

    def PartialSig(self) -> PartialSig:  # dss.go:113-134
        alpha, beta = self.long.PriShare().V, self.random.PriShare().V
        right = self.suite.Scalar().Mul(self.hashSig(), alpha)
        ps = PartialSig(share.PriShare(self.index, right.Add(right, beta)), self.sessionID)
        ps.Signature = schnorr.Sign(self.suite, self.secret, ps.Hash(self.suite), self.rand)
        self._own(ps)
        return ps

    def _own(self, ps: PartialSig) -> None:
        if not self.signed:
            self.partialsIdx[self.index] = True
            self.partials.append(ps.Partial)
            self.signed = True

    def ProcessPartialSig(self, ps: PartialSig) -> None:  # dss.go:141-173
        public, ok = findPub(self.participants, ps.Partial.I)
        if not ok:
            raise ErrInvalidSignatureIndex
        schnorr.Verify(self.suite, public, ps.Hash(self.suite), ps.Signature)
        if bytes(ps.SessionID) != self.sessionID:
            raise ValueError("dss: session id do not match")
        if ps.Partial.I in self.partialsIdx:
            raise ValueError("dss: partial signature already received from peer")
        h, idx = self.hashSig(), ps.Partial.I
        randShare, longShare = self.randomPoly.Eval(idx), self.longPoly.Eval(idx)
        right = self.suite.Point().Mul(h, longShare.V)
        right.Add(randShare.V, right)
        left = self.suite.Point().Mul(ps.Partial.V, None)
        if not left.Equal(right):
            raise ValueError("dss: partial signature not valid")
        self._accept(ps)

    def _accept(self, ps: PartialSig) -> None:
        self.partialsIdx[ps.Partial.I] = True
        self.partials.append(ps.Partial)

    def EnoughPartialSig(self) -> bool:  # dss.go:178-180
        return len(self.partials) >= self.T

    def Signature(self) -> bytes:  # dss.go:186-199
        if not self.EnoughPartialSig():
            raise ValueError("dkg: not enough partial signatures to sign")
        gamma = share.recover_secret(self.suite, self.partials, self.T, len(self.participants))
        return ed._pt(self.random.Commitments()[0]).MarshalBinary() + gamma.MarshalBinary()  # RandomPublic || gamma

    def hashSig(self):  # dss.go:201-211: H(R || A || msg)
        h = hashlib.sha512(_commit_bytes(self.random)[0] + _commit_bytes(self.long)[0] + self.msg)
        return self.suite.Scalar().SetBytes(h.digest())


def NewDSS(suite, secret, participants, long, random, msg: bytes, t: int, rand=None) -> DSS:  # dss.go:77-107
    public = suite.Point().Mul(secret, None)
    for j, p in enumerate(participants):
        if p.Equal(public):
            return DSS(suite, secret, public, j, participants, long, random, msg, t, rand)
    raise ValueError("dss: public key not found in list of participants")


def Verify(public, msg: bytes, sig: bytes) -> None:  # dss.go:215-217: eddsa.Verify
    if not eddsa.batch_verify_with_checks([ed._pt(public).MarshalBinary()], [bytes(msg)], [bytes(sig)])[0]:
        raise ValueError("eddsa: invalid signature")


# ---------------------------------------------------------------------------------------------------- the batch entries
def _same_key(dsss, what: str):
    """the roster and the long-term commitments every DSS of a batch shares, as bytes"""
    first = dsss[0]
    pk = [ed._pt(p).MarshalBinary() for p in first.participants]
    lc = _commit_bytes(first.long)
    for d in dsss[1:]:
        if d.participants is not first.participants and [ed._pt(p).MarshalBinary() for p in d.participants] != pk:
            raise ValueError(what + ": one roster")
        if d.long is not first.long and _commit_bytes(d.long) != lc:
            raise ValueError(what + ": one long-term key")
    return pk, lc


def _rand_commits(dsss, what: str):
    rc = [_commit_bytes(d.random) for d in dsss]
    if len(set(len(r) for r in rc)) != 1:
        raise ValueError(what + ": random keys of one threshold")
    return b"".join(b"".join(r) for r in rc)


def PartialSigBatch(dsss) -> list:
    """[d.PartialSig() for d in dsss] as ONE engine call (kyb_ed25519_dss_partial) for DSS objects of one signer over one
    roster and one long-term share.  The nonces are drawn here, one Scalar.Pick per session in list order from each
    object's stream: what the loop of PartialSig draws; the output is byte-identical to the loop's."""
    dsss = list(dsss)
    if not dsss:
        return []
    first = dsss[0]
    _, lc = _same_key(dsss, "PartialSigBatch")
    for d in dsss[1:]:
        if d.index != first.index or not d.secret.Equal(first.secret) or not d.long.PriShare().V.Equal(first.long.PriShare().V):
            raise ValueError("PartialSigBatch: one signer and one long-term share")
    ks = b"".join(ed._sc(d.suite.Scalar().Pick(d.rand)).v for d in dsss)
    beta = b"".join(ed._sc(d.random.PriShare().V).v for d in dsss)
    V, sid, sigs = ed.batch_dss_partial(ed._sc(first.secret).v, first.index, ed._sc(first.long.PriShare().V).v, beta, ks, b"".join(lc),
                                        _rand_commits(dsss, "PartialSigBatch"), [d.msg for d in dsss])
    out = []
    for b, d in enumerate(dsss):
        ps = PartialSig(share.PriShare(d.index, ed.Scalar(bytes(V[b]))), bytes(sid[b]), bytes(sigs[b]))
        d._own(ps)
        out.append(ps)
    return out


_SIG_STATUSES = (_lib.ST_DSS_SIG, 5, 6)  # ... KYB_ST_SIG_NONCANONICAL, KYB_ST_SIG_SMALL_ORDER: kyb_ed25519_verify's own
_MESSAGES = {
    _lib.ST_DSS_SESSION: "dss: session id do not match",
    _lib.ST_DSS_PARTIAL: "dss: partial signature not valid",
}


def process_partial_sigs(pairs) -> list:
    """[error or None of dss.ProcessPartialSig(ps) for (dss, ps) in pairs], in list order, for pairs over one roster and
    one long-term key: ONE kyb_ed25519_dss_check, then the sequential rules on the host.  A pair rejected for its
    signature is verified again on its own to get the reference's message; a SessionID whose length is not 32, or a
    signature whose length is not 64, goes the sequential way."""
    pairs = list(pairs)
    out = [None] * len(pairs)
    sessions, order = {}, []
    for d, _ in pairs:
        if id(d) not in sessions:
            sessions[id(d)] = len(order)
            order.append(d)
    batch = [j for j, (d, ps) in enumerate(pairs) if len(bytes(ps.SessionID)) == 32 and len(bytes(ps.Signature)) == 64 and 0 <= ps.Partial.I < 2**32]
    status = {}
    if batch:
        pk, lc = _same_key(order, "process_partial_sigs")
        ok, st, sst = ed.batch_dss_check(b"".join(pk), b"".join(lc), _rand_commits(order, "process_partial_sigs"), [d.msg for d in order],
                                         [sessions[id(pairs[j][0])] for j in batch], [pairs[j][1].Partial.I for j in batch],
                                         b"".join(ed._sc(pairs[j][1].Partial.V).v for j in batch),
                                         b"".join(bytes(pairs[j][1].SessionID) for j in batch),
                                         b"".join(bytes(pairs[j][1].Signature) for j in batch))
        status = {j: int(s) for j, s in zip(batch, st)}
    for j, (d, ps) in enumerate(pairs):
        try:
            st = status.get(j)
            if st is None or st == _lib.ST_BAD_POINT:  # (a key or a commitment that does not decode: the sequential way names it)
                d.ProcessPartialSig(ps)
                continue
            if st == _lib.ST_DSS_INDEX:
                raise ErrInvalidSignatureIndex
            if st in _SIG_STATUSES:  # the signature: verified again on its own for the reference's message
                schnorr.Verify(d.suite, d.participants[ps.Partial.I], ps.Hash(d.suite), ps.Signature)
                raise ValueError("schnorr: invalid signature")
            if st == _lib.ST_DSS_SESSION:
                raise ValueError(_MESSAGES[st])
            if ps.Partial.I in d.partialsIdx:  # dss.go:156-158, between the session id and the equation
                raise ValueError("dss: partial signature already received from peer")
            if st == _lib.ST_DSS_PARTIAL:
                raise ValueError(_MESSAGES[st])
            d._accept(ps)
        except ValueError as e:
            out[j] = e
    return out


def SignatureBatch(dsss) -> list:
    """[d.Signature() for d in dsss]: share.recover_secret on the host, B t^2 scalar operations"""
    return [d.Signature() for d in dsss]
