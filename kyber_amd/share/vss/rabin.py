"""Host-side mirror of the reference's ``share/vss/rabin`` (vss.go, dh.go) on Ed25519, function for function, with the
reference's error strings in the reference's order (a Go ``error`` is a raised ``ValueError``).  What the package shares
with ``share/vss/pedersen`` is ``_common.py``'s -- the batch entries and the engine calls behind them are described
there; here is what rabin/vss.go has of its own: the second polynomial g and its share (``RndShare``) with the Deal's
own wire form, ``H = deriveH(verifiers)`` and the commitments C = F + G with G = g.Commit(H) (ONE same-base call and ONE
batched Add), the context of 128 bytes read from the suite's XOF, ``DHKey`` as a point, the share check
f_i B + g_i H == sum C_k x^k (kyb_ed25519_deal_check2), the aggregator a Verifier only has once it has a deal,
``EnoughApprovals``, ``cleanVerifiers`` behind ``SetTimeout`` and the certification rule built on them.
``protocol``-level networking is not here.
"""
from __future__ import annotations

from ...group import edwards25519 as ed
from .. import poly as share
from . import _common, _wire
from ._common import (ErrDealAlreadyProcessed as _ErrDealAlreadyProcessed, Justification, MinimumT, NewSuite, Response, Suite,  # noqa: F401
                      dhExchange, findPub, process_encrypted_deals, process_responses, sessionID, validT)

keySize = 128  # dh.go:43: arbitrary, long enough to seed the XOF


class Deal:  # vss.go:76-89
    def __init__(self, SessionID=b"", SecShare=None, RndShare=None, T=0, Commitments=None):
        self.SessionID, self.SecShare, self.RndShare, self.T, self.Commitments = SessionID, SecShare, RndShare, T, Commitments or []

    def Marshal(self) -> bytes:  # vss.go:102-119
        sec = _wire.encode_pri_share(self.SecShare.I, self.SecShare.V.MarshalBinary())
        rnd = _wire.encode_pri_share(self.RndShare.I, self.RndShare.V.MarshalBinary())
        return _wire.encode_deal_rabin(self.SessionID, sec, rnd, self.T, [c.MarshalBinary() for c in self.Commitments])

    _decode = staticmethod(_wire.decode_deal_rabin)

    def Unmarshal(self, data: bytes, suite) -> "Deal":  # vss.go:123-147
        raw = _wire.decode_deal_rabin(bytes(data))
        out, st = ed.batch_unmarshal(b"".join(raw[4])) if raw[4] else ((), ())
        return self._set(raw, out, st, suite)

    def _set(self, raw, points, status, suite) -> "Deal":
        sid, sec, rnd, t, commits = raw
        if any(len(c) != 32 for c in commits) or any(status):
            raise ValueError("invalid Ed25519 curve point")
        self.SecShare = _common.decode_shares(sec, suite)
        self.RndShare = _common.decode_shares(rnd, suite)
        self.SessionID, self.T = sid, t
        self.Commitments = [ed.Point(bytes(p)) for p in points]
        return self


class EncryptedDeal:  # vss.go:153-160: DHKey is a kyber.Point
    def __init__(self, DHKey, Signature: bytes, Cipher: bytes):
        self.DHKey = DHKey if isinstance(DHKey, ed.Point) else ed.Point(bytes(DHKey))
        self.Signature, self.Cipher = bytes(Signature), bytes(Cipher)


def context(suite, dealer, verifiers) -> bytes:  # dh.go:46-67
    h = suite.XOF(b"vss-dealer")
    h.Write(dealer.MarshalBinary())
    h.Write(b"vss-verifiers")
    for v in verifiers:
        h.Write(v.MarshalBinary())
    return h.Read(keySize)


def deriveH(suite, verifiers):  # vss.go:775-782: Point.Pick is Embed(nil, rand) (point.go:180-182)
    return suite.Point().Embed(None, suite.XOF(b"".join(v.MarshalBinary() for v in verifiers)))


def _check_shares(verifier_sets, deals) -> list:
    """ci.Equal(commitPoly.Eval(fi.I).V) with ci = fi B + gi H (vss.go:638-649) for every deal: ONE
    kyb_ed25519_deal_check2 per number of commitments met, H per deal (every verifier set derives its own)"""
    ok = [False] * len(deals)
    by_t, hs = {}, {}
    for j, d in enumerate(deals):
        by_t.setdefault(len(d.Commitments), []).append(j)
    for t, rows in by_t.items():
        H = []
        for j in rows:
            key = b"".join(v.MarshalBinary() for v in verifier_sets[j])
            if key not in hs:
                hs[key] = deriveH(NewSuite(), verifier_sets[j]).MarshalBinary()
            H.append(hs[key])
        commits = b"".join(c.MarshalBinary() for j in rows for c in deals[j].Commitments)
        one_h = len(set(H)) == 1
        got, _ = ed.batch_deal_check2(list(range(len(rows))), [deals[j].SecShare.I for j in rows],
                                      b"".join(deals[j].SecShare.V.v for j in rows), b"".join(deals[j].RndShare.V.v for j in rows),
                                      commits or bytes(32), H[0] if one_h else b"".join(H), len(rows), t)
        for j, g in zip(rows, got):
            ok[j] = bool(g)
    return ok


class aggregator(_common.AggregatorBase):  # vss.go:573-584
    SID_MAY_BE_UNSET = False  # vss.go:668

    def VerifyDeal(self, d: Deal, inclusion: bool, _share_ok=None) -> None:  # vss.go:611-651
        if self.deal is not None and inclusion:
            raise _ErrDealAlreadyProcessed()
        if self.deal is None:
            self.commits, self.sid, self.deal = d.Commitments, d.SessionID, d
        if not validT(d.T, self.verifiers):
            raise ValueError("vss: invalid t received in Deal")
        if bytes(self.sid) != bytes(d.SessionID):
            raise ValueError("vss: find different sessionIDs from Deal")
        fi, gi = d.SecShare, d.RndShare
        if fi.I != gi.I:
            raise ValueError("vss: not the same index for f and g share in Deal")
        if fi.I >= len(self.verifiers):
            raise ValueError("vss: index out of bounds in Deal")
        if _share_ok is None:
            _share_ok = _check_shares([self.verifiers], [d])[0]
        if not _share_ok:
            raise ValueError("vss: share does not verify against commitments in Deal")

    def cleanVerifiers(self) -> None:  # vss.go:655-665
        for i in range(len(self.verifiers)):
            if i not in self.responses:
                self.responses[i] = Response(self.sid, i, Approved=False)

    def EnoughApprovals(self) -> bool:  # vss.go:718-726
        return sum(1 for r in self.responses.values() if r.Approved) >= self.t

    def DealCertified(self) -> bool:  # vss.go:730-747
        unstable = sum(1 for i in range(len(self.verifiers)) if i not in self.responses)
        return self.EnoughApprovals() and not (unstable > 0 or self.badDealer)

    def UnsafeSetResponseDKG(self, idx: int, approval: bool) -> None:  # vss.go:751-760
        try:
            self.addResponse(Response(self.sid, idx, Approved=approval))
        except ValueError:
            pass  # (the reference drops the error)


class Dealer(_common.DealerBase, aggregator):  # vss.go:60-74
    _encrypted_deal = staticmethod(EncryptedDeal)

    def __init__(self, suite, longterm, secret, verifiers, t: int):
        """NewDealer (vss.go:193-245)"""
        verifiers = list(verifiers)
        if not validT(t, verifiers):
            raise ValueError("dealer: t %d invalid" % t)
        self.long, self.secret = longterm, secret
        H = deriveH(suite, verifiers)
        rand = suite.RandomStream()
        f = share.PriPoly(suite, [secret] + [suite.Scalar().Pick(rand) for _ in range(t - 1)])  # NewPriPoly(.., secret, ..)
        g = share.PriPoly(suite, [suite.Scalar().Pick(rand) for _ in range(t)])  # NewPriPoly(.., nil, ..)
        self.pub = suite.Point().Mul(longterm, None)
        F = f.Commit(suite.Point().Base())
        self.secretCommits = F.Info()[1]
        G = g.Commit(H)  # ONE same-base call
        commitments = F.Add(G).Info()[1]  # C = F + G: ONE batched Add
        self.sessionID = sessionID(suite, self.pub, verifiers, commitments, t)
        aggregator.__init__(self, suite, self.pub, verifiers, commitments, t, self.sessionID)
        fs, gs = f.Shares(len(verifiers)), g.Shares(len(verifiers))
        self.deals = [Deal(self.sessionID, fi, gi, t, commitments) for fi, gi in zip(fs, gs)]
        self.hkdfContext = context(suite, self.pub, verifiers)

    ProcessResponse = _common.DealerBase.ProcessResponse  # vss.go:316-337

    def SecretCommit(self):  # vss.go:341-346
        return self.suite.Point().Mul(self.secret, None) if self.EnoughApprovals() and self.DealCertified() else None

    def Commits(self):  # vss.go:350-355
        return self.secretCommits if self.EnoughApprovals() and self.DealCertified() else None

    def SetTimeout(self) -> None:  # vss.go:371-373
        self.cleanVerifiers()


def NewDealer(suite, longterm, secret, verifiers, t: int) -> Dealer:
    return Dealer(suite, longterm, secret, verifiers, t)


class Verifier(_common.VerifierBase, aggregator):  # vss.go:377-386
    """the embedded aggregator is nil until the first deal (vss.go:452-454): ``has_aggregator`` says which; without one
    DealCertified is false (vss.go:732-734) and the calls that dereference it in Go -- where they panic -- raise"""

    DealType = Deal

    def __init__(self, suite, longterm, dealerKey, verifiers):
        """NewVerifier (vss.go:393-426)"""
        verifiers = list(verifiers)
        self._new(suite, longterm, dealerKey, verifiers)
        aggregator.__init__(self, suite, dealerKey, verifiers, None, 0, None)
        self.has_aggregator = False
        self.hkdfContext = context(suite, dealerKey, verifiers)

    @staticmethod
    def _dhkey_bytes(e) -> bytes:
        return e.DHKey.MarshalBinary()  # vss.go:480

    @staticmethod
    def _check_shares(verifiers, deals) -> list:
        return _check_shares([v.verifiers for v in verifiers], deals)

    def _respond(self, d: Deal, share_ok: bool) -> Response:
        """ProcessEncryptedDeal between decryptDeal and the signature (vss.go:441-468)"""
        if d.SecShare.I != self.index:
            raise ValueError("vss: verifier got wrong index from deal")
        sid = sessionID(self.suite, self.dealer, self.verifiers, d.Commitments, d.T)
        if not self.has_aggregator:  # newAggregator(suite, dealer, verifiers, d.Commitments, d.T, d.SessionID)
            self.commits, self.t, self.sid, self.has_aggregator = d.Commitments, d.T, d.SessionID, True
        r = Response(sid, self.index, Approved=True)
        try:
            self.VerifyDeal(d, True, _share_ok=share_ok)
        except _ErrDealAlreadyProcessed:
            raise
        except ValueError:
            r.Approved = False
        return r

    def _need(self) -> None:
        if not self.has_aggregator:
            raise ValueError("vss: verifier has no aggregator before its first deal")  # (a nil dereference in the reference)

    def ProcessResponse(self, resp: Response) -> None:  # vss.go:509-511
        self._need()
        self.verifyResponse(resp)

    def _before_responses(self):
        return None if self.has_aggregator else (lambda: ValueError("vss: verifier has no aggregator before its first deal"))

    def EnoughApprovals(self) -> bool:
        self._need()
        return aggregator.EnoughApprovals(self)

    def DealCertified(self) -> bool:  # vss.go:732-734: false on a nil aggregator
        return self.has_aggregator and aggregator.DealCertified(self)

    def Deal(self):  # vss.go:515-520
        return self.deal if self.EnoughApprovals() and self.DealCertified() else None

    def SetTimeout(self) -> None:  # vss.go:567-569
        self._need()
        self.cleanVerifiers()


def NewVerifier(suite, longterm, dealerKey, verifiers) -> Verifier:
    return Verifier(suite, longterm, dealerKey, verifiers)


def RecoverSecret(suite, deals, n: int, t: int):  # vss.go:550-561
    return _common.recover_secret(suite, deals, n, t)
