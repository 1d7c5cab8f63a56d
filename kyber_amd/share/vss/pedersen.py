"""Host-side mirror of the reference's ``share/vss/pedersen`` (vss.go, dh.go) on Ed25519, function for function, with the
reference's error strings in the reference's order (a Go ``error`` is a raised ``ValueError``).  What the package shares
with ``share/vss/rabin`` is ``_common.py``'s -- the batch entries and the engine calls behind them are described there;
here is what pedersen/vss.go has of its own: the Deal with one share and its wire form, the SHA-256 context of 32 bytes,
the share check f_i B == sum C_k x^k, ``SetThreshold``, the timeout and the certification rule with absent responses.
``protocol``-level networking is not here.
"""
from __future__ import annotations

from ...group import edwards25519 as ed
from .. import poly as share
from . import _common, _wire
from ._common import (ErrDealAlreadyProcessed as _ErrDealAlreadyProcessed, Justification, MinimumT, NewSuite, Response, Suite,  # noqa: F401
                      dhExchange, findPub, process_encrypted_deals, process_responses, sessionID, validT)

StatusComplaint, StatusApproval = False, True  # vss.go:135-142


class ErrNoDealBeforeResponse(ValueError):  # vss.go:466
    def __init__(self):
        super().__init__("verifier: need to receive deal before response")


class Deal:  # vss.go:51-60
    def __init__(self, SessionID=b"", SecShare=None, T=0, Commitments=None):
        self.SessionID, self.SecShare, self.T, self.Commitments = SessionID, SecShare, T, Commitments or []

    def Marshal(self) -> bytes:  # vss.go:73-85
        sec = _wire.encode_pri_share(self.SecShare.I, self.SecShare.V.MarshalBinary())
        return _wire.encode_deal(self.SessionID, sec, self.T, [c.MarshalBinary() for c in self.Commitments])

    _decode = staticmethod(_wire.decode_deal)

    def Unmarshal(self, data: bytes, suite) -> "Deal":  # vss.go:89-107
        raw = _wire.decode_deal(bytes(data))
        out, st = ed.batch_unmarshal(b"".join(raw[3])) if raw[3] else ((), ())
        return self._set(raw, out, st, suite)

    def _set(self, raw, points, status, suite) -> "Deal":
        """the decoded fields and the engine's decoding of the commitments (canonical bytes, status)"""
        sid, sec, t, commits = raw
        if any(len(c) != 32 for c in commits) or any(status):
            raise ValueError("invalid Ed25519 curve point")
        self.SecShare = _common.decode_shares(sec, suite)
        self.SessionID, self.T = sid, t
        self.Commitments = [ed.Point(bytes(p)) for p in points]
        return self


class EncryptedDeal:  # vss.go:113-120: DHKey is the key's bytes
    def __init__(self, DHKey: bytes, Signature: bytes, Cipher: bytes):
        self.DHKey, self.Signature, self.Cipher = bytes(DHKey), bytes(Signature), bytes(Cipher)


def context(suite, dealer, verifiers) -> bytes:  # dh.go:43-51
    h = suite.Hash()
    h.update(b"vss-dealer" + dealer.MarshalBinary() + b"vss-verifiers")
    for v in verifiers:
        h.update(v.MarshalBinary())
    return h.digest()


def _check_shares(deals) -> list:
    """fig.Equal(commitPoly.Eval(fi.I).V) (vss.go:637-645) for every deal: ONE kyb_ed25519_deal_check per number of
    commitments met -- one, where every dealer uses the same threshold"""
    ok = [False] * len(deals)
    by_t = {}
    for j, d in enumerate(deals):
        by_t.setdefault(len(d.Commitments), []).append(j)
    for t, rows in by_t.items():
        commits = b"".join(c.MarshalBinary() for j in rows for c in deals[j].Commitments)
        got, _ = ed.batch_deal_check(list(range(len(rows))), [deals[j].SecShare.I for j in rows],
                                     b"".join(deals[j].SecShare.V.v for j in rows), commits or bytes(32), len(rows), t)
        for j, g in zip(rows, got):
            ok[j] = bool(g)
    return ok


class Aggregator(_common.AggregatorBase):  # vss.go:560-572
    def VerifyDeal(self, d: Deal, inclusion: bool, _share_ok=None) -> None:  # vss.go:610-647
        """_share_ok: the verdict of the share check where a batch has it already (process_encrypted_deals)"""
        if self.deal is not None and inclusion:
            raise _ErrDealAlreadyProcessed()
        if self.deal is None:
            self.commits, self.sid, self.deal, self.t = d.Commitments, d.SessionID, d, d.T
        if not validT(d.T, self.verifiers):
            raise ValueError("vss: invalid t received in Deal")
        if d.T != self.t:
            raise ValueError("vss: incompatible threshold - potential attack")
        if bytes(self.sid) != bytes(d.SessionID):
            raise ValueError("vss: find different sessionIDs from Deal")
        fi = d.SecShare
        if fi.I >= len(self.verifiers):
            raise ValueError("vss: index out of bounds in Deal")
        if _share_ok is None:
            _share_ok = _check_shares([d])[0]
        if not _share_ok:
            raise ValueError("vss: share does not verify against commitments in Deal")

    def SetThreshold(self, t: int) -> None:  # vss.go:654-656
        self.t = t

    def ProcessResponse(self, r: Response) -> None:  # vss.go:661-663
        self.verifyResponse(r)

    def Responses(self) -> dict:  # vss.go:716-718
        return self.responses

    def DealCertified(self) -> bool:  # vss.go:733-755
        absent = approvals = 0
        complaint = False
        for i in range(len(self.verifiers)):
            r = self.responses.get(i)
            if r is None:
                absent += 1
            elif r.StatusApproved:
                approvals += 1
            else:
                complaint = True
        base = (not self.badDealer) and approvals >= self.t and not complaint
        if self.timeout:
            # (uint32 arithmetic: n - t wraps where t > n, and nothing is then too much)
            return base and not absent > (len(self.verifiers) - self.t) % 2**32
        return base and absent <= 0

    def MissingResponses(self) -> list:  # vss.go:758-766
        return [i for i in range(len(self.verifiers)) if i not in self.responses]


def NewEmptyAggregator(suite, verifiers) -> Aggregator:  # vss.go:596-602
    return Aggregator(suite, None, verifiers, None, 0, None)


class Dealer(_common.DealerBase, Aggregator):  # vss.go:31-48
    _encrypted_deal = staticmethod(EncryptedDeal)

    def __init__(self, suite, longterm, secret, verifiers, t: int):
        """NewDealer (vss.go:164-204)"""
        verifiers = list(verifiers)
        if not validT(t, verifiers):
            raise ValueError("dealer: t %d invalid" % t)
        self.long, self.secret = longterm, secret
        # share.NewPriPoly(suite, t, secret, RandomStream): the secret stands, then t - 1 coefficients are drawn
        rand = suite.RandomStream()
        f = share.PriPoly(suite, [secret] + [suite.Scalar().Pick(rand) for _ in range(t - 1)])
        self.pub = suite.Point().Mul(longterm, None)
        self.secretCommits = f.Commit(suite.Point().Base()).Info()[1]
        self.sessionID = sessionID(suite, self.pub, verifiers, self.secretCommits, t)
        Aggregator.__init__(self, suite, self.pub, verifiers, self.secretCommits, t, self.sessionID)
        self.deals = [Deal(self.sessionID, fi, t, self.secretCommits) for fi in f.Shares(len(verifiers))]
        self.hkdfContext = context(suite, self.pub, verifiers)
        self.secretPoly = f

    ProcessResponse = _common.DealerBase.ProcessResponse  # vss.go:276-297 (the Dealer's own, not the aggregator's)

    def SecretCommit(self):  # vss.go:302-307
        return self.suite.Point().Mul(self.secret, None) if self.DealCertified() else None

    def Commits(self) -> list:  # vss.go:311-313
        return self.secretCommits

    def SetTimeout(self) -> None:  # vss.go:329-331
        self.timeout = True

    def PrivatePoly(self):  # vss.go:337-339
        return self.secretPoly


def NewDealer(suite, longterm, secret, verifiers, t: int) -> Dealer:
    return Dealer(suite, longterm, secret, verifiers, t)


class Verifier(_common.VerifierBase, Aggregator):  # vss.go:343-352
    DealType = Deal

    def __init__(self, suite, longterm, dealerKey, verifiers):
        """NewVerifier (vss.go:362-389)"""
        verifiers = list(verifiers)
        self._new(suite, longterm, dealerKey, verifiers)
        Aggregator.__init__(self, suite, None, verifiers, None, 0, None)  # NewEmptyAggregator
        self.dealer = dealerKey  # (Verifier.dealer: the embedded aggregator's stays nil in the reference and is not read)
        self.hkdfContext = context(suite, dealerKey, verifiers)

    @staticmethod
    def _dhkey_bytes(e) -> bytes:
        return bytes(e.DHKey)

    @staticmethod
    def _check_shares(verifiers, deals) -> list:
        return _check_shares(deals)

    def _respond(self, d: Deal, share_ok: bool) -> Response:
        """ProcessEncryptedDeal between decryptDeal and the signature (vss.go:405-424)"""
        if d.SecShare.I != self.index:
            raise ValueError("vss: verifier got wrong index from deal")
        r = Response(sessionID(self.suite, self.dealer, self.verifiers, d.Commitments, d.T), self.index, StatusApproval)
        try:
            self.VerifyDeal(d, True, _share_ok=share_ok)
        except _ErrDealAlreadyProcessed:
            raise
        except ValueError:
            r.StatusApproved = StatusComplaint
        return r

    def _before_responses(self):
        return ErrNoDealBeforeResponse if self.deal is None else None

    def ProcessResponse(self, resp: Response) -> None:  # vss.go:472-477
        if self.deal is None:
            raise ErrNoDealBeforeResponse()
        self.verifyResponse(resp)

    def Commits(self) -> list:  # vss.go:482-484
        return self.deal.Commitments

    def Deal(self):  # vss.go:488-493
        return self.deal if self.DealCertified() else None

    def SetTimeout(self) -> None:  # vss.go:541-543
        self.timeout = True

    def UnsafeSetResponseDKG(self, idx: int, approval: bool) -> None:  # vss.go:547-556
        try:
            self.addResponse(Response(self.sid, idx, approval))
        except ValueError:
            pass  # (the reference drops the error)


def NewVerifier(suite, longterm, dealerKey, verifiers) -> Verifier:
    return Verifier(suite, longterm, dealerKey, verifiers)


def RecoverSecret(suite, deals, n: int, t: int):  # vss.go:524-535
    return _common.recover_secret(suite, deals, n, t)
