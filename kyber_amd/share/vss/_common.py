"""What share/vss/pedersen/vss.go and share/vss/rabin/vss.go have in common, written once: the suite, the messages, the
functions at the end of both files, the parts of the aggregator, the dealer and the verifier that read the same in both,
and the batch entries.  kyber_amd/share/vss/pedersen.py and rabin.py differ only where the Go files differ; each says
where.  A Go ``error`` is a raised ``ValueError`` with the reference's string.

The engine calls behind it:
  Dealer.EncryptedDeals()                  ONE kyb_ed25519_vss_seal for the n verifiers: the ephemeral scalar and the
                                           signature's nonce are drawn interleaved, dh_0, k_0, dh_1, k_1, ..., which is the
                                           order of the loop over EncryptedDeal(i) -- under one deterministic stream the
                                           batch equals the loop byte for byte
  process_encrypted_deals(verifiers, deals)   many Verifiers with one deal each (a node of share/dkg/rabin verifying n
                                           dealers): ONE kyb_ed25519_verify, ONE kyb_ed25519_vss_open, ONE batch_unmarshal
                                           of every commitment, ONE share check per threshold met (kyb_ed25519_deal_check in
                                           pedersen, kyb_ed25519_deal_check2 in rabin) and ONE SignBatch for the responses;
                                           the sequential rules run on the host in input order
  process_responses(aggregator, responses)    ONE kyb_ed25519_verify
"""
from __future__ import annotations

import hashlib
import os
import struct

from ... import _lib
from ...group import edwards25519 as ed
from ...sign import schnorr
from ...util import blake2xb
from .. import poly as share
from . import _wire


class Suite(ed.Curve):
    """edwards25519.NewBlakeSHA256Ed25519WithRand(rand) as far as vss.Suite asks (vss.go:22-27): Group, HashFactory,
    XOFFactory, Random.  rand: the stream every Scalar.Pick of the package draws from (None: the system's randomness)."""

    def __init__(self, rand=None):
        self._rand = rand if rand is not None else blake2xb.New(os.urandom(64))

    def Hash(self):
        return hashlib.sha256()

    def XOF(self, seed: bytes):
        return blake2xb.New(seed)

    def RandomStream(self):
        return self._rand


def NewSuite(rand=None) -> Suite:
    return Suite(rand)


class ErrDealAlreadyProcessed(ValueError):  # errDealAlreadyProcessed
    def __init__(self):
        super().__init__("vss: verifier already received a deal")


# ------------------------------------------------------------------------------------------------------------ messages
class Response:
    """Response (pedersen/vss.go:124-133, rabin/vss.go:164-173): the verdict is ``StatusApproved`` in pedersen and
    ``Approved`` in rabin; both names read and write the one field"""

    def __init__(self, SessionID, Index: int, StatusApproved: bool = False, Signature: bytes = b"", Approved=None):
        self.SessionID, self.Index, self.Signature = SessionID, Index, Signature
        self.StatusApproved = StatusApproved if Approved is None else Approved

    @property
    def Approved(self) -> bool:
        return self.StatusApproved

    @Approved.setter
    def Approved(self, v: bool) -> None:
        self.StatusApproved = v

    def Hash(self, s=None) -> bytes:
        return hashlib.sha256(b"response" + bytes(self.SessionID or b"") + struct.pack("<I", self.Index) +
                              (b"\x01" if self.StatusApproved else b"\x00")).digest()


class Justification:
    def __init__(self, SessionID, Index: int, Deal, Signature: bytes = b""):
        self.SessionID, self.Index, self.Deal, self.Signature = SessionID, Index, Deal, Signature

    def Hash(self, s=None) -> bytes:
        return hashlib.sha256(b"justification" + bytes(self.SessionID or b"") + struct.pack("<I", self.Index) + self.Deal.Marshal()).digest()


# ------------------------------------------------------------------------------------------- the functions at the end
def MinimumT(n: int) -> int:
    return (n >> 1) + 1


def validT(t: int, verifiers) -> bool:
    return 2 <= t <= len(verifiers)


def findPub(verifiers, idx: int):
    return (verifiers[idx], True) if 0 <= idx < len(verifiers) else (None, False)


def sessionID(suite, dealer, verifiers, commitments, t: int) -> bytes:
    h = suite.Hash()
    h.update(dealer.MarshalBinary())
    for p in list(verifiers) + list(commitments):
        h.update(p.MarshalBinary())
    h.update(struct.pack("<I", t))
    return h.digest()


def dhExchange(suite, ownPrivate, remotePublic):
    return suite.Point().Mul(ownPrivate, remotePublic)


def verify_error(sig: bytes, ok: bool):
    """what schnorr.Verify returns (schnorr.go:163-169) as far as the engine's verdict tells: the length check is the
    reference's first; every other failed check or a failed equation reads "invalid signature" here"""
    if len(sig) != 64:
        return ValueError("schnorr: signature of invalid length %d instead of %d" % (len(sig), 64))
    return None if ok else ValueError("schnorr: invalid signature")


def decode_shares(raw_share: bytes, suite):
    """internal.UnmarshalPriShare"""
    i, v = _wire.decode_pri_share(raw_share)
    if v is None:
        raise ValueError("vss: deal without a share")  # (the reference goes on with a nil scalar and panics)
    return share.PriShare(i, suite.Scalar().UnmarshalBinary(v))


# ----------------------------------------------------------------------------------------------------------- aggregator
class AggregatorBase:
    """the fields of both aggregators (pedersen/vss.go:560-572, rabin/vss.go:573-584; rabin's has no timeout) and the
    three methods that read the same in both files"""

    SID_MAY_BE_UNSET = True  # pedersen compares the session only once it has one (vss.go:666); rabin always (vss.go:668)

    def __init__(self, suite, dealer, verifiers, commitments, t: int, sid):
        self.suite, self.dealer, self.verifiers, self.commits = suite, dealer, list(verifiers), commitments
        self.responses, self.sid, self.deal, self.t = {}, sid, None, t
        self.badDealer = self.timeout = False

    def verifyResponse(self, r: Response, _sig_ok=None) -> None:
        if not (self.SID_MAY_BE_UNSET and self.sid is None) and bytes(r.SessionID or b"") != bytes(self.sid or b""):
            raise ValueError("vss: receiving inconsistent sessionID in response")
        pub, ok = findPub(self.verifiers, r.Index)
        if not ok:
            raise ValueError("vss: index out of bounds in response")
        if _sig_ok is None:
            _sig_ok = schnorr.batch_verify_with_checks([pub.MarshalBinary()], [r.Hash(self.suite)], [bytes(r.Signature)])[0]
        e = verify_error(bytes(r.Signature), bool(_sig_ok))
        if e is not None:
            raise e
        self.addResponse(r)

    def verifyJustification(self, j: Justification) -> None:
        if not findPub(self.verifiers, j.Index)[1]:
            raise ValueError("vss: index out of bounds in justification")
        r = self.responses.get(j.Index)
        if r is None:
            raise ValueError("vss: no complaints received for this justification")
        if r.StatusApproved:
            raise ValueError("vss: justification received for an approval")
        try:
            self.VerifyDeal(j.Deal, False)
        except ValueError:
            self.badDealer = True  # if one justification is bad, then flag the dealer as malicious
            raise
        r.StatusApproved = True

    def addResponse(self, r: Response) -> None:
        if not findPub(self.verifiers, r.Index)[1]:
            raise ValueError("vss: index out of bounds in Complaint")
        if r.Index in self.responses:
            raise ValueError("vss: already existing response from same origin")
        self.responses[r.Index] = r


# --------------------------------------------------------------------------------------------------------------- dealer
class DealerBase:
    """what both Dealers do alike once NewDealer has made the deals: self.suite, long, pub, verifiers, deals, sessionID,
    hkdfContext"""

    def PlaintextDeal(self, i: int):
        if i >= len(self.deals):
            raise ValueError("dealer: PlaintextDeal given wrong index")
        return self.deals[i]

    def _seal(self, rows) -> list:
        """EncryptedDeal for these verifiers as ONE engine call; draws dh, k per row in order"""
        rand = self.suite.RandomStream()
        dh, k = [], []
        for _ in rows:
            dh.append(self.suite.Scalar().Pick(rand).v)  # dhSecret
            k.append(self.suite.Scalar().Pick(rand).v)   # schnorr.Sign's nonce (schnorr.go:59)
        keys, sigs, ciphers, st = ed.batch_vss_seal(b"".join(dh), b"".join(k), self.long.v, self.pub.MarshalBinary(),
                                                    b"".join(self.verifiers[i].MarshalBinary() for i in rows), self.hkdfContext,
                                                    [self.deals[i].Marshal() for i in rows], ctx_len=len(self.hkdfContext))
        if st.any():
            raise ValueError("invalid Ed25519 curve point")
        return [self._encrypted_deal(bytes(a), bytes(b), c) for a, b, c in zip(keys, sigs, ciphers)]

    def EncryptedDeal(self, i: int):
        if not findPub(self.verifiers, i)[1]:
            raise ValueError("dealer: wrong index to generate encrypted deal")
        return self._seal([i])[0]

    def EncryptedDeals(self) -> list:
        return self._seal(range(len(self.verifiers))) if self.verifiers else []

    def ProcessResponse(self, r: Response):
        self.verifyResponse(r)
        if r.StatusApproved:
            return None
        j = Justification(self.sessionID, r.Index, self.deals[r.Index])
        j.Signature = schnorr.Sign(self.suite, self.long, j.Hash(self.suite), self.suite.RandomStream())
        return j

    def Key(self):
        return self.long, self.pub

    def SessionID(self) -> bytes:
        return self.sessionID


# ------------------------------------------------------------------------------------------------------------- verifier
class VerifierBase:
    def _new(self, suite, longterm, dealerKey, verifiers) -> None:
        """NewVerifier's search for the own key (pedersen/vss.go:362-377)"""
        pub = suite.Point().Mul(longterm, None)
        for i, v in enumerate(verifiers):
            if v.Equal(pub):
                index = i
                break
        else:
            raise ValueError("vss: public key not found in the list of verifiers")
        self.longterm, self.pub, self.index = longterm, pub, index

    def ProcessEncryptedDeal(self, e):
        out = process_encrypted_deals([self], [e])[0]
        if isinstance(out, Exception):
            raise out
        return out

    def decryptDeal(self, e):
        out = _decrypt_deals([self], [e])[0]
        if isinstance(out, Exception):
            raise out
        return out

    def ProcessJustification(self, dr: Justification) -> None:
        self.verifyJustification(dr)

    def Key(self):
        return self.longterm, self.pub

    def Index(self) -> int:
        return self.index

    def SessionID(self):
        return self.sid


def recover_secret(suite, deals, n: int, t: int):
    for d in deals:
        if bytes(d.SessionID) != bytes(deals[0].SessionID):
            raise ValueError("vss: all deals need to have same session id")
    return share.recover_secret(suite, [d.SecShare for d in deals], t, n)


# -------------------------------------------------------------------------------------------------------- batch entries
def _decrypt_deals(verifiers, deals) -> list:
    """decryptDeal (pedersen/vss.go:436-460, rabin/vss.go:479-503) for verifier i on deal i: a Deal, or the error the
    reference returns.  ONE verify of every signature over its DHKey, ONE vss_open, ONE batch_unmarshal of every
    commitment."""
    n = len(verifiers)
    out = [None] * n
    keys = [verifiers[i]._dhkey_bytes(deals[i]) for i in range(n)]
    sig_ok = schnorr.batch_verify_with_checks([v.dealer.MarshalBinary() for v in verifiers], keys, [e.Signature for e in deals])
    for i in range(n):
        out[i] = verify_error(deals[i].Signature, bool(sig_ok[i]))
    rows = [i for i in range(n) if out[i] is None]
    for i in list(rows):
        if len(keys[i]) != 32:  # dhKey.UnmarshalBinary (pedersen/vss.go:445)
            out[i] = ValueError("invalid Ed25519 curve point")
            rows.remove(i)
    if not rows:
        return out
    clen = len(verifiers[rows[0]].hkdfContext)
    ctxs = b"".join(verifiers[i].hkdfContext for i in rows)
    plain, st = ed.batch_vss_open(b"".join(verifiers[i].longterm.v for i in rows), b"".join(keys[i] for i in rows),
                                  ctxs if len(rows) > 1 else verifiers[rows[0]].hkdfContext, [deals[i].Cipher for i in rows],
                                  ctx_len=clen)
    # the engine names a cipher shorter than its tag before a key that does not decode; the reference meets the key first
    # (dhKey.UnmarshalBinary, vss.go:445, before Open, vss.go:453): ask about the keys of the short ones
    short = [j for j in range(len(rows)) if st[j] == _lib.ST_ECIES_SHORT]
    key_bad = dict(zip(short, ed.batch_unmarshal(b"".join(keys[rows[j]] for j in short))[1])) if short else {}
    raws = {}
    for j, i in enumerate(rows):
        if st[j] == _lib.ST_BAD_POINT or key_bad.get(j):
            out[i] = ValueError("invalid Ed25519 curve point")
        elif st[j]:  # a cipher shorter than its tag fails in Open too (crypto/cipher gcm.Open)
            out[i] = ValueError("cipher: message authentication failed")
        else:
            try:
                raws[i] = verifiers[i].DealType._decode(plain[j])
            except ValueError as err:
                out[i] = err
    for i in [i for i, raw in raws.items() if any(len(c) != 32 for c in raw[-1])]:
        out[i] = ValueError("invalid Ed25519 curve point")
        del raws[i]
    flat = b"".join(c for raw in raws.values() for c in raw[-1])
    pts, pst = ed.batch_unmarshal(flat) if flat else ((), ())
    pos = 0
    for i, raw in raws.items():
        cnt = len(raw[-1])
        try:
            out[i] = verifiers[i].DealType()._set(raw, pts[pos:pos + cnt], pst[pos:pos + cnt], verifiers[i].suite)
        except ValueError as err:
            out[i] = err
        pos += cnt
    return out


def process_encrypted_deals(verifiers, deals) -> list:
    """[verifiers[i].ProcessEncryptedDeal(deals[i])] for many Verifiers of ONE package with one deal each: the Response,
    or the error the reference returns, per element.  The engine work is batched (see the head of this file); every
    rule that reads or writes a verifier's state runs on the host, element by element in input order, so a Verifier that
    appears twice sees its second deal as the reference's loop would."""
    n = len(verifiers)
    out = _decrypt_deals(verifiers, deals)
    rows = [i for i in range(n) if not isinstance(out[i], Exception)]
    share_ok = dict(zip(rows, verifiers[rows[0]]._check_shares([verifiers[i] for i in rows], [out[i] for i in rows]))) if rows else {}
    pending = []  # (element, response) in input order: signed in one batch, then added
    for i in rows:
        try:
            pending.append((i, verifiers[i]._respond(out[i], share_ok[i])))
        except ValueError as err:
            out[i] = err
    if pending:
        sigs = schnorr.SignBatch(verifiers[0].suite, [verifiers[i].longterm for i, _ in pending], [r.Hash() for _, r in pending],
                                 rand=[verifiers[i].suite.RandomStream() for i, _ in pending])
        for (i, r), sig in zip(pending, sigs):
            r.Signature = sig
            try:
                verifiers[i].addResponse(r)
                out[i] = r
            except ValueError as err:
                out[i] = err
    return out


def process_responses(aggregator, responses) -> list:
    """[aggregator.ProcessResponse(r) for r in responses] with ONE kyb_ed25519_verify: None, or the error the reference
    returns, per response.  Works on an aggregator, a Dealer (its verifyResponse: no Justification is made here) and a
    Verifier that holds its deal."""
    early = aggregator._before_responses() if hasattr(aggregator, "_before_responses") else None
    if early is not None:
        return [early() for _ in responses]
    rows = [j for j, r in enumerate(responses) if findPub(aggregator.verifiers, r.Index)[1]]
    ok = {}
    if rows:
        got = schnorr.batch_verify_with_checks([aggregator.verifiers[responses[j].Index].MarshalBinary() for j in rows],
                                               [responses[j].Hash() for j in rows], [bytes(responses[j].Signature) for j in rows])
        ok = dict(zip(rows, got))
    out = []
    for j, r in enumerate(responses):
        try:
            aggregator.verifyResponse(r, _sig_ok=bool(ok.get(j, False)))
            out.append(None)
        except ValueError as err:
            out.append(err)
    return out
