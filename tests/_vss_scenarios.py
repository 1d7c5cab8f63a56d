"""The scenarios of the reference's share/vss/pedersen/vss_test.go and share/vss/rabin/vss_test.go (TestVSSWhole ...
TestVSSContext in both), restated once and run over two implementations through a small kit: kyber_amd.share.vss.pedersen
or .rabin (the product, over the engine or over the host harness) and the sequential oracle tests/_vss_oracle.py.  Where
the two Go test files read the same the scenario is written once and branches on ``K.rabin`` where they differ.  A scenario asserts what the Go test asserts and returns
a transcript -- every byte string the protocol produced, every verdict, every error string in order -- and the tests hold
the two transcripts equal.  As in the Go file ONE random stream serves the keys, the dealer and every verifier; where the
Go tests call crypto/rand (randomBytes, a random index) a second seeded stream stands in, the same for both kits.
nbVerifiers is the Go file's 7 unless a test says otherwise."""
import hashlib

from kyber_amd.util import blake2xb


class Kit:
    """what a scenario needs of an implementation; scalars, points and streams stay the implementation's own types"""

    name = ""

    def stream(self, seed: bytes): ...
    def pick(self, S): ...
    def base_mul(self, x): ...
    def enc(self, v) -> bytes: ...
    def NewDealer(self, S, long, secret, pubs, t): ...
    def NewVerifier(self, S, long, dealer_pub, pubs): ...
    def Response(self, **kw): ...
    def sign(self, S, priv, msg): ...
    def verify(self, pub, msg, sig): ...
    def RecoverSecret(self, S, deals, n, t): ...
    def add(self, a, b): ...
    def null(self): ...
    def aggregator(self, x): return x
    def process_deals(self, verifiers, deals): ...
    def process_responses(self, agg, responses): ...


class ProductKit(Kit):
    name = "product"

    def __init__(self, flavour="pedersen"):
        from kyber_amd.share.vss import pedersen, rabin
        from kyber_amd.sign import schnorr

        self.rabin = flavour == "rabin"
        self.m, self.schnorr = (rabin if self.rabin else pedersen), schnorr
        self.MinimumT, self.findPub = self.m.MinimumT, self.m.findPub

    def dhkey(self, pt):  # EncryptedDeal.DHKey: the key's bytes in pedersen, a point in rabin
        return pt if self.rabin else pt.MarshalBinary()

    def stream(self, seed):
        return self.m.NewSuite(blake2xb.New(seed))

    def pick(self, S):
        return S.Scalar().Pick(S.RandomStream())

    def base_mul(self, x):
        return self.m.ed.Point().Mul(x, None)

    def enc(self, v):
        return b"nil" if v is None else v.MarshalBinary()

    def NewDealer(self, S, long, secret, pubs, t):
        return self.m.NewDealer(S, long, secret, pubs, t)

    def NewVerifier(self, S, long, dealer_pub, pubs):
        return self.m.NewVerifier(S, long, dealer_pub, pubs)

    def Response(self, **kw):
        kw.setdefault("SessionID", b"")
        kw.setdefault("Index", 0)
        return self.m.Response(**kw)

    def sign(self, S, priv, msg):
        return self.schnorr.Sign(S, priv, msg, S.RandomStream())

    def verify(self, pub, msg, sig):
        self.schnorr.Verify(None, pub, msg, sig)

    def RecoverSecret(self, S, deals, n, t):
        return self.m.RecoverSecret(S, deals, n, t)

    def add(self, a, b):
        return self.m.ed.Point().Add(a, b)

    def null(self):
        return self.m.ed.Point().Null()

    def sessionID(self, S, dealer, pubs, commits, t):
        return self.m.sessionID(S, dealer, pubs, commits, t)

    def context(self, S, dealer, pubs):
        return self.m.context(S, dealer, pubs)

    def dhExchange(self, S, priv, pub):
        return self.m.dhExchange(S, priv, pub)

    def process_deals(self, verifiers, deals):
        return self.m.process_encrypted_deals(verifiers, deals)

    def process_responses(self, agg, responses):
        return self.m.process_responses(agg, responses)


class OracleKit(Kit):
    name = "oracle"

    def __init__(self, flavour="pedersen"):
        from tests import _vss_oracle as VO

        self.rabin = flavour == "rabin"
        self.m = VO
        self.MinimumT, self.findPub = VO.MinimumT, VO.findPub

    def dhkey(self, pt):
        return pt

    def stream(self, seed):
        return blake2xb.New(seed).Read

    def pick(self, S):
        return self.m.pick(S)

    def base_mul(self, x):
        return self.m.DO.base_mul(x)

    def enc(self, v):
        return b"nil" if v is None else (v if isinstance(v, bytes) else self.m.sc(v))

    def NewDealer(self, S, long, secret, pubs, t):
        return (self.m.RabinDealer if self.rabin else self.m.Dealer)(S, long, secret, list(pubs), t)

    def NewVerifier(self, S, long, dealer_pub, pubs):
        return (self.m.RabinVerifier if self.rabin else self.m.Verifier)(S, long, dealer_pub, list(pubs))

    def Response(self, **kw):
        if "Approved" in kw:  # rabin's name of the field
            kw["StatusApproved"] = kw.pop("Approved")
        return self.m.Response(**kw)

    def sign(self, S, priv, msg):
        return self.m.DO.Scheme(S).Sign(priv, msg)

    def verify(self, pub, msg, sig):
        self.m.DO.Scheme(None).Verify(pub, msg, sig)

    def RecoverSecret(self, S, deals, n, t):
        return self.m.RecoverSecret(deals, n, t)

    def add(self, a, b):
        from oracle import ed25519 as O

        return O.encode(O.add(O.decode(a), O.decode(b)))

    def null(self):
        from oracle import ed25519 as O

        return O.encode(O.IDENTITY)

    def sessionID(self, S, dealer, pubs, commits, t):
        return self.m.sessionID(dealer, list(pubs), list(commits), t)

    def context(self, S, dealer, pubs):
        return (self.m.rabin_context if self.rabin else self.m.context)(dealer, list(pubs))

    def dhExchange(self, S, priv, pub):
        return self.m.dhExchange(priv, pub)

    def process_deals(self, verifiers, deals):  # the loop the batch entry stands for
        out = []
        for v, e in zip(verifiers, deals):
            try:
                out.append(v.ProcessEncryptedDeal(e))
            except ValueError as err:
                out.append(err)
        return out

    def process_responses(self, agg, responses):
        out = []
        for r in responses:
            try:
                out.append(agg.ProcessResponse(r) and None)
            except ValueError as err:
                out.append(err)
        return out


def random_bytes(tag: bytes, n: int) -> bytes:
    """crypto/rand's stand-in: the same bytes for both kits"""
    return hashlib.shake_256(b"vss scenario " + tag).digest(n)


class World:
    """vss_test.go's package variables and init(): verifiers' keys, the dealer's, the secret, all from ONE stream"""

    def __init__(self, K, seed: bytes = b"vss_test.go", n: int = 7, t=None):
        self.K, self.n = K, n
        self.S = K.stream(seed)
        self.verifiersSec = [K.pick(self.S) for _ in range(n)]  # genCommits: a pair after a pair
        self.verifiersPub = [K.base_mul(x) for x in self.verifiersSec]
        self.dealerSec = K.pick(self.S)
        self.dealerPub = K.base_mul(self.dealerSec)
        self.secret = K.pick(self.S)
        self.t = K.MinimumT(n) if t is None else t

    def genDealer(self):
        return self.K.NewDealer(self.S, self.dealerSec, self.secret, self.verifiersPub, self.t)

    def genAll(self):
        return self.genDealer(), [self.K.NewVerifier(self.S, x, self.dealerPub, self.verifiersPub) for x in self.verifiersSec]


def err(f, *a):
    """the error string a call ends with, or None"""
    try:
        f(*a)
    except ValueError as e:
        return str(e)
    return None


def t_resp(K, r):
    return ("resp", r.SessionID, r.Index, r.StatusApproved, r.Signature)


def t_enc(e):
    key = e.DHKey.MarshalBinary() if hasattr(e.DHKey, "MarshalBinary") else bytes(e.DHKey)
    return ("enc", key, bytes(e.Signature), bytes(e.Cipher))


def t_result(K, x):
    """an element of a batch entry's result: a Response, None or an error"""
    return str(x) if isinstance(x, Exception) else (None if x is None else t_resp(K, x))


# ---------------------------------------------------------------------------------------------------------- scenarios
def whole(K, n=7, batched=False):  # TestVSSWhole; batched: through the batch entries
    w = World(K, n=n)
    dealer, verifiers = w.genAll()
    T = [K.enc(c) for c in dealer.secretCommits] + [dealer.sessionID, dealer.hkdfContext]
    encDeals = dealer.EncryptedDeals()
    T += [t_enc(e) for e in encDeals]
    if not K.rabin:  # (pedersen/vss_test.go:73; rabin's verifier has no aggregator yet and the Go test does not ask)
        for v in verifiers:
            assert err(v.ProcessResponse, None) == "verifier: need to receive deal before response"
    if batched:
        resps = K.process_deals(verifiers, encDeals)
        assert not any(isinstance(r, Exception) for r in resps), resps
    else:
        resps = [v.ProcessEncryptedDeal(e) for v, e in zip(verifiers, encDeals)]
    T += [t_resp(K, r) for r in resps]
    if batched:
        for i, v in enumerate(verifiers):
            assert K.process_responses(v, [r for r in resps if r.Index != i]) == [None] * (n - 1)
        assert K.process_responses(dealer, resps) == [None] * n
    else:
        for r in resps:
            for i, v in enumerate(verifiers):
                if r.Index != i:
                    assert v.ProcessResponse(r) is None
            assert dealer.ProcessResponse(r) is None
    assert all(v.DealCertified() for v in verifiers) and dealer.DealCertified()
    deals = [v.Deal() for v in verifiers]
    T += [d.Marshal() for d in deals]
    sec = K.RecoverSecret(w.S, deals, n, K.MinimumT(n))
    assert K.enc(sec) == K.enc(dealer.secret) == K.enc(w.secret)
    T += [K.enc(sec), K.enc(dealer.SecretCommit())]
    return T


def loop_equals_batch(K, n=7):
    """Dealer.EncryptedDeals() against the loop over EncryptedDeal(i) under the same stream"""
    a, b = World(K, n=n).genDealer(), World(K, n=n).genDealer()
    batch, loop = a.EncryptedDeals(), [b.EncryptedDeal(i) for i in range(n)]
    assert [t_enc(e) for e in batch] == [t_enc(e) for e in loop]
    assert err(a.EncryptedDeal, n) == "dealer: wrong index to generate encrypted deal"
    return [t_enc(e) for e in batch]


def dealer_new(K):  # TestVSSDealerNew
    w = World(K)
    T = [err(K.NewDealer, w.S, w.dealerSec, w.secret, w.verifiersPub, bad) for bad in (0, 1, 8)]
    assert T == ["dealer: t 0 invalid", "dealer: t 1 invalid", "dealer: t 8 invalid"]
    d = w.genDealer()
    assert err(d.PlaintextDeal, 7) == "dealer: PlaintextDeal given wrong index" and d.PlaintextDeal(6) is d.deals[6]
    return T + [d.deals[6].Marshal()]


def verifier_new(K):  # TestVSSVerifierNew
    w = World(K)
    idx = random_bytes(b"index", 1)[0] % 7
    v = K.NewVerifier(w.S, w.verifiersSec[idx], w.dealerPub, w.verifiersPub)
    assert v.index == idx
    e = err(K.NewVerifier, w.S, K.pick(w.S), w.dealerPub, w.verifiersPub)
    assert e == "vss: public key not found in the list of verifiers"
    return [idx, e]


def share(K):  # TestVSSShare
    w = World(K)
    dealer, verifiers = w.genAll()
    ver = verifiers[0]
    resp = ver.ProcessEncryptedDeal(dealer.EncryptedDeal(0))
    assert resp.StatusApproved is True
    for i in range(1, ver.t - 1):
        ver.responses[i] = K.Response(StatusApproved=True)
    assert ver.Deal() is None  # not enough approvals
    ver.responses[ver.t] = K.Response(StatusApproved=True)
    ver.SetTimeout()
    ver.badDealer = True
    assert ver.Deal() is None
    ver.badDealer = False
    assert ver.Deal() is not None
    return [t_resp(K, resp), ver.Deal().Marshal()]


def dealer_certified(K):  # TestVSSAggregatorDealCertified, ...AllResponses, TestVSSDealerTimeout
    w = World(K)
    dealer = w.genDealer()
    for i in range(dealer.t):
        dealer.responses[i] = K.Response(StatusApproved=True)
    assert not dealer.DealCertified() and dealer.MissingResponses() == list(range(dealer.t, 7))
    dealer.SetTimeout()
    assert dealer.DealCertified() and K.enc(dealer.SecretCommit()) == K.enc(K.base_mul(w.secret))
    dealer.badDealer = True
    assert not dealer.DealCertified() and dealer.SecretCommit() is None
    dealer.badDealer = False
    for i in range(dealer.t):
        dealer.responses[i] = K.Response(StatusApproved=False)
    assert not dealer.DealCertified()
    d2 = w.genDealer()
    for i in range(7):
        assert not d2.DealCertified()
        d2.responses[i] = K.Response(StatusApproved=True)
    assert d2.DealCertified()
    return [K.enc(d2.SecretCommit())]


def decrypt_deal(K):  # TestVSSVerifierDecryptDeal
    w = World(K)
    dealer, verifiers = w.genAll()
    v, encD = verifiers[0], dealer.EncryptedDeal(0)
    T = [t_enc(encD)]
    assert v.decryptDeal(encD).Marshal() == dealer.deals[0].Marshal()
    good = encD.DHKey
    encD.DHKey = K.dhkey(K.null())
    T.append(err(v.decryptDeal, encD))
    encD.DHKey = good
    good = encD.Signature
    encD.Signature = random_bytes(b"sig", 32)
    T.append(err(v.decryptDeal, encD))
    encD.Signature = good
    good = encD.Cipher
    encD.Cipher = random_bytes(b"cipher", len(good))
    T.append(err(v.decryptDeal, encD))
    encD.Cipher = good[:15]
    T.append(err(v.decryptDeal, encD))
    encD.Cipher = good
    if not K.rabin:  # a key that is no point under a good signature, and a cipher shorter than a tag: the key is met first
        from tests._dkg_cases import UNDECODABLE

        key, sig = encD.DHKey, encD.Signature
        encD.DHKey, encD.Cipher = UNDECODABLE, good[:15]
        encD.Signature = K.sign(w.S, w.dealerSec, UNDECODABLE)
        assert err(v.decryptDeal, encD) == "invalid Ed25519 curve point"
        encD.Cipher = good
        assert err(v.decryptDeal, encD) == "invalid Ed25519 curve point"
        encD.DHKey, encD.Signature = key, sig
    assert T[1:] == ["schnorr: invalid signature", "schnorr: signature of invalid length 32 instead of 64"] + ["cipher: message authentication failed"] * 2
    return T


def receive_deal(K):  # TestVSSVerifierReceiveDeal
    w = World(K)
    dealer, verifiers = w.genAll()
    v, d = verifiers[0], dealer.deals[0]
    encD = dealer.EncryptedDeal(0)
    resp = v.ProcessEncryptedDeal(encD)
    assert resp.StatusApproved is True and resp.Index == v.index and resp.SessionID == dealer.sid
    K.verify(v.pub, resp.Hash(), resp.Signature)
    assert v.responses[v.index] is resp
    T = [t_resp(K, resp)]
    good = encD.Signature
    encD.Signature = random_bytes(b"sig2", 32)
    T.append(err(v.ProcessEncryptedDeal, encD))  # wrong encryption
    encD.Signature = good
    goodI = d.SecShare.I
    d.SecShare.I = (goodI - 1) % 7
    T.append(err(v.ProcessEncryptedDeal, dealer.EncryptedDeal(0)))  # wrong index
    d.SecShare.I = goodI
    goodC = d.Commitments[0]
    d.Commitments[0] = K.base_mul(K.pick(w.S))
    encD = dealer.EncryptedDeal(0)
    T.append(err(v.ProcessEncryptedDeal, encD))  # (the verifier has a deal already)
    d.Commitments[0] = goodC
    T.append(err(v.ProcessEncryptedDeal, encD))  # already seen twice
    v.deal = None
    v.responses[v.index] = K.Response(StatusApproved=True)
    d.Commitments[0] = K.base_mul(K.pick(w.S))
    T.append(err(v.ProcessEncryptedDeal, encD))  # approval already existing from same origin
    d.Commitments[0] = goodC
    v.deal = None
    del v.responses[v.index]
    resp = v.ProcessEncryptedDeal(encD)  # valid complaint
    assert resp.StatusApproved is False
    T.append(t_resp(K, resp))
    assert T[1:6] == ["schnorr: signature of invalid length 32 instead of 64", "vss: verifier got wrong index from deal", "vss: verifier already received a deal",
                      "vss: verifier already received a deal", "vss: already existing response from same origin"]
    return T


def justification(K):  # TestVSSAggregatorVerifyJustification
    w = World(K)
    dealer, verifiers = w.genAll()
    v, d = verifiers[0], dealer.deals[0]
    wrongV, goodV = K.pick(w.S), d.SecShare.V
    d.SecShare.V = wrongV
    resp = v.ProcessEncryptedDeal(dealer.EncryptedDeal(0))
    assert resp.StatusApproved is False and v.responses[v.index] is resp
    d.SecShare.V = goodV
    j = dealer.ProcessResponse(resp)
    T = [t_resp(K, resp), ("just", j.SessionID, j.Index, j.Deal.Marshal(), j.Signature)]
    K.verify(dealer.pub, j.Hash(), j.Signature)
    j.Deal.SecShare.V = wrongV
    T.append(err(v.ProcessJustification, j))  # invalid deal justified
    assert v.badDealer
    j.Deal.SecShare.V = goodV
    v.badDealer = False
    assert err(v.ProcessJustification, j) is None and resp.StatusApproved is True
    good = resp.SessionID
    resp.SessionID = random_bytes(b"sid", len(good))
    T.append(err(dealer.ProcessResponse, resp))  # invalid complaint
    resp.SessionID = good
    del v.responses[v.index]
    T.append(err(v.ProcessJustification, j))
    v.responses[v.index] = resp
    T.append(err(v.ProcessJustification, j))
    assert T[2:] == ["vss: share does not verify against commitments in Deal", "vss: receiving inconsistent sessionID in response",
                     "vss: no complaints received for this justification", "vss: justification received for an approval"]
    return T


def response_duplicate(K):  # TestVSSAggregatorVerifyResponseDuplicate
    w = World(K)
    dealer, verifiers = w.genAll()
    v1, v2 = verifiers[0], verifiers[1]
    encD1, encD2 = dealer.EncryptedDeal(0), dealer.EncryptedDeal(1)
    resp1, resp2 = v1.ProcessEncryptedDeal(encD1), v2.ProcessEncryptedDeal(encD2)
    assert resp1.StatusApproved and resp2.StatusApproved
    assert v1.ProcessResponse(resp2) is None and v1.responses[v2.index] is resp2
    T = [t_resp(K, resp1), t_resp(K, resp2), err(v1.ProcessResponse, resp2)]
    del v1.responses[v2.index]
    v1.responses[v2.index] = K.Response(StatusApproved=True)
    T.append(err(v1.ProcessResponse, resp2))
    assert T[2:] == ["vss: already existing response from same origin"] * 2
    return T


def verify_response(K):  # TestVSSAggregatorVerifyResponse
    w = World(K)
    dealer, verifiers = w.genAll()
    v, deal = verifiers[0], dealer.deals[0]
    deal.SecShare.V = K.pick(w.S)
    resp = v.ProcessEncryptedDeal(dealer.EncryptedDeal(0))
    assert resp.StatusApproved is False and resp.SessionID == dealer.sid and v.responses[v.index].StatusApproved is False
    T = [t_resp(K, resp)]
    resp.Index = 7
    resp.Signature = K.sign(w.S, v.longterm, resp.Hash())
    T.append(err(v.verifyResponse, resp))
    resp.Index = 0
    good = resp.Signature
    resp.Signature = random_bytes(b"sig3", len(good))
    T.append(err(v.verifyResponse, resp))
    resp.Signature = good
    goodID = resp.SessionID
    resp.SessionID = random_bytes(b"sid2", len(goodID))
    T.append(err(v.verifyResponse, resp))
    resp.SessionID = goodID
    assert T[1:] == ["vss: index out of bounds in response", "schnorr: invalid signature", "vss: receiving inconsistent sessionID in response"]
    return T


def verifier_timeout(K):  # TestVSSVerifierTimeout
    w = World(K)
    dealer, verifiers = w.genAll()
    v = verifiers[0]
    resp = v.ProcessEncryptedDeal(dealer.EncryptedDeal(0))
    for i in range(v.t):
        v.responses[i] = K.Response(StatusApproved=True)
    assert not v.DealCertified()
    v.SetTimeout()
    assert v.DealCertified() and v.Deal() is not None
    return [t_resp(K, resp)]


def verify_deal(K):  # TestVSSAggregatorVerifyDeal, TestVSSAggregatorAddComplaint
    w = World(K)
    dealer = w.genDealer()
    deal = dealer.deals[0]
    assert err(dealer.VerifyDeal, deal, True) is None and dealer.deal is deal
    T = [err(dealer.VerifyDeal, deal, True)]
    goodT, deal.T = deal.T, 1
    T.append(err(dealer.VerifyDeal, deal, False))
    deal.T = goodT + 1  # (rabin's VerifyDeal does not compare thresholds: vss.go has no such check)
    T.append(err(dealer.VerifyDeal, deal, False))
    deal.T = goodT
    goodSid, deal.SessionID = deal.SessionID, bytes(32)
    T.append(err(dealer.VerifyDeal, deal, False))
    deal.SessionID = goodSid
    goodI = deal.SecShare.I
    deal.SecShare.I = goodI + 1
    T.append(err(dealer.VerifyDeal, deal, False))
    deal.SecShare.I = 7
    if K.rabin:
        deal.RndShare.I = 7
    T.append(err(dealer.VerifyDeal, deal, False))
    deal.SecShare.I = goodI
    if K.rabin:
        deal.RndShare.I = goodI
    deal.SecShare.V = K.pick(w.S)
    T.append(err(dealer.VerifyDeal, deal, False))
    assert T == ["vss: verifier already received a deal", "vss: invalid t received in Deal",
                 None if K.rabin else "vss: incompatible threshold - potential attack", "vss: find different sessionIDs from Deal",
                 "vss: not the same index for f and g share in Deal" if K.rabin else "vss: share does not verify against commitments in Deal",
                 "vss: index out of bounds in Deal", "vss: share does not verify against commitments in Deal"]
    c = K.Response(Index=1, StatusApproved=False)
    assert err(dealer.addResponse, c) is None and dealer.responses[1] is c
    T.append(err(dealer.addResponse, c))
    T.append(err(dealer.addResponse, K.Response(Index=7, StatusApproved=False)))
    assert T[-2:] == ["vss: already existing response from same origin", "vss: index out of bounds in Complaint"]
    return T


def small_functions(K):  # TestMinimumT, TestVSSSessionID, TestVSSFindPub, TestVSSDHExchange, TestVSSContext
    assert [K.MinimumT(n) for n in (10, 6, 4, 3, 2, 7, 8, 9)] == [6, 4, 3, 2, 2, 4, 5, 5]
    w = World(K)
    dealer = w.genDealer()
    commits = dealer.deals[0].Commitments
    sid = K.sessionID(w.S, w.dealerPub, w.verifiersPub, commits, dealer.t)
    assert sid == K.sessionID(w.S, w.dealerPub, w.verifiersPub, commits, dealer.t) == dealer.sid
    sid3 = K.sessionID(w.S, K.add(w.dealerPub, w.dealerPub), w.verifiersPub, commits, dealer.t)
    assert sid3 != sid
    p, ok = K.findPub(w.verifiersPub, 0)
    assert ok and p is w.verifiersPub[0] and K.findPub(w.verifiersPub, 7) == (None, False)
    priv = K.pick(w.S)
    dh = K.dhExchange(w.S, priv, K.base_mul(K.pick(w.S)))
    c = K.context(w.S, w.dealerPub, w.verifiersPub)
    assert len(c) == (128 if K.rabin else 32) and c == dealer.hkdfContext
    return [sid, sid3, K.enc(dh), c]


def batch_with_rejects(K, n=9):
    """process_encrypted_deals over n verifiers, each of its OWN dealer (the shape of share/dkg/rabin: a node verifies n
    dealers), with every kind of reject planted in first, middle and last place, then process_responses with a forged
    signature, a foreign session and an index out of bounds among the good ones.  The oracle's kit runs the loops."""
    S = K.stream(b"vss batch")
    vsec = [K.pick(S) for _ in range(n)]
    vpub = [K.base_mul(x) for x in vsec]
    dealers = []
    for k in range(n):
        dsec = K.pick(S)
        dealers.append(K.NewDealer(S, dsec, K.pick(S), vpub, 2 + k % (n - 1)))  # thresholds 2 .. n: one deal_check per value
    verifiers = [K.NewVerifier(S, vsec[k], dealers[k].pub, vpub) for k in range(n)]
    dealers[n // 2].deals[n // 2].SecShare.V = K.pick(S)  # a forged share: a complaint
    dealers[n - 1].deals[n - 1].SecShare.I = 0  # a foreign index
    deals = [dealers[k].EncryptedDeal(k) for k in range(n)]
    deals[0].Signature = random_bytes(b"bsig", 64)
    deals[1].Cipher = deals[1].Cipher[:-1] + bytes([deals[1].Cipher[-1] ^ 1])
    deals[2].Cipher = deals[2].Cipher[:15]
    deals[n - 2].DHKey, deals[n - 2].Signature = deals[3].DHKey, deals[3].Signature  # another dealer's key: its signature fails
    out = K.process_deals(verifiers + [verifiers[3]], deals + [deals[3]])  # the last: a verifier's second deal
    T = [t_result(K, x) for x in out]
    assert T[0] == T[n - 2] == "schnorr: invalid signature" and T[1] == T[2] == "cipher: message authentication failed"
    assert T[n - 1] == "vss: verifier got wrong index from deal" and T[n] == "vss: verifier already received a deal"
    assert out[n // 2].StatusApproved is False and out[3].StatusApproved is True
    # responses to verifier 3 about dealer 3's deal: every verifier of that dealer answers
    d = dealers[3]
    vs = [K.NewVerifier(S, vsec[k], d.pub, vpub) for k in range(n)]
    resps = K.process_deals(vs, d.EncryptedDeals())
    assert all(not isinstance(r, Exception) and r.StatusApproved for r in resps)
    bad_sig = K.Response(SessionID=resps[1].SessionID, Index=1, StatusApproved=True, Signature=random_bytes(b"rsig", 64))
    foreign = K.Response(SessionID=bytes(32), Index=2, StatusApproved=True, Signature=resps[2].Signature)
    outside = K.Response(SessionID=resps[2].SessionID, Index=n, StatusApproved=True, Signature=resps[2].Signature)
    seq = [resps[4], bad_sig, resps[1], foreign, outside, resps[1], resps[0]] + resps[5:]
    got = K.process_responses(vs[3], seq)
    T += [t_result(K, x) for x in got]
    assert [t_result(K, x) for x in got[:7]] == [None, "schnorr: invalid signature", None, "vss: receiving inconsistent sessionID in response",
                                                 "vss: index out of bounds in response", "vss: already existing response from same origin", None]
    assert sorted(set(range(n)) - set(vs[3].responses)) == [2]
    return T


def rabin_share(K):  # rabin TestVSSShare
    w = World(K)
    dealer, verifiers = w.genAll()
    ver = verifiers[0]
    assert ver.DealCertified() is False  # no aggregator yet (vss.go:732-734)
    resp = ver.ProcessEncryptedDeal(dealer.EncryptedDeal(0))
    assert resp.Approved is True
    for i in range(1, ver.t - 1):
        ver.responses[i] = K.Response(Approved=True)
    ver.SetTimeout()
    assert ver.Deal() is None  # not enough approvals
    ver.responses[ver.t] = K.Response(Approved=True)
    ver.badDealer = True
    assert ver.Deal() is None
    ver.badDealer = False
    assert ver.Deal() is not None
    return [t_resp(K, resp), ver.Deal().Marshal()]


def rabin_approvals_and_timeouts(K):
    """rabin TestVSSAggregatorEnoughApprovals, ...DealCertified, ...CleanVerifiers, TestVSSDealerSetTimeout,
    TestVSSVerifierSetTimeout"""
    w = World(K)
    dealer = w.genDealer()
    for i in range(dealer.t - 1):
        dealer.responses[i] = K.Response(Approved=True)
    dealer.SetTimeout()
    assert not dealer.EnoughApprovals() and dealer.SecretCommit() is None and dealer.Commits() is None
    dealer.responses[dealer.t] = K.Response(Approved=True)
    assert dealer.EnoughApprovals()
    for i in range(dealer.t + 1, 7):
        dealer.responses[i] = K.Response(Approved=True)
    assert dealer.EnoughApprovals() and K.enc(dealer.SecretCommit()) == K.enc(K.base_mul(w.secret))
    T = [K.enc(c) for c in dealer.Commits()]
    d2 = w.genDealer()
    for i in range(d2.t):
        d2.responses[i] = K.Response(Approved=True)
    assert d2.EnoughApprovals() and not d2.DealCertified()
    d2.cleanVerifiers()
    assert d2.DealCertified() and [r.Approved for r in d2.responses.values()] == [True] * d2.t + [False] * (7 - d2.t)
    d2.badDealer = True
    assert not d2.DealCertified() and d2.SecretCommit() is None
    d2.badDealer = False
    for i in range(d2.t):
        d2.responses[i] = K.Response(Approved=False)
    assert not d2.DealCertified()
    d3 = w.genDealer()
    for i in range(d3.t):
        d3.responses[i] = K.Response(Approved=True)
    assert not d3.DealCertified()
    d3.SetTimeout()
    assert d3.DealCertified()
    dealer, verifiers = w.genAll()
    ver = verifiers[0]
    resp = ver.ProcessEncryptedDeal(dealer.EncryptedDeal(0))
    for i in range(ver.t):
        ver.responses[i] = K.Response(Approved=True)
    assert ver.EnoughApprovals() and not ver.DealCertified()
    ver.SetTimeout()
    assert ver.DealCertified()
    return T + [t_resp(K, resp)]


RABIN_SCENARIOS = {
    "whole": whole,
    "whole, batch entries": lambda K: whole(K, batched=True),
    "loop equals batch": loop_equals_batch,
    "dealer new": dealer_new,
    "verifier new": verifier_new,
    "share": rabin_share,
    "approvals and timeouts": rabin_approvals_and_timeouts,
    "decrypt deal": decrypt_deal,
    "receive deal": receive_deal,
    "justification": justification,
    "response duplicate": response_duplicate,
    "verify response": verify_response,
    "verify deal": verify_deal,
    "small functions": small_functions,
    "batch with rejects": batch_with_rejects,
}

SCENARIOS = {
    "whole": whole,
    "whole, batch entries": lambda K: whole(K, batched=True),
    "loop equals batch": loop_equals_batch,
    "dealer new": dealer_new,
    "verifier new": verifier_new,
    "share": share,
    "dealer certified": dealer_certified,
    "decrypt deal": decrypt_deal,
    "receive deal": receive_deal,
    "justification": justification,
    "response duplicate": response_duplicate,
    "verify response": verify_response,
    "verifier timeout": verifier_timeout,
    "verify deal": verify_deal,
    "small functions": small_functions,
    "batch with rejects": batch_with_rejects,
}
