"""share/vss's engine calls restated sequentially in Python integers, hashlib and hmac over oracle/ed25519.py -- no GPU, no
engine: the checker of kyb_ed25519_schnorr_sign, kyb_ed25519_vss_seal / _open and kyb_ed25519_deal_check2, never the
thing shipped, written from the reference's text (sign/schnorr/schnorr.go, share/vss/pedersen/vss.go and dh.go,
share/vss/rabin/vss.go) and the standards.  Points are their 32 encoded bytes; scalars are their 32 bytes where the
reference keeps them unreduced and Python integers otherwise.  The second half of the file is share/vss/pedersen itself
(vss.go, dh.go, internal/v3marshaling.go and the protobuf form), function for function and one deal at a time: the checker
of kyber_amd/share/vss/pedersen.py.

AES-GCM with additional data reuses the pure-Python AES of tests/_ecies_oracle.py by import and is pinned by OpenSSL's
outputs in tests/golden/aes256gcm_aad.json; the HKDF with an info string is pinned by RFC 5869 test case 1.  The
reference's VSS tests print no bytes and no Go toolchain is at hand, so no transcript of the Go program is pinned."""
import hashlib
import hmac

from oracle import ed25519 as O
from tests import _ecies_oracle as EO

L = O.L
ST_OK, ST_BAD_POINT, ST_SHORT, ST_AUTH = 0, 1, 9, 10
ZERO_NONCE = bytes(12)


# ------------------------------------------------------------------------------------- AES-256-GCM with additional data
def _tag_aad(w, nonce: bytes, aad: bytes, ct: bytes) -> bytes:
    """SP 800-38D section 7.1: GHASH over A zero-padded, C zero-padded and the two bit lengths, masked with E(J0)"""
    h = int.from_bytes(EO.encrypt_block(w, bytes(16)), "big")
    pad = lambda b: b + bytes(-len(b) % 16)
    y = EO._ghash(h, pad(aad) + pad(ct) + (len(aad) * 8).to_bytes(8, "big") + (len(ct) * 8).to_bytes(8, "big"))
    mask = int.from_bytes(EO.encrypt_block(w, nonce + b"\0\0\0\1"), "big")
    return (y ^ mask).to_bytes(16, "big")


def gcm_seal_aad(key: bytes, nonce: bytes, msg: bytes, aad: bytes) -> bytes:
    assert len(nonce) == 12
    w = EO.expand_key(key)
    ct = EO._ctr(w, nonce, msg)
    return ct + _tag_aad(w, nonce, aad, ct)


def gcm_open_aad(key: bytes, nonce: bytes, sealed: bytes, aad: bytes):
    """the plaintext, or None (cipher: message authentication failed)"""
    if len(sealed) < 16:
        return None
    w = EO.expand_key(key)
    ct, tag = sealed[:-16], sealed[-16:]
    if not hmac.compare_digest(_tag_aad(w, nonce, aad, ct), tag):
        return None
    return EO._ctr(w, nonce, ct)


# ---------------------------------------------------------------------------------------------------------- HKDF, dh.go
def hkdf_sha256(secret: bytes, salt: bytes, info: bytes, n: int) -> bytes:
    """RFC 5869, the general function: a nil salt is HashLen zero bytes"""
    prk = hmac.new(salt or bytes(32), secret, hashlib.sha256).digest()
    out, t, i = b"", b"", 1
    while len(out) < n:
        t = hmac.new(prk, t + info + bytes([i]), hashlib.sha256).digest()
        out += t
        i += 1
    return out[:n]


def aead_key(pre: bytes, context: bytes) -> bytes:
    """newAEAD (dh.go:23-40): sharedKeyLength = 32 bytes of hkdf.New(hash, pre's bytes, nil, context)"""
    return hkdf_sha256(pre, b"", context, 32)


# ----------------------------------------------------------------------------------------------------- schnorr.go:56-82
def schnorr_sign(k: bytes, x: bytes, msg: bytes, pub: bytes = None) -> bytes:
    """Sign with the nonce given: R = k B, A = x B (Point.Mul's values for the 32 bytes as they are), h = SHA-512(R || A ||
    msg) mod l, S = k + x h mod l.  pub: the key hashed in A's place (the dealer's, in EncryptedDeal)."""
    R, A = O.mul_base(k), pub if pub is not None else O.mul_base(x)
    h = int.from_bytes(hashlib.sha512(R + A + msg).digest(), "little") % L
    S = (int.from_bytes(k, "little") + int.from_bytes(x, "little") * h) % L
    return R + S.to_bytes(32, "little")


def schnorr_holds(pub: bytes, msg: bytes, sig: bytes) -> bool:
    """the verification equation alone (RFC 8032 section 5.1.7 without cofactor): S B == R + h A"""
    R, A, S = O.decode(sig[:32]), O.decode(pub), int.from_bytes(sig[32:], "little")
    if R is None or A is None or S >= L:
        return False
    h = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % L
    return O.mul_int(S, O.B) == O.add(R, O.mul_int(h, A))


# ------------------------------------------------------------------------------ vss.go:222-255 and 443-457, per element
def seal(dh: bytes, k: bytes, dealer_priv: bytes, dealer_pub: bytes, vpub: bytes, context: bytes, msg: bytes):
    """EncryptedDeal with the ephemeral scalar and the signature's nonce given: (DHKey, Signature, Cipher), or None when
    the verifier's key does not decode"""
    pre = O.mul(dh, vpub)
    if pre is None:
        return None
    dhkey = O.mul_base(dh)
    sig = schnorr_sign(k, dealer_priv, dhkey, dealer_pub)
    return dhkey, sig, gcm_seal_aad(aead_key(pre, context), ZERO_NONCE, msg, context)


def open_(priv: bytes, dhkey: bytes, context: bytes, cipher: bytes):
    """decryptDeal after its Verify: (plaintext, 0) or (None, status)"""
    if len(cipher) < 16:
        return None, ST_SHORT
    pre = O.mul(priv, dhkey)
    if pre is None:
        return None, ST_BAD_POINT
    msg = gcm_open_aad(aead_key(pre, context), ZERO_NONCE, cipher, context)
    return (msg, ST_OK) if msg is not None else (None, ST_AUTH)


# ------------------------------------------------------------------------------------------------ rabin/vss.go:611-651
def pub_eval(commits, idx: int):
    """PubPoly.Eval (share/poly.go:340-348) at x = idx + 1 on decoded commitments"""
    x, v = idx + 1, O.IDENTITY
    for c in reversed(commits):
        v = O.add(O.mul_int(x, v), c)
    return v


def deal_check2(f: bytes, g: bytes, commits, H: bytes, idx: int):
    """Equal(Add(Mul(f, nil), Mul(g, H)), Eval(idx).V) on raw 32-byte scalars: 1, 0, or None when H or a commitment does
    not decode"""
    pts = [O.decode(c) for c in commits]
    gh = O.mul(g, H)
    if gh is None or any(p is None for p in pts):
        return None
    left = O.add(O.decode(O.mul_base(f)), O.decode(gh))
    return 1 if O.encode(left) == O.encode(pub_eval(pts, idx)) else 0


# ===================================================================================================================
# share/vss/pedersen (vss.go, dh.go, internal/v3marshaling.go, internal/protobuf) restated sequentially: every deal is
# sealed, opened and checked one at a time, in the reference's order.  Points are their 32 encoded bytes, scalars Python
# integers; a random stream is a callable read(n) (the streams of util/blake2xb); a Go error is a raised ValueError
# with the reference's string.
import struct  # noqa: E402

from kyber_amd.util.blake2xb import pick_int  # noqa: E402
from tests import _dkg_oracle as DO  # noqa: E402  (sign/schnorr and share/poly, restated there)

StatusComplaint, StatusApproval = False, True


def pick(read) -> int:
    return pick_int(read)[0]


def sc(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


# ------------------------------------------------------------------------------------------------- internal/protobuf
def pb_uvarint(v: int) -> bytes:
    out = b""
    while v > 127:
        out += bytes([v & 127 | 128])
        v >>= 7
    return out + bytes([v])


def pb_bytes(num: int, b: bytes) -> bytes:  # wire type 2: a key, a length, the bytes; no type tag
    return pb_uvarint(num * 8 + 2) + pb_uvarint(len(b)) + b


def pb_uint(num: int, v: int) -> bytes:  # wire type 0, plain
    return pb_uvarint(num * 8) + pb_uvarint(v)


def pb_sint(num: int, v: int) -> bytes:  # wire type 0, zigzag: 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...
    return pb_uvarint(num * 8) + pb_uvarint(2 * v if v >= 0 else -2 * v - 1)


def pb_parse(buf: bytes):
    out, p = [], 0

    def varint():
        nonlocal p
        v = s = 0
        while True:
            if p >= len(buf):
                raise ValueError("bad protobuf varint value")
            b = buf[p]
            p += 1
            v |= (b & 127) << s
            s += 7
            if b < 128:
                return v

    while p < len(buf):
        key = varint()
        if key & 7 == 0:
            out.append((key >> 3, 0, varint()))
        elif key & 7 == 2:
            n = varint()
            if p + n > len(buf):
                raise ValueError("bad protobuf length-delimited value")
            out.append((key >> 3, 2, buf[p:p + n]))
            p += n
        else:
            raise ValueError("unknown protobuf wire-type")
    return out


class PriShare:
    def __init__(self, I, V):
        self.I, self.V = I, V


class Deal:
    def __init__(self, SessionID, SecShare, T, Commitments):
        self.SessionID, self.SecShare, self.T, self.Commitments = SessionID, SecShare, T, Commitments

    def Marshal(self) -> bytes:  # vss.go:73-85 over v3marshaling.go:28-34
        share = pb_sint(1, self.SecShare.I) + pb_bytes(2, sc(self.SecShare.V))
        return pb_bytes(1, self.SessionID) + pb_bytes(2, share) + pb_uint(3, self.T) + b"".join(pb_bytes(4, c) for c in self.Commitments)

    @staticmethod
    def Unmarshal(data: bytes) -> "Deal":  # vss.go:89-107
        sid, share, t, commits = b"", b"", 0, []
        for num, wt, v in pb_parse(data):
            if num == 1:
                sid = v
            elif num == 2:
                share = v
            elif num == 3:
                t = v
            elif num == 4:
                if len(v) != 32 or O.decode(v) is None:
                    raise ValueError("invalid Ed25519 curve point")
                commits.append(O.encode(O.decode(v)))
        i, val = 0, None
        for num, wt, v in pb_parse(share):
            if num == 1:
                i = v // 2 if v % 2 == 0 else -(v + 1) // 2
            elif num == 2:
                val = int.from_bytes(v, "little")
        if i < 0 or i > 2**32 - 1:
            raise ValueError("cannot cast I as uint32 due to overflow")
        return Deal(sid, PriShare(i, val), t, commits)


class EncryptedDeal:
    def __init__(self, DHKey, Signature, Cipher):
        self.DHKey, self.Signature, self.Cipher = DHKey, Signature, Cipher


class Response:
    def __init__(self, SessionID=b"", Index=0, StatusApproved=False, Signature=b""):
        self.SessionID, self.Index, self.StatusApproved, self.Signature = SessionID, Index, StatusApproved, Signature

    Approved = property(lambda self: self.StatusApproved, lambda self, v: setattr(self, "StatusApproved", v))  # rabin's name

    def Hash(self) -> bytes:
        return hashlib.sha256(b"response" + (self.SessionID or b"") + struct.pack("<I", self.Index) + bytes([int(self.StatusApproved)])).digest()


class Justification:
    def __init__(self, SessionID, Index, Deal, Signature=b""):
        self.SessionID, self.Index, self.Deal, self.Signature = SessionID, Index, Deal, Signature

    def Hash(self) -> bytes:
        return hashlib.sha256(b"justification" + self.SessionID + struct.pack("<I", self.Index) + self.Deal.Marshal()).digest()


def MinimumT(n):
    return n // 2 + 1


def validT(t, verifiers):
    return 2 <= t <= len(verifiers)


def findPub(verifiers, idx):
    return (verifiers[idx], True) if idx < len(verifiers) else (None, False)


def sessionID(dealer, verifiers, commitments, t):
    return hashlib.sha256(dealer + b"".join(verifiers) + b"".join(commitments) + struct.pack("<I", t)).digest()


def context(dealer, verifiers):
    return hashlib.sha256(b"vss-dealer" + dealer + b"vss-verifiers" + b"".join(verifiers)).digest()


def dhExchange(priv: int, pub: bytes):
    return O.mul(sc(priv), pub)


def schnorr_verify(pub, msg, sig):  # schnorr.go:163-169: the length first, with its numbers
    if len(sig) != 64:
        raise ValueError("schnorr: signature of invalid length %d instead of %d" % (len(sig), 64))
    DO.Scheme(None).Verify(pub, msg, sig)


class Aggregator:
    def __init__(self, dealer, verifiers, commits, t, sid):
        self.dealer, self.verifiers, self.commits, self.t, self.sid = dealer, verifiers, commits, t, sid
        self.responses, self.deal, self.badDealer, self.timeout = {}, None, False, False

    def VerifyDeal(self, d, inclusion):
        if self.deal is not None and inclusion:
            raise ValueError("vss: verifier already received a deal")
        if self.deal is None:
            self.commits, self.sid, self.deal, self.t = d.Commitments, d.SessionID, d, d.T
        if not validT(d.T, self.verifiers):
            raise ValueError("vss: invalid t received in Deal")
        if d.T != self.t:
            raise ValueError("vss: incompatible threshold - potential attack")
        if self.sid != d.SessionID:
            raise ValueError("vss: find different sessionIDs from Deal")
        if d.SecShare.I >= len(self.verifiers):
            raise ValueError("vss: index out of bounds in Deal")
        if O.mul_base(sc(d.SecShare.V)) != O.encode(pub_eval([O.decode(c) for c in d.Commitments], d.SecShare.I)):
            raise ValueError("vss: share does not verify against commitments in Deal")

    def SetThreshold(self, t):
        self.t = t

    def verifyResponse(self, r):
        if self.sid is not None and r.SessionID != self.sid:
            raise ValueError("vss: receiving inconsistent sessionID in response")
        pub, ok = findPub(self.verifiers, r.Index)
        if not ok:
            raise ValueError("vss: index out of bounds in response")
        schnorr_verify(pub, r.Hash(), r.Signature)
        self.addResponse(r)

    def verifyJustification(self, j):
        if not findPub(self.verifiers, j.Index)[1]:
            raise ValueError("vss: index out of bounds in justification")
        if j.Index not in self.responses:
            raise ValueError("vss: no complaints received for this justification")
        r = self.responses[j.Index]
        if r.StatusApproved:
            raise ValueError("vss: justification received for an approval")
        try:
            self.VerifyDeal(j.Deal, False)
        except ValueError:
            self.badDealer = True
            raise
        r.StatusApproved = StatusApproval

    def addResponse(self, r):
        if not findPub(self.verifiers, r.Index)[1]:
            raise ValueError("vss: index out of bounds in Complaint")
        if r.Index in self.responses:
            raise ValueError("vss: already existing response from same origin")
        self.responses[r.Index] = r

    def DealCertified(self):
        absent = sum(1 for i in range(len(self.verifiers)) if i not in self.responses)
        approvals = sum(1 for i in range(len(self.verifiers)) if i in self.responses and self.responses[i].StatusApproved)
        complaint = any(i in self.responses and not self.responses[i].StatusApproved for i in range(len(self.verifiers)))
        base = not self.badDealer and approvals >= self.t and not complaint
        if self.timeout:
            return base and not absent > (len(self.verifiers) - self.t) % 2**32
        return base and absent <= 0

    def MissingResponses(self):
        return [i for i in range(len(self.verifiers)) if i not in self.responses]

    def SetTimeout(self):
        self.timeout = True

    ProcessResponse = verifyResponse


class Dealer(Aggregator):
    def __init__(self, read, longterm, secret, verifiers, t):
        if not validT(t, verifiers):
            raise ValueError("dealer: t %d invalid" % t)
        self.read, self.long, self.secret = read, longterm, secret
        self.coeffs = [secret] + [pick(read) for _ in range(t - 1)]  # NewPriPoly: the secret stands
        self.pub = DO.base_mul(longterm)
        self.secretCommits = [DO.base_mul(c) for c in self.coeffs]
        self.sessionID = sessionID(self.pub, verifiers, self.secretCommits, t)
        super().__init__(self.pub, verifiers, self.secretCommits, t, self.sessionID)
        self.deals = [Deal(self.sessionID, PriShare(i, DO.pri_eval(self.coeffs, i)), t, self.secretCommits) for i in range(len(verifiers))]
        self.hkdfContext = context(self.pub, verifiers)

    def PlaintextDeal(self, i):
        if i >= len(self.deals):
            raise ValueError("dealer: PlaintextDeal given wrong index")
        return self.deals[i]

    def EncryptedDeal(self, i):
        vpub, ok = findPub(self.verifiers, i)
        if not ok:
            raise ValueError("dealer: wrong index to generate encrypted deal")
        dh = pick(self.read)
        dhkey = DO.base_mul(dh)
        sig = DO.Scheme(self.read).Sign(self.long, dhkey)
        pre = dhExchange(dh, vpub)
        cipher = gcm_seal_aad(aead_key(pre, self.hkdfContext), ZERO_NONCE, self.deals[i].Marshal(), self.hkdfContext)
        return EncryptedDeal(dhkey, sig, cipher)

    def EncryptedDeals(self):
        return [self.EncryptedDeal(i) for i in range(len(self.verifiers))]

    def ProcessResponse(self, r):
        self.verifyResponse(r)
        if r.StatusApproved:
            return None
        j = Justification(self.sessionID, r.Index, self.deals[r.Index])
        j.Signature = DO.Scheme(self.read).Sign(self.long, j.Hash())
        return j

    def SecretCommit(self):
        return DO.base_mul(self.secret) if self.DealCertified() else None


class Verifier(Aggregator):
    def __init__(self, read, longterm, dealerKey, verifiers):
        pub = DO.base_mul(longterm)
        if pub not in verifiers:
            raise ValueError("vss: public key not found in the list of verifiers")
        super().__init__(None, verifiers, None, 0, None)
        self.read, self.longterm, self.pub, self.index, self.dealer = read, longterm, pub, verifiers.index(pub), dealerKey
        self.hkdfContext = context(dealerKey, verifiers)

    def decryptDeal(self, e):
        schnorr_verify(self.dealer, e.DHKey, e.Signature)
        if len(e.DHKey) != 32 or O.decode(e.DHKey) is None:
            raise ValueError("invalid Ed25519 curve point")
        pre = dhExchange(self.longterm, e.DHKey)
        plain = gcm_open_aad(aead_key(pre, self.hkdfContext), ZERO_NONCE, e.Cipher, self.hkdfContext)
        if plain is None:
            raise ValueError("cipher: message authentication failed")
        return Deal.Unmarshal(plain)

    def ProcessEncryptedDeal(self, e):
        d = self.decryptDeal(e)
        if d.SecShare.I != self.index:
            raise ValueError("vss: verifier got wrong index from deal")
        r = Response(sessionID(self.dealer, self.verifiers, d.Commitments, d.T), self.index, StatusApproval)
        try:
            self.VerifyDeal(d, True)
        except ValueError as err:
            if str(err) == "vss: verifier already received a deal":
                raise
            r.StatusApproved = StatusComplaint
        r.Signature = DO.Scheme(self.read).Sign(self.longterm, r.Hash())
        self.addResponse(r)
        return r

    def ProcessResponse(self, resp):
        if self.deal is None:
            raise ValueError("verifier: need to receive deal before response")
        self.verifyResponse(resp)

    def ProcessJustification(self, j):
        self.verifyJustification(j)

    def Deal(self):
        return self.deal if self.DealCertified() else None

    def UnsafeSetResponseDKG(self, idx, approval):
        try:
            self.addResponse(Response(self.sid, idx, approval))
        except ValueError:
            pass


def RecoverSecret(deals, n, t):
    if any(d.SessionID != deals[0].SessionID for d in deals):
        raise ValueError("vss: all deals need to have same session id")
    return DO.recover_secret([(d.SecShare.I, d.SecShare.V) for d in deals], t)


# ===================================================================================================================
# share/vss/rabin (rabin/vss.go, rabin/dh.go) restated the same way.  What reads the same in both Go files is inherited
# from the classes above; everything the two files differ in is written out here from rabin's text.
from kyber_amd.util import blake2xb as _xof  # noqa: E402  (the suite's XOF; its outputs are pinned by tests/test_blake2xb*.py)


def point_pick(read) -> bytes:
    """Point.Pick(rand) = Embed(nil, rand) (point.go:132-182): 32 stream bytes until they decode to a point whose
    multiple by the cofactor is not the identity; that multiple"""
    while True:
        p = O.decode(read(32))
        if p is None:
            continue
        q = O.mul_int(8, p)
        if q != O.IDENTITY:
            return O.encode(q)


def deriveH(verifiers) -> bytes:  # rabin/vss.go:775-782
    return point_pick(_xof.New(b"".join(verifiers)).Read)


def rabin_context(dealer, verifiers) -> bytes:  # rabin/dh.go:46-67: 128 bytes of the XOF seeded "vss-dealer"
    h = _xof.New(b"vss-dealer")
    h.Write(dealer)
    h.Write(b"vss-verifiers")
    for v in verifiers:
        h.Write(v)
    return h.Read(128)


class RabinDeal:
    def __init__(self, SessionID, SecShare, RndShare, T, Commitments):
        self.SessionID, self.SecShare, self.RndShare, self.T, self.Commitments = SessionID, SecShare, RndShare, T, Commitments

    def Marshal(self) -> bytes:  # rabin/vss.go:102-119
        f = pb_sint(1, self.SecShare.I) + pb_bytes(2, sc(self.SecShare.V))
        g = pb_sint(1, self.RndShare.I) + pb_bytes(2, sc(self.RndShare.V))
        return pb_bytes(1, self.SessionID) + pb_bytes(2, f) + pb_bytes(3, g) + pb_uint(4, self.T) + b"".join(pb_bytes(5, c) for c in self.Commitments)

    @staticmethod
    def Unmarshal(data: bytes) -> "RabinDeal":  # rabin/vss.go:123-147
        got = {1: b"", 2: b"", 3: b"", 4: 0}
        commits = []
        for num, wt, v in pb_parse(data):
            if num == 5:
                if len(v) != 32 or O.decode(v) is None:
                    raise ValueError("invalid Ed25519 curve point")
                commits.append(O.encode(O.decode(v)))
            elif num in got:
                got[num] = v
        shares = []
        for raw in (got[2], got[3]):
            i, val = 0, None
            for num, wt, v in pb_parse(raw):
                if num == 1:
                    i = v // 2 if v % 2 == 0 else -(v + 1) // 2
                elif num == 2:
                    val = int.from_bytes(v, "little")
            if i < 0 or i > 2**32 - 1:
                raise ValueError("cannot cast I as uint32 due to overflow")
            shares.append(PriShare(i, val))
        return RabinDeal(got[1], shares[0], shares[1], got[4], commits)


class RabinAggregator(Aggregator):
    def VerifyDeal(self, d, inclusion):  # rabin/vss.go:611-651
        if self.deal is not None and inclusion:
            raise ValueError("vss: verifier already received a deal")
        if self.deal is None:
            self.commits, self.sid, self.deal = d.Commitments, d.SessionID, d
        if not validT(d.T, self.verifiers):
            raise ValueError("vss: invalid t received in Deal")
        if self.sid != d.SessionID:
            raise ValueError("vss: find different sessionIDs from Deal")
        if d.SecShare.I != d.RndShare.I:
            raise ValueError("vss: not the same index for f and g share in Deal")
        if d.SecShare.I >= len(self.verifiers):
            raise ValueError("vss: index out of bounds in Deal")
        ci = O.add(O.decode(O.mul_base(sc(d.SecShare.V))), O.decode(O.mul(sc(d.RndShare.V), deriveH(self.verifiers))))
        if O.encode(ci) != O.encode(pub_eval([O.decode(c) for c in d.Commitments], d.SecShare.I)):
            raise ValueError("vss: share does not verify against commitments in Deal")

    def verifyResponse(self, r):  # rabin/vss.go:667-682: the session is compared whether or not there is one
        if (r.SessionID or b"") != (self.sid or b""):
            raise ValueError("vss: receiving inconsistent sessionID in response")
        pub, ok = findPub(self.verifiers, r.Index)
        if not ok:
            raise ValueError("vss: index out of bounds in response")
        schnorr_verify(pub, r.Hash(), r.Signature)
        self.addResponse(r)

    ProcessResponse = verifyResponse

    def cleanVerifiers(self):  # rabin/vss.go:655-665
        for i in range(len(self.verifiers)):
            if i not in self.responses:
                self.responses[i] = Response(self.sid, i, False)

    SetTimeout = cleanVerifiers

    def EnoughApprovals(self):  # rabin/vss.go:718-726
        return sum(1 for r in self.responses.values() if r.StatusApproved) >= self.t

    def DealCertified(self):  # rabin/vss.go:730-747
        unstable = sum(1 for i in range(len(self.verifiers)) if i not in self.responses)
        return self.EnoughApprovals() and not (unstable > 0 or self.badDealer)


class RabinDealer(RabinAggregator):
    def __init__(self, read, longterm, secret, verifiers, t):  # rabin/vss.go:193-245
        if not validT(t, verifiers):
            raise ValueError("dealer: t %d invalid" % t)
        self.read, self.long, self.secret = read, longterm, secret
        H = O.decode(deriveH(verifiers))
        f = [secret] + [pick(read) for _ in range(t - 1)]
        g = [pick(read) for _ in range(t)]
        self.pub = DO.base_mul(longterm)
        self.secretCommits = [DO.base_mul(c) for c in f]
        commitments = [O.encode(O.add(O.decode(F), O.mul_int(b, H))) for F, b in zip(self.secretCommits, g)]
        self.sessionID = sessionID(self.pub, verifiers, commitments, t)
        Aggregator.__init__(self, self.pub, verifiers, commitments, t, self.sessionID)
        self.deals = [RabinDeal(self.sessionID, PriShare(i, DO.pri_eval(f, i)), PriShare(i, DO.pri_eval(g, i)), t, commitments)
                      for i in range(len(verifiers))]
        self.hkdfContext = rabin_context(self.pub, verifiers)

    PlaintextDeal = Dealer.PlaintextDeal
    EncryptedDeal = Dealer.EncryptedDeal  # rabin/vss.go:263-297: the same steps; DHKey travels as a point, here its bytes
    EncryptedDeals = Dealer.EncryptedDeals
    ProcessResponse = Dealer.ProcessResponse

    def SecretCommit(self):
        return DO.base_mul(self.secret) if self.EnoughApprovals() and self.DealCertified() else None

    def Commits(self):
        return self.secretCommits if self.EnoughApprovals() and self.DealCertified() else None


class RabinVerifier(RabinAggregator):
    def __init__(self, read, longterm, dealerKey, verifiers):  # rabin/vss.go:393-426
        pub = DO.base_mul(longterm)
        if pub not in verifiers:
            raise ValueError("vss: public key not found in the list of verifiers")
        Aggregator.__init__(self, dealerKey, verifiers, None, 0, None)
        self.read, self.longterm, self.pub, self.index = read, longterm, pub, verifiers.index(pub)
        self.has_aggregator = False  # v.aggregator == nil
        self.hkdfContext = rabin_context(dealerKey, verifiers)

    def decryptDeal(self, e):  # rabin/vss.go:479-503
        schnorr_verify(self.dealer, e.DHKey, e.Signature)
        pre = dhExchange(self.longterm, e.DHKey)
        plain = gcm_open_aad(aead_key(pre, self.hkdfContext), ZERO_NONCE, e.Cipher, self.hkdfContext)
        if plain is None:
            raise ValueError("cipher: message authentication failed")
        return RabinDeal.Unmarshal(plain)

    def ProcessEncryptedDeal(self, e):  # rabin/vss.go:436-476
        d = self.decryptDeal(e)
        if d.SecShare.I != self.index:
            raise ValueError("vss: verifier got wrong index from deal")
        sid = sessionID(self.dealer, self.verifiers, d.Commitments, d.T)
        if not self.has_aggregator:
            self.commits, self.t, self.sid, self.has_aggregator = d.Commitments, d.T, d.SessionID, True
        r = Response(sid, self.index, True)
        try:
            self.VerifyDeal(d, True)
        except ValueError as err:
            if str(err) == "vss: verifier already received a deal":
                raise
            r.StatusApproved = False
        r.Signature = DO.Scheme(self.read).Sign(self.longterm, r.Hash())
        self.addResponse(r)
        return r

    def _need(self):
        if not self.has_aggregator:
            raise ValueError("vss: verifier has no aggregator before its first deal")  # (Go dereferences nil here)

    def ProcessResponse(self, resp):
        self._need()
        self.verifyResponse(resp)

    def ProcessJustification(self, j):
        self.verifyJustification(j)

    def EnoughApprovals(self):
        self._need()
        return RabinAggregator.EnoughApprovals(self)

    def DealCertified(self):  # false on a nil aggregator (rabin/vss.go:732-734)
        return self.has_aggregator and RabinAggregator.DealCertified(self)

    def SetTimeout(self):
        self._need()
        self.cleanVerifiers()

    def Deal(self):
        return self.deal if self.EnoughApprovals() and self.DealCertified() else None
