"""sign/dss (dss.go) restated sequentially in Python integers over oracle/ed25519.py, and the two engine calls'
element-by-element values (kyb_ed25519_dss_check, kyb_ed25519_dss_partial): the checker, never the thing shipped.

Points are their 32 encoded bytes, scalars Python integers, a random stream is a callable read(n), a Go error is a
raised ValueError with the reference's string.

Limit of the check: the reference's dss_test.go prints no bytes and no Go toolchain is at hand, so no transcript of the
Go program is pinned.  The outside pins are: the final signature is an EdDSA signature of the message under the
distributed public key (dss_test.go:133-135), so Signature() must pass the standing eddsa oracle
(tests/_ed_verify_oracle.py) and kyb_ed25519_verify; every PartialSig.Signature must pass schnorr.Verify; and
h = SHA-512(R || A || msg) mod l is pinned by an RFC 8032 row already in tests/golden (its S = r + h a).  The composition is
this file's, written from dss.go's text."""
import hashlib
import struct

from oracle import ed25519 as O
from tests import _dkg_oracle as DO
from tests import _ed_verify_oracle as V
from tests import _vss_oracle as VO

L = O.L
ST_OK, ST_BAD_POINT = 0, 1
ST_DSS_INDEX, ST_DSS_SIG, ST_DSS_SESSION, ST_DSS_PARTIAL = 14, 15, 16, 17  # include/kyber_hip.h

ErrInvalidSignatureIndex = "dss: partial signature with invalid index"


def sc(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


# ------------------------------------------------------------------------------------------------ the hashes of dss.go
def hash_sig(rand0: bytes, long0: bytes, msg: bytes) -> int:
    """hashSig (dss.go:201-211): the commitments enter through the bytes MarshalTo writes"""
    return int.from_bytes(hashlib.sha512(rand0 + long0 + msg).digest(), "little") % L


def session_id(long_commits, rand_commits) -> bytes:
    """sessionID (dss.go:235-246)"""
    return hashlib.sha256(b"".join(long_commits) + b"".join(rand_commits)).digest()


def partial_hash(v: bytes, index: int, sid: bytes) -> bytes:
    """PartialSig.Hash (dss.go:221-226) over PriShare.Hash (share/poly.go:35-40)"""
    return hashlib.sha256(hashlib.sha256(v + struct.pack("<I", index)).digest() + sid).digest()


# ------------------------------------------------------------------------------------- the engine calls, per element
def partial(priv: bytes, index: int, alpha: bytes, beta: bytes, k: bytes, long_commits, rand_commits, msg: bytes):
    """(V, sid, sig) of kyb_ed25519_dss_partial for one session"""
    h = hash_sig(rand_commits[0], long_commits[0], msg)
    v = sc(h * int.from_bytes(alpha, "little") + int.from_bytes(beta, "little"))
    sid = session_id(long_commits, rand_commits)
    return v, sid, VO.schnorr_sign(k, priv, partial_hash(v, index, sid))


def folded(long_commits, rand_commits, msg: bytes):
    """D_k = R_k + h A_k, k < max(tl, tr), as encoded points; None when a commitment does not decode"""
    h = hash_sig(rand_commits[0], long_commits[0], msg)
    A, R = [O.decode(c) for c in long_commits], [O.decode(c) for c in rand_commits]
    if any(p is None for p in A + R):
        return None
    T = max(len(A), len(R))
    A += [O.IDENTITY] * (T - len(A))
    R += [O.IDENTITY] * (T - len(R))
    return [O.encode(O.add(r, O.mul_int(h, a))) for r, a in zip(R, A)]


def right_side(long_commits, rand_commits, msg: bytes, index: int):
    """randomPoly.Eval(I).V + h longPoly.Eval(I).V as dss.go:160-165 computes it (NOT through the fold)"""
    h = hash_sig(rand_commits[0], long_commits[0], msg)
    A, R = [O.decode(c) for c in long_commits], [O.decode(c) for c in rand_commits]
    if any(p is None for p in A + R):
        return None
    return O.encode(O.add(VO.pub_eval(R, index), O.mul_int(h, VO.pub_eval(A, index))))


def check(participants, long_commits, rand_commits, msg: bytes, index: int, v: bytes, sid: bytes, sig: bytes):
    """(ok, status) of kyb_ed25519_dss_check for one partial signature of one session"""
    if index >= len(participants):
        return 0, ST_DSS_INDEX
    pub, m = participants[index], partial_hash(v, index, sid)
    st = V.abi_status(pub, m, sig)
    if st:
        return 0, st
    if not V.verify_with_checks(pub, m, sig)[0]:
        return 0, ST_DSS_SIG
    if sid != session_id(long_commits, rand_commits):
        return 0, ST_DSS_SESSION
    right = right_side(long_commits, rand_commits, msg, index)
    if right is None:
        return 0, ST_BAD_POINT
    return (1, ST_OK) if O.mul_base(v) == right else (0, ST_DSS_PARTIAL)


# ------------------------------------------------------------------------------------------------------- dss.go, in full
class PriShare:
    def __init__(self, I, V):
        self.I, self.V = I, V


class PartialSig:
    def __init__(self, Partial, SessionID, Signature):
        self.Partial, self.SessionID, self.Signature = Partial, SessionID, Signature

    def Hash(self) -> bytes:
        return hashlib.sha256(hashlib.sha256(sc(self.Partial.V) + struct.pack("<I", self.Partial.I)).digest() + self.SessionID).digest()


class DistKeyShare:
    """what share/dkg/rabin's DistKeyShare gives dss: the commitments (encoded) and the private share"""

    def __init__(self, commits, share: PriShare):
        self.Commits, self.Share = list(commits), share

    def PriShare(self):
        return self.Share

    def Commitments(self):
        return self.Commits


def schnorr_verify(pub: bytes, msg: bytes, sig: bytes):
    """schnorr.Verify (schnorr.go:84-169) with the reference's error strings"""
    VO.schnorr_verify(pub, msg, sig)


class DSS:
    def __init__(self, read, secret: int, participants, long, random, msg: bytes, t: int):  # NewDSS, dss.go:77-107
        self.read, self.secret, self.public = read, secret, O.mul_base(sc(secret))
        self.index = None
        for j, p in enumerate(participants):
            if p == self.public:
                self.index = j
                break
        if self.index is None:
            raise ValueError("dss: public key not found in list of participants")
        self.participants, self.long, self.random, self.msg, self.T = list(participants), long, random, msg, t
        self.partials, self.partialsIdx, self.signed = [], {}, False
        self.sessionID = session_id(long.Commitments(), random.Commitments())

    def hashSig(self) -> int:
        return hash_sig(self.random.Commitments()[0], self.long.Commitments()[0], self.msg)

    def PartialSig(self) -> PartialSig:  # dss.go:113-134
        v = (self.hashSig() * self.long.PriShare().V + self.random.PriShare().V) % L
        ps = PartialSig(PriShare(self.index, v), self.sessionID, b"")
        ps.Signature = DO.Scheme(self.read).Sign(self.secret, ps.Hash())
        if not self.signed:
            self.partialsIdx[self.index] = True
            self.partials.append(ps.Partial)
            self.signed = True
        return ps

    def ProcessPartialSig(self, ps: PartialSig):  # dss.go:141-173
        if ps.Partial.I >= len(self.participants):
            raise ValueError(ErrInvalidSignatureIndex)
        schnorr_verify(self.participants[ps.Partial.I], ps.Hash(), ps.Signature)
        if ps.SessionID != self.sessionID:
            raise ValueError("dss: session id do not match")
        if ps.Partial.I in self.partialsIdx:
            raise ValueError("dss: partial signature already received from peer")
        right = right_side(self.long.Commitments(), self.random.Commitments(), self.msg, ps.Partial.I)
        if O.mul_base(sc(ps.Partial.V)) != right:
            raise ValueError("dss: partial signature not valid")
        self.partialsIdx[ps.Partial.I] = True
        self.partials.append(ps.Partial)

    def EnoughPartialSig(self) -> bool:
        return len(self.partials) >= self.T

    def Signature(self) -> bytes:  # dss.go:186-199
        if not self.EnoughPartialSig():
            raise ValueError("dkg: not enough partial signatures to sign")
        gamma = DO.recover_secret([(p.I, p.V) for p in self.partials], self.T)
        return self.random.Commitments()[0] + sc(gamma)


def Verify(public: bytes, msg: bytes, sig: bytes):
    """dss.Verify = eddsa.Verify (dss.go:215-217)"""
    ok, why = V.verify_with_checks(public, msg, sig)
    if not ok:
        raise ValueError(why)
