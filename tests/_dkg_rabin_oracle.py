"""share/dkg/rabin (dkg.go) restated sequentially in Python integers over oracle/ed25519.py and the standing Rabin VSS
oracle (tests/_vss_oracle.py): the checker of kyber_amd.share.dkg_rabin, never the thing shipped.  Points are their 32
encoded bytes, scalars Python integers, a random stream is a callable read(n), a Go error is a raised ValueError with the
reference's string, a panic a RuntimeError.  QUAL is walked in ascending index order (Go's map order is not defined).

Limit of the check: the reference's dkg_test.go prints no bytes and no Go toolchain is at hand, so no transcript of the Go
program is pinned.  The outside pins are those of the VSS oracle underneath (AES-GCM, HKDF, the wire form, RFC 8032's
equation) and the algebra: every participant's DistKeyShare carries the same commitments, its share lies on them, and t
shares recover the secret whose commitment is Public().  The composition is this file's, written from dkg.go's text."""
import hashlib
import struct

from oracle import ed25519 as O
from tests import _dkg_oracle as DO
from tests import _vss_oracle as VO

L = O.L


class DistKeyShare:
    def __init__(self, Commits, Share):
        self.Commits, self.Share = Commits, Share

    def Public(self):
        return self.Commits[0]

    def PriShare(self):
        return self.Share

    def Commitments(self):
        return self.Commits


class Deal:
    def __init__(self, Index, Deal):
        self.Index, self.Deal = Index, Deal


class Response:
    def __init__(self, Index, Response):
        self.Index, self.Response = Index, Response


class Justification:
    def __init__(self, Index, Justification):
        self.Index, self.Justification = Index, Justification


class SecretCommits:
    def __init__(self, Index, Commitments, SessionID, Signature=b""):
        self.Index, self.Commitments, self.SessionID, self.Signature = Index, Commitments, SessionID, Signature

    def Hash(self):
        return hashlib.sha256(b"secretcommits" + struct.pack("<I", self.Index) + b"".join(self.Commitments)).digest()


class ComplaintCommits:
    def __init__(self, Index, DealerIndex, Deal, Signature=b""):
        self.Index, self.DealerIndex, self.Deal, self.Signature = Index, DealerIndex, Deal, Signature

    def Hash(self):
        return hashlib.sha256(b"commitcomplaint" + struct.pack("<II", self.Index, self.DealerIndex) + self.Deal.Marshal()).digest()


class ReconstructCommits:
    def __init__(self, SessionID, Index, DealerIndex, Share, Signature=b""):
        self.SessionID, self.Index, self.DealerIndex, self.Share, self.Signature = SessionID, Index, DealerIndex, Share, Signature

    def Hash(self):
        inner = hashlib.sha256(VO.sc(self.Share.V) + struct.pack("<I", self.Share.I)).digest()
        return hashlib.sha256(b"reconstructcommits" + struct.pack("<II", self.Index, self.DealerIndex) + inner).digest()


def _check(commits, s) -> bool:  # PubPoly.Check, share/poly.go:405-409
    return O.mul_base(VO.sc(s.V)) == DO.pub_eval(commits, s.I)


def _unsafe_set(agg, idx, approval):  # UnsafeSetResponseDKG, rabin/vss.go:751-760: the error is dropped
    try:
        agg.addResponse(VO.Response(agg.sid, idx, approval))
    except ValueError:
        pass


class DistKeyGenerator:
    def __init__(self, read, longterm, participants, t):  # dkg.go:180-221
        pub = DO.base_mul(longterm)
        if pub not in participants:
            raise ValueError("dkg: own public key not found in list of participants")
        self.index = participants.index(pub)
        ownSec = VO.pick(read)
        self.dealer = VO.RabinDealer(read, longterm, ownSec, participants, t)
        self.verifiers, self.commitments, self.pendingReconstruct, self.reconstructed = {}, {}, {}, {}
        self.read, self.t, self.long, self.pub, self.participants = read, t, longterm, pub, participants

    def sign(self, msg):
        return DO.Scheme(self.read).Sign(self.long, msg)

    def Deals(self):  # dkg.go:234-266
        deals = self.dealer.EncryptedDeals()
        dd = {}
        for i in range(len(self.participants)):
            distd = Deal(self.index, deals[i])
            if i == self.index:
                if self.index in self.verifiers:
                    continue
                try:
                    resp = self.ProcessDeal(distd)
                except ValueError as err:
                    raise RuntimeError(str(err))
                if not resp.Response.StatusApproved:
                    raise RuntimeError("dkg: own deal gave a complaint")
                _unsafe_set(self.dealer, self.index, True)
                continue
            dd[i] = distd
        return dd

    def ProcessDeal(self, dd):  # dkg.go:272-303
        if dd.Index >= len(self.participants):
            raise ValueError("dkg: dist deal out of bounds index")
        if dd.Index in self.verifiers:
            raise ValueError("dkg: already received dist deal from same index")
        ver = VO.RabinVerifier(self.read, self.long, self.participants[dd.Index], self.participants)
        resp = ver.ProcessEncryptedDeal(dd.Deal)
        _unsafe_set(ver, dd.Index, True)
        self.verifiers[dd.Index] = ver
        return Response(dd.Index, resp)

    def ProcessResponse(self, resp):  # dkg.go:310-342
        v = self.verifiers.get(resp.Index)
        if v is None:
            raise ValueError("dkg: complaint received but no deal for it")
        v.ProcessResponse(resp.Response)
        if resp.Index != self.index:
            return None
        j = self.dealer.ProcessResponse(resp.Response)
        if j is None:
            return None
        v.ProcessJustification(j)
        return Justification(self.index, j)

    def ProcessJustification(self, j):  # dkg.go:346-352
        v = self.verifiers.get(j.Index)
        if v is None:
            raise ValueError("dkg: Justification received but no deal for it")
        v.ProcessJustification(j.Justification)

    def SetTimeout(self):
        for i in sorted(self.verifiers):
            self.verifiers[i].SetTimeout()

    def qual(self):
        return [i for i in sorted(self.verifiers) if self.verifiers[i].DealCertified()]

    QUAL = qual

    def Certified(self):
        return len(self.qual()) >= self.t

    def SecretCommits(self):  # dkg.go:411-429
        if not self.dealer.DealCertified():
            raise ValueError("dkg: can't give SecretCommits if deal not certified")
        sc = SecretCommits(self.index, self.dealer.Commits(), self.dealer.sessionID)
        sc.Signature = self.sign(sc.Hash())
        self.commitments[self.index] = sc.Commitments
        return sc

    def ProcessSecretCommits(self, sc):  # dkg.go:436-478
        if sc.Index >= len(self.participants):
            raise ValueError("dkg: secretcommits received with index out of bounds")
        if sc.Index not in self.qual():
            raise ValueError("dkg: secretcommits from a non QUAL member")
        v = self.verifiers[sc.Index]
        if v.sid != sc.SessionID:
            raise ValueError("dkg: secretcommits received with wrong session id")
        VO.schnorr_verify(self.participants[sc.Index], sc.Hash(), sc.Signature)
        deal = v.Deal()
        if not _check(sc.Commitments, deal.SecShare):
            cc = ComplaintCommits(self.index, sc.Index, deal)
            cc.Signature = self.sign(cc.Hash())
            return cc
        self.commitments[sc.Index] = sc.Commitments
        return None

    def ProcessComplaintCommits(self, cc):  # dkg.go:484-541
        if cc.Index >= len(self.participants):
            raise ValueError("dkg: commitcomplaint with unknown issuer")
        if cc.Index not in self.qual():
            raise ValueError("dkg: complaintcommit from non-qual member")
        VO.schnorr_verify(self.participants[cc.Index], cc.Hash(), cc.Signature)
        v = self.verifiers.get(cc.DealerIndex)
        if v is None:
            raise ValueError("dkg: commitcomplaint linked to unknown verifier")
        try:
            v.VerifyDeal(cc.Deal, False)
        except ValueError as err:
            raise ValueError("dkg: verifying deal: %s" % err)
        if cc.DealerIndex not in self.commitments:
            raise ValueError("dkg: complaint about non received commitments")
        if _check(self.commitments[cc.DealerIndex], cc.Deal.SecShare):
            raise ValueError("dkg: invalid complaint, deal verifying")
        deal = v.Deal()
        if deal is None:
            raise ValueError("dkg: complaint linked to non certified deal")
        del self.commitments[cc.DealerIndex]
        rc = ReconstructCommits(cc.Deal.SessionID, self.index, cc.DealerIndex, deal.SecShare)
        rc.Signature = self.sign(rc.Hash())
        self.pendingReconstruct.setdefault(cc.DealerIndex, []).append(rc)
        return rc

    def ProcessReconstructCommits(self, rs):  # dkg.go:547-596
        if rs.DealerIndex in self.reconstructed:
            return
        if rs.DealerIndex in self.commitments:
            raise ValueError("dkg: commitments not invalidated by any complaints")
        if rs.Index >= len(self.participants):
            raise ValueError("dkg: reconstruct commits with invalid verifier index")
        VO.schnorr_verify(self.participants[rs.Index], rs.Hash(), rs.Signature)
        arr = self.pendingReconstruct.setdefault(rs.DealerIndex, [])
        for r in arr:
            if r.Index == rs.Index:
                return
            if r.SessionID != rs.SessionID:
                raise ValueError("dkg: reconstruct commits invalid session id")
        arr.append(rs)
        if len(arr) >= self.t:
            coeffs = DO.recover_pri_poly([(r.Share.I, r.Share.V) for r in arr], self.t)
            self.commitments[rs.DealerIndex] = [DO.base_mul(c) for c in coeffs]
            self.reconstructed[rs.DealerIndex] = True
            del self.pendingReconstruct[rs.DealerIndex]

    def Finished(self):  # dkg.go:601-615
        q = self.qual()
        return all(i in self.commitments for i in q) and len(q) >= self.t

    def DistKeyShare(self):  # dkg.go:624-664
        if not self.Certified():
            raise ValueError("dkg: distributed key not certified")
        sh, pub = 0, None
        for i in self.qual():
            sh = (sh + self.verifiers[i].Deal().SecShare.V) % L
            if i not in self.commitments:
                raise ValueError("dkg: protocol not finished: %d commitments missing" % i)
            c = self.commitments[i]
            pub = c if pub is None else [O.encode(O.add(O.decode(a), O.decode(b))) for a, b in zip(pub, c)]
        return DistKeyShare(pub, VO.PriShare(self.index, sh))
