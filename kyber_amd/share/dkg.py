"""Host-side mirror of the reference's ``share/dkg/pedersen`` (dkg.go, structs.go, status.go) on Ed25519, function for
function, over the engine's fused calls: ``Deals()`` draws every ephemeral scalar in the reference's order and makes ONE
seal call (kyb_ed25519_ecies_seal); ``ProcessDeals()`` makes ONE open call for all ciphertexts addressed to this node and
ONE kyb_ed25519_deal_check (plus ONE ``olddpub.EvalMany`` over the dealers' indices when resharing), then applies the
reference's sequential rules on the host in bundle order -- duplicate dealers, evictions, the ``break`` on a foreign share
index, the skip of our own bundle; ``ProcessJustifications()`` makes ONE deal_check over all justifications.  The final
``PubPoly`` sum stays on ``PubPoly.Add``.  ``protocol.go`` (the board, the phaser, timeouts) is networking and not here.

Where the reference draws from ``crypto/rand`` or the suite's RandomStream, ``Config`` carries the streams: ``Reader`` for
the secret coefficient (dkg.go:272-279), ``Rand`` for the other coefficients (dkg.go:293) and the ephemeral scalars of the
deals (ecies.go:29); each is what ``Scalar.Pick`` takes, None for the operating system's randomness.
"""
from __future__ import annotations

import hashlib
import os
import struct

from ..encrypt import ecies
from ..group import edwards25519 as ed
from ..sign import schnorr
from . import poly as share

Success, Complaint = 0, 1  # status.go:13-16
InitPhase, DealPhase, ResponsePhase, JustifPhase, FinishPhase = range(5)  # dkg.go:124-130
NonceLength = 32


class ErrEvicted(Exception):
    """dkg.go:1073: our node is evicted from the list of qualified participants"""

    result = bundle = None


class Node:  # structs.go:26-33
    def __init__(self, Index: int, Public):
        self.Index, self.Public = Index, Public

    def Equal(self, n2) -> bool:
        return self.Index == n2.Index and self.Public.Equal(n2.Public)


class DistKeyShare:  # structs.go:65-87
    def __init__(self, Commits, Share):
        self.Commits, self.Share = Commits, Share

    def Public(self):
        return self.Commits[0]

    def PriShare(self):
        return self.Share

    def Commitments(self):
        return self.Commits


class Result:  # structs.go:38-62
    def __init__(self, QUAL, Key):
        self.QUAL, self.Key = QUAL, Key

    def PublicEqual(self, r2) -> bool:
        if len(self.Key.Commits) != len(r2.Key.Commits) or len(self.QUAL) != len(r2.QUAL):
            return False
        return all(a.Equal(b) for a, b in zip(self.Key.Commits, r2.Key.Commits)) and all(a.Equal(b) for a, b in zip(self.QUAL, r2.QUAL))


class Deal:  # structs.go:91-96
    def __init__(self, ShareIndex: int, EncryptedShare: bytes):
        self.ShareIndex, self.EncryptedShare = ShareIndex, EncryptedShare


class Response:  # structs.go:159-163
    def __init__(self, DealerIndex: int, Status: int):
        self.DealerIndex, self.Status = DealerIndex, Status


class Justification:  # structs.go:240-243
    def __init__(self, ShareIndex: int, Share):
        self.ShareIndex, self.Share = ShareIndex, Share


def _u32(i: int) -> bytes:
    return struct.pack(">I", i)


class DealBundle:  # structs.go:102-155
    def __init__(self, DealerIndex, Deals, Public, SessionID, Signature=b""):
        self.DealerIndex, self.Deals, self.Public, self.SessionID, self.Signature = DealerIndex, Deals, Public, SessionID, Signature

    def Hash(self) -> bytes:
        self.Deals.sort(key=lambda d: d.ShareIndex)  # (stable)
        h = hashlib.sha256(_u32(self.DealerIndex))
        for c in self.Public or []:
            h.update(c.MarshalBinary())
        for d in self.Deals:
            h.update(_u32(d.ShareIndex) + bytes(d.EncryptedShare))
        h.update(bytes(self.SessionID))
        return h.digest()

    def Index(self):
        return self.DealerIndex

    def Sig(self):
        return self.Signature


class ResponseBundle:  # structs.go:169-225
    def __init__(self, ShareIndex, Responses, SessionID, Signature=b""):
        self.ShareIndex, self.Responses, self.SessionID, self.Signature = ShareIndex, Responses, SessionID, Signature

    def Hash(self) -> bytes:
        self.Responses.sort(key=lambda r: r.DealerIndex)
        h = hashlib.sha256(_u32(self.ShareIndex))
        for r in self.Responses:
            h.update(_u32(r.DealerIndex) + (b"\x01" if r.Status == Success else b"\x00"))
        h.update(bytes(self.SessionID))
        return h.digest()

    def Index(self):
        return self.ShareIndex

    def Sig(self):
        return self.Signature


class JustificationBundle:  # structs.go:231-279
    def __init__(self, DealerIndex, Justifications, SessionID, Signature=b""):
        self.DealerIndex, self.Justifications, self.SessionID, self.Signature = DealerIndex, Justifications, SessionID, Signature

    def Hash(self) -> bytes:
        self.Justifications.sort(key=lambda j: j.ShareIndex)
        h = hashlib.sha256(_u32(self.DealerIndex))
        for j in self.Justifications:
            h.update(_u32(j.ShareIndex) + j.Share.MarshalBinary())
        h.update(bytes(self.SessionID))
        return h.digest()

    def Index(self):
        return self.DealerIndex

    def Sig(self):
        return self.Signature


class BitSet(dict):  # status.go:18, 118-126
    def LengthComplaints(self) -> int:
        return sum(1 for s in self.values() if s == Complaint)


class StatusMatrix(dict):  # status.go:19-82
    def __init__(self, dealers, shareHolders, status):
        super().__init__((d.Index, BitSet((h.Index, status) for h in shareHolders)) for d in dealers)

    def StatusesForShare(self, shareIndex) -> BitSet:
        return BitSet((d, bs[shareIndex]) for d, bs in self.items())

    def StatusesOfDealer(self, dealerIndex) -> BitSet:
        return self[dealerIndex]

    def Set(self, dealer, share_, status):
        self[dealer][share_] = status

    def SetAll(self, dealer, status):
        for s in self[dealer]:
            self[dealer][s] = status

    def AllTrue(self, dealer) -> bool:
        return all(s != Complaint for s in self[dealer].values())

    def CompleteSuccess(self) -> bool:
        return all(self.AllTrue(d) for d in self)

    def Get(self, dealer, share_):
        return self[dealer][share_]


def MinimumT(n: int) -> int:  # dkg.go:1126-1128
    return (n >> 1) + 1


def GetNonce() -> bytes:  # dkg.go:1143-1153
    return os.urandom(NonceLength)


def findPub(nodes, toFind):  # dkg.go:1108-1115
    for n in nodes or []:
        if n.Public.Equal(toFind):
            return n.Index, True
    return 0, False


def findIndex(nodes, index):  # dkg.go:1117-1124
    for n in nodes or []:
        if n.Index == index:
            return n.Public, True
    return None, False


def isIndexIncluded(nodes, index) -> bool:  # dkg.go:1130-1137
    return any(n.Index == index for n in nodes or [])


class Config:  # dkg.go:35-119
    def __init__(self, Suite=None, Longterm=None, OldNodes=None, PublicCoeffs=None, NewNodes=None, Share=None, Threshold=0,
                 OldThreshold=0, Reader=None, UserReaderOnly=False, FastSync=False, Nonce=None, Auth=None, Log=None, Rand=None):
        self.Suite, self.Longterm, self.OldNodes, self.PublicCoeffs, self.NewNodes = Suite, Longterm, OldNodes, PublicCoeffs, NewNodes
        self.Share, self.Threshold, self.OldThreshold, self.Reader, self.UserReaderOnly = Share, Threshold, OldThreshold, Reader, UserReaderOnly
        self.FastSync, self.Nonce, self.Auth, self.Log, self.Rand = FastSync, Nonce, Auth, Log, Rand

    def copy(self) -> "Config":
        c = Config()
        c.__dict__.update(self.__dict__)
        return c

    def CheckForDuplicates(self) -> None:  # dkg.go:1189-1208
        for what, nodes in (("old", self.OldNodes), ("new", self.NewNodes)):
            seen = set()
            for n in nodes or []:
                if n.Index in seen:
                    raise ValueError(f"found duplicate in {what} nodes list: index {n.Index}")
                seen.add(n.Index)

    def Info(self, *kv):
        if self.Log is not None:
            self.Log.Info("dkg-log", kv)

    def Error(self, *kv):
        if self.Log is not None:
            self.Log.Error("dkg-log", kv)


def VerifyPacketSignature(c: Config, p) -> None:  # structs.go:293-348
    """raises ValueError unless the packet carries its author's signature"""
    if not verify_packets(c, [p])[0]:
        raise ValueError("invalid signature")


def verify_packets(c: Config, packets) -> list:
    """[VerifyPacketSignature(c, p) == nil for p in packets] with ONE batch_verify_with_checks over the list (what the
    engine adds: the reference verifies packet by packet)"""
    dealers = c.NewNodes if c.OldNodes is None else c.OldNodes
    ok = [False] * len(packets)
    rows = []
    for i, p in enumerate(packets):
        if isinstance(p, ResponseBundle):
            pub, found = findIndex(c.NewNodes, p.ShareIndex)
        elif isinstance(p, (DealBundle, JustificationBundle)):
            pub, found = findIndex(dealers, p.DealerIndex)
        else:
            raise TypeError("unknown packet type")
        if found:
            rows.append((i, pub.MarshalBinary(), p.Hash(), bytes(p.Signature)))
    if rows:
        good = schnorr.batch_verify_with_checks([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
        for (i, _, _, _), g in zip(rows, good):
            ok[i] = bool(g)
    return ok


class DistKeyGenerator:  # dkg.go:175-214
    def sign(self, p) -> bytes:  # dkg.go:1155-1163
        return self.c.Auth.Sign(self.c.Longterm, p.Hash())

    # ------------------------------------------------------------------------------------------------ dkg.go:356-397
    def Deals(self) -> DealBundle:
        if not self.canIssue:
            raise ValueError("new members can't issue deals")
        if self.state != InitPhase:
            raise ValueError("dkg not in the initial state, can't produce deals: %d" % self.state)
        c = self.c
        to, pubs, msgs, r = [], [], [], []
        idx = [node.Index for node in c.NewNodes]  # the n evaluations: one launch from PriPoly's device threshold on
        evals = self.dpriv.EvalMany(idx) if len(idx) >= share.PriPoly.DEVICE_MIN else [self.dpriv.Eval(i) for i in idx]
        for node, sh in zip(c.NewNodes, evals):
            si = sh.V
            if self.canReceive and self.nidx == node.Index:
                self.validShares[self.oidx] = si
                self.allPublics[self.oidx] = self.dpub
                self.statuses.Set(self.oidx, self.nidx, Success)
                continue
            to.append(node.Index)
            pubs.append(node.Public)
            msgs.append(si.MarshalBinary())
            r.append(c.Suite.Scalar().Pick(c.Rand))  # ecies.go:29, in the reference's order of draws
        ctx = ecies.EncryptBatch(c.Suite, pubs, msgs, hashlib.sha256, r=r) if to else []  # ONE seal call
        self.state = DealPhase
        bundle = DealBundle(self.oidx, [Deal(i, x) for i, x in zip(to, ctx)], list(self.dpub.commits), c.Nonce)
        bundle.Signature = self.sign(bundle)
        return bundle

    # ------------------------------------------------------------------------------------------------ dkg.go:403-569
    def ProcessDeals(self, bundles):
        c = self.c
        if self.canIssue and self.state != DealPhase:
            raise ValueError("processdeals can only be called after producing shares")
        if self.canReceive and not self.canIssue and self.state != InitPhase:
            raise ValueError("processdeals can only be called once after creating the dkg for a new member")
        if not self.canReceive:
            self.state = ResponsePhase
            return None

        # the bundles whose deals the sequential loop below will look at, by the reference's rules up to "seenIndex"
        def looked_at(b):
            return not (b is None or (self.canIssue and b.DealerIndex == self.oidx) or not isIndexIncluded(c.OldNodes, b.DealerIndex)
                        or bytes(b.SessionID) != bytes(c.Nonce) or b.Public is None or len(b.Public) != c.Threshold)

        mine = []  # (bundle position, deal position) of every ciphertext addressed to this node that the loop can reach
        for bi, b in enumerate(bundles):
            if not looked_at(b):
                continue
            for di, deal in enumerate(b.Deals):
                if not isIndexIncluded(c.NewNodes, deal.ShareIndex):
                    break
                if deal.ShareIndex == self.nidx:
                    mine.append((bi, di))
        plain, status = ecies.DecryptBatch(c.Suite, self.long, [bundles[bi].Deals[di].EncryptedShare for bi, di in mine],
                                           hashlib.sha256) if mine else ([], [])  # ONE open call
        shares, checked = {}, []
        for k, pos in enumerate(mine):
            if status[k] == 0 and len(plain[k]) == 32:
                shares[pos] = c.Suite.Scalar().UnmarshalBinary(plain[k])
                checked.append(pos)
        polys = {bi: share.PubPoly(c.Suite, None, bundles[bi].Public) for bi in {bi for bi, _ in checked}}
        good = dict(zip(checked, _check_shares([polys[bi] for bi, _ in checked],
                                               [share.PriShare(self.nidx, shares[p]) for p in checked])))  # ONE deal_check
        old = {}
        if self.isResharing and checked:  # ONE EvalMany over the dealers' indices
            dealers = sorted({bundles[bi].DealerIndex for bi, _ in checked})
            old = {s.I: s.V for s in self.olddpub.EvalMany(dealers)}

        seenIndex = set()
        for bi, bundle in enumerate(bundles):
            if bundle is None:
                c.Error("found nil Deal bundle")
                continue
            if self.canIssue and bundle.DealerIndex == self.oidx:
                continue
            if not isIndexIncluded(c.OldNodes, bundle.DealerIndex):
                c.Error("dealer %d not in OldNodes" % bundle.DealerIndex)
                continue
            if bytes(bundle.SessionID) != bytes(c.Nonce):
                self.evicted.append(bundle.DealerIndex)
                c.Error("Deal with invalid session ID")
                continue
            if bundle.Public is None or len(bundle.Public) != c.Threshold:
                self.evicted.append(bundle.DealerIndex)
                c.Error("Deal with nil public key or invalid threshold")
                continue
            if bundle.DealerIndex in seenIndex:
                self.evicted.append(bundle.DealerIndex)
                c.Error("Deal bundle already seen")
                continue
            seenIndex.add(bundle.DealerIndex)
            self.allPublics[bundle.DealerIndex] = share.PubPoly(c.Suite, None, bundle.Public)
            for di, deal in enumerate(bundle.Deals):
                if not isIndexIncluded(c.NewNodes, deal.ShareIndex):
                    self.evicted.append(bundle.DealerIndex)
                    c.Error("Deal share holder evicted normally")
                    break
                if deal.ShareIndex != self.nidx:
                    continue
                if not good.get((bi, di), False):  # decryption, unmarshalling or the check against the public polynomial
                    c.Error("Deal share invalid")
                    continue
                if self.isResharing and not old[bundle.DealerIndex].Equal(bundle.Public[0]):
                    continue
                self.statuses.Set(bundle.DealerIndex, deal.ShareIndex, Success)
                self.validShares[bundle.DealerIndex] = shares[(bi, di)]

        for dealer in c.OldNodes:
            nidx, found = findPub(c.NewNodes, dealer.Public)
            if found:
                self.statuses.Set(dealer.Index, nidx, Success)
        responses = []
        myshares = self.statuses.StatusesForShare(self.nidx)
        for node in c.OldNodes:
            if node.Index in self.evicted:
                continue
            if myshares[node.Index] == Success:
                if c.FastSync:
                    responses.append(Response(node.Index, Success))
            else:
                responses.append(Response(node.Index, Complaint))
        bundle = None
        if responses:
            bundle = ResponseBundle(self.nidx, responses, c.Nonce)
            bundle.Signature = self.sign(bundle)
        self.state = ResponsePhase
        return bundle

    def ExpectedResponsesFastSync(self) -> int:  # dkg.go:571-573
        return len(self.c.NewNodes)

    # ------------------------------------------------------------------------------------------------ dkg.go:581-752
    def ProcessResponses(self, bundles):
        """(result, justification bundle); raises ErrEvicted where the reference returns it, the pair it returns next to
        the error as the exception's ``result`` and ``bundle``"""
        c = self.c
        if not self.canReceive and self.state != DealPhase:
            raise ValueError("leaving node can only process responses after creating shares")
        elif self.state != ResponsePhase:
            raise ValueError("can only process responses after processing shares")
        res = self._process_responses(bundles)
        try:
            self.checkIfEvicted(ResponsePhase)
        except ErrEvicted as e:  # the reference returns the result and the bundle next to the error
            e.result, e.bundle = res
            raise
        return res

    def _process_responses(self, bundles):
        c = self.c
        if not c.FastSync and len(bundles) == 0 and self.canReceive and self.statuses.CompleteSuccess():
            return self.computeResult(), None
        validAuthors, foundComplaint = [], False
        for bundle in bundles:
            if bundle is None:
                continue
            if self.canIssue and bundle.ShareIndex == self.nidx:
                continue
            if not isIndexIncluded(c.NewNodes, bundle.ShareIndex):
                continue
            if bytes(bundle.SessionID) != bytes(c.Nonce):
                self.evictedHolders.append(bundle.ShareIndex)
                continue
            for response in bundle.Responses:
                if not isIndexIncluded(c.OldNodes, response.DealerIndex):
                    self.evictedHolders.append(bundle.ShareIndex)
                    continue
                if not c.FastSync and response.Status == Success:
                    self.evictedHolders.append(bundle.ShareIndex)
                    continue
                self.statuses.Set(response.DealerIndex, bundle.ShareIndex, response.Status)
                if response.Status == Complaint:
                    foundComplaint = True
                validAuthors.append(bundle.ShareIndex)
        if c.FastSync:
            allSent = validAuthors + self.evictedHolders
            for n in c.NewNodes:
                if self.canReceive and self.nidx == n.Index:
                    continue
                if n.Index not in allSent:
                    self.evictedHolders.append(n.Index)
        if not foundComplaint and self.statuses.CompleteSuccess():
            self.state = FinishPhase
            return (self.computeResult(), None) if self.canReceive else (None, None)
        for n in c.OldNodes:
            if self.statuses.StatusesOfDealer(n.Index).LengthComplaints() >= c.Threshold:
                self.evicted.append(n.Index)
        self.state = JustifPhase
        if not self.canIssue:
            return None, None
        justifications = []
        for shareIndex, status in sorted(self.statuses.StatusesOfDealer(self.oidx).items()):
            if status != Complaint:
                continue
            justifications.append(Justification(shareIndex, self.dpriv.Eval(shareIndex).V))
            self.statuses.Set(self.oidx, shareIndex, Success)
        if not justifications:
            return None, None
        bundle = JustificationBundle(self.oidx, justifications, c.Nonce)
        bundle.Signature = self.sign(bundle)
        return None, bundle

    # ------------------------------------------------------------------------------------------------ dkg.go:759-889
    def ProcessJustifications(self, bundles):
        c = self.c
        if not self.canReceive:
            return None
        if self.state != JustifPhase:
            raise ValueError("node can only process justifications after processing responses")
        bundles = list(bundles or [])
        # every justification of a dealer whose public polynomial we hold, checked in ONE deal_check
        todo = [(bi, ji) for bi, b in enumerate(bundles) if b is not None and b.DealerIndex in self.allPublics
                for ji, j in enumerate(b.Justifications) if 0 <= j.ShareIndex < 2**32]
        good = dict(zip(todo, _check_shares([self.allPublics[bundles[bi].DealerIndex] for bi, _ in todo],
                                            [share.PriShare(bundles[bi].Justifications[ji].ShareIndex, bundles[bi].Justifications[ji].Share)
                                             for bi, ji in todo])))
        old = {}
        if self.isResharing and todo:
            dealers = sorted({bundles[bi].DealerIndex for bi, _ in todo})
            old = {s.I: s.V for s in self.olddpub.EvalMany(dealers)}
        seen = set()
        for bi, bundle in enumerate(bundles):
            if bundle is None:
                continue
            if bundle.DealerIndex in seen:
                self.evicted.append(bundle.DealerIndex)
                continue
            if self.canIssue and bundle.DealerIndex == self.oidx:
                continue
            if not isIndexIncluded(c.OldNodes, bundle.DealerIndex):
                continue
            if bundle.DealerIndex in self.evicted:
                continue
            if bytes(bundle.SessionID) != bytes(c.Nonce):
                self.evicted.append(bundle.DealerIndex)
                continue
            seen.add(bundle.DealerIndex)
            for ji, justif in enumerate(bundle.Justifications):
                if not isIndexIncluded(c.NewNodes, justif.ShareIndex):
                    self.evicted.append(bundle.DealerIndex)
                    continue
                pubPoly = self.allPublics.get(bundle.DealerIndex)
                if pubPoly is None:
                    self.evicted.append(bundle.DealerIndex)
                    break
                if not good[(bi, ji)]:
                    self.evicted.append(bundle.DealerIndex)
                    continue
                if self.isResharing and not old[bundle.DealerIndex].Equal(pubPoly.Commit()):
                    self.evicted.append(bundle.DealerIndex)
                    continue
                self.statuses.Set(bundle.DealerIndex, justif.ShareIndex, Success)
                if justif.ShareIndex == self.nidx:
                    self.validShares[bundle.DealerIndex] = justif.Share
        self.checkIfEvicted(JustifPhase)
        allGood = sum(1 for n in c.OldNodes if n.Index not in self.evicted and self.statuses.AllTrue(n.Index))
        target = c.OldThreshold if self.isResharing else c.Threshold
        if allGood < target:
            self.state = FinishPhase
            raise ValueError("process-justifications: only %d/%d valid deals - dkg abort" % (allGood, target))
        return self.computeResult()

    # ------------------------------------------------------------------------------------------------ dkg.go:891-1071
    def computeResult(self) -> Result:
        self.state = FinishPhase
        for index in self.evicted:
            self.statuses.SetAll(index, Complaint)
        return self.computeResharingResult() if self.isResharing else self.computeDKGResult()

    def computeResharingResult(self) -> Result:
        c, g = self.c, self.suite
        shares, coeffs = [], {}
        for n in c.OldNodes:
            if not self.statuses.AllTrue(n.Index):
                continue
            if n.Index not in self.allPublics:
                raise ValueError("BUG: nidx %d: public polynomial not found from dealer %d" % (self.nidx, n.Index))
            coeffs[n.Index] = self.allPublics[n.Index].commits
            if n.Index not in self.validShares:
                raise ValueError("BUG: nidx %d private share not found from dealer %d" % (self.nidx, n.Index))
            shares.append(share.PriShare(n.Index, self.validShares[n.Index]))
        priPoly = share.recover_pri_poly(g, shares, self.oldT, len(c.OldNodes))
        privateShare = share.PriShare(self.nidx, priPoly.coeffs[0])
        finalCoeffs = []
        for i in range(self.newT):
            tmp = [share.PubShare(j, coeffs[j][i]) for j in sorted(coeffs)]
            finalCoeffs.append(share.recover_commit(g, tmp, self.oldT, len(c.OldNodes)))
        pubPoly = share.PubPoly(g, None, finalCoeffs)
        if not pubPoly.Check(privateShare):
            raise ValueError("dkg: share do not correspond to public polynomial ><")
        qual = []
        for newNode in c.NewNodes:
            invalid = any(not self.statuses.AllTrue(o.Index) and o.Public.Equal(newNode.Public) for o in c.OldNodes)
            if not invalid and newNode.Index not in self.evictedHolders:
                qual.append(newNode)
        if len(qual) < c.Threshold:
            raise ValueError("dkg: too many uncompliant new participants %d/%d" % (len(qual), c.Threshold))
        return Result(qual, DistKeyShare(finalCoeffs, privateShare))

    def computeDKGResult(self) -> Result:
        c = self.c
        finalShare, finalPub, nodes = c.Suite.Scalar().Zero(), None, []
        for n in c.OldNodes:
            if not self.statuses.AllTrue(n.Index) or n.Index in self.evictedHolders:
                continue
            if n.Index not in self.validShares:
                raise ValueError("BUG: private share not found from dealer %d" % n.Index)
            if n.Index not in self.allPublics:
                raise ValueError("BUG: idx %d public polynomial not found from dealer %d" % (self.nidx, n.Index))
            finalShare = c.Suite.Scalar().Add(finalShare, self.validShares[n.Index])
            pub = self.allPublics[n.Index]
            finalPub = pub if finalPub is None else finalPub.Add(pub)
            nodes.append(n)
        if finalPub is None:
            raise ValueError("BUG: final public polynomial is nil")
        return Result(nodes, DistKeyShare(list(finalPub.commits), share.PriShare(self.nidx, finalShare)))

    def checkIfEvicted(self, phase) -> None:  # dkg.go:1080-1106
        if self.isResharing and phase == ResponsePhase:
            if not self.canReceive:
                return
            arr, index = self.evictedHolders, self.nidx
        else:
            if not self.canIssue:
                return
            arr, index = self.evicted, self.oidx
        if index in arr:
            raise ErrEvicted("our node is evicted from list of qualified participants")


def _check_shares(pub_polys, pri_shares) -> list:
    """share.check_shares, with a polynomial whose commitment does not decode failing its own checks only"""
    if not pub_polys:
        return []
    t = pub_polys[0].Threshold()
    n = len(pub_polys)
    commits = b"".join(c.MarshalBinary() for p in pub_polys for c in p.commits)
    ok, _ = ed.batch_deal_check(list(range(n)), [s.I for s in pri_shares], b"".join(ed._sc(s.V).v for s in pri_shares), commits, n, t)
    return [bool(v) for v in ok]


def NewDistKeyHandler(c: Config) -> DistKeyGenerator:  # dkg.go:218-354
    if not c.NewNodes and not c.OldNodes:
        raise ValueError("dkg: can't run with empty node list")
    if c.Nonce is None or len(c.Nonce) != NonceLength:
        raise ValueError("dkg: invalid nonce length")
    if c.Auth is None:
        raise ValueError("dkg: need authentication scheme")
    isResharing = c.Share is not None or c.PublicCoeffs is not None
    if isResharing:
        if not c.OldNodes:
            raise ValueError("dkg: resharing config needs old nodes list")
        if c.OldThreshold == 0:
            raise ValueError("dkg: resharing case needs old threshold field")
    canReceive = True
    pub = c.Suite.Point().Mul(c.Longterm, None)
    oidx, oldPresent = findPub(c.OldNodes, pub)
    nidx, newPresent = findPub(c.NewNodes, pub)
    if not oldPresent and not newPresent:
        raise ValueError("dkg: public key not found in old list or new list")
    newThreshold = c.Threshold if c.Threshold != 0 else MinimumT(len(c.NewNodes))
    if not newPresent:
        canReceive = False
    canIssue, secretCoeff, olddpub, oldThreshold = False, None, None, 0
    if not isResharing and newPresent:
        secretCoeff = c.Suite.Scalar().Pick(c.Reader)
        c.OldNodes = c.NewNodes
        oidx, oldPresent = findPub(c.OldNodes, pub)
        canIssue = True
    elif c.Share is not None:
        secretCoeff = c.Share.Share.V
        canIssue = True
    c.CheckForDuplicates()
    # share.NewPriPoly(suite, c.Threshold, secretCoeff, RandomStream): the secret (drawn if nil), then t - 1 coefficients
    coeffs = [secretCoeff if secretCoeff is not None else c.Suite.Scalar().Pick(c.Rand)]
    coeffs += [c.Suite.Scalar().Pick(c.Rand) for _ in range(1, c.Threshold)]
    dpriv = share.PriPoly(c.Suite, coeffs)
    dpub = dpriv.Commit()
    if isResharing and newPresent:
        if c.PublicCoeffs is None:
            c.PublicCoeffs = c.Share.Commits
        olddpub = share.PubPoly(c.Suite, None, c.PublicCoeffs)
        canReceive = True
        oldThreshold = len(c.PublicCoeffs)
    if c.FastSync:
        statuses = StatusMatrix(c.OldNodes, c.NewNodes, Complaint)
    else:
        statuses = StatusMatrix(c.OldNodes, c.NewNodes, Success)
        if canReceive:
            for node in c.OldNodes:
                statuses.Set(node.Index, nidx, Complaint)
    d = DistKeyGenerator()
    d.state, d.suite, d.long, d.pub, d.canReceive, d.canIssue, d.isResharing = InitPhase, c.Suite, c.Longterm, pub, canReceive, canIssue, isResharing
    d.dpriv, d.dpub, d.olddpub, d.oidx, d.nidx, d.c, d.oldT, d.newT = dpriv, dpub, olddpub, oidx, nidx, c, oldThreshold, newThreshold
    d.newPresent, d.oldPresent, d.statuses, d.validShares, d.allPublics, d.evicted, d.evictedHolders = newPresent, oldPresent, statuses, {}, {}, [], []
    return d
