"""share/dkg/pedersen (dkg.go, structs.go, status.go), encrypt/ecies and sign/schnorr's Sign restated sequentially in Python
integers over oracle/ed25519.py and tests/_ecies_oracle.py -- no GPU, no engine: the checker of kyber_amd/share/dkg.py,
never the thing shipped, written from the reference's text.  Points are their 32 encoded bytes, scalars Python integers;
every deal is encrypted, decrypted and checked one at a time, in the reference's order.  Random streams are callables
read(n) (the streams of util/blake2xb): ``Reader`` for the secret coefficient, ``Rand`` for the other coefficients and the
ephemeral scalars of ecies, the scheme's own for Sign's nonce.

The reference's DKG tests print no bytes and no Go toolchain is at hand, so no transcript of the Go program is pinned."""
import hashlib
import struct

from kyber_amd.util.blake2xb import pick_int
from oracle import ed25519 as O
from tests import _ecies_oracle as EO

L = O.L
Success, Complaint = 0, 1
InitPhase, DealPhase, ResponsePhase, JustifPhase, FinishPhase = range(5)


class ErrEvicted(Exception):
    result = bundle = None


def le(x):
    return (x % L).to_bytes(32, "little")


def pick(read):
    return pick_int(read)[0]


def base_mul(x):
    return O.mul_base(le(x))


# ------------------------------------------------------------------------------------------------------ sign/schnorr
class Scheme:
    def __init__(self, read):
        self.read = read

    def Sign(self, private, msg):  # schnorr.go:56-82
        k = pick(self.read)
        R, pub = base_mul(k), base_mul(private)
        h = int.from_bytes(hashlib.sha512(R + pub + msg).digest(), "little") % L
        return R + le(k + private * h)

    def Verify(self, public, msg, sig):  # schnorr.go:84-160 (the checks that matter for honest and tampered bundles)
        if len(sig) != 64:
            raise ValueError("schnorr: signature of invalid length")
        R, A, S = O.decode(sig[:32]), O.decode(public), int.from_bytes(sig[32:], "little")
        if R is None or A is None or S >= L or O.is_small_order(R) or O.is_small_order(A):
            raise ValueError("schnorr: invalid signature")
        h = int.from_bytes(hashlib.sha512(sig[:32] + public + msg).digest(), "little") % L
        if O.mul_base(le(S)) != O.encode(O.add(R, O.mul_int(h, A))):
            raise ValueError("schnorr: invalid signature")


# ------------------------------------------------------------------------------------------------------ share/poly
def pri_eval(coeffs, i):
    x, v = i + 1, 0
    for c in reversed(coeffs):
        v = (v * x + c) % L
    return v


def pub_eval(commits, i):
    x, v = i + 1, O.IDENTITY
    for c in reversed(commits):
        v = O.add(O.mul_int(x, v), O.decode(c))
    return O.encode(v)


def _lagrange_at_zero(xs):
    out = {}
    for i in xs:
        num = den = 1
        for j in xs:
            if j != i:
                num = num * (j + 1) % L
                den = den * ((j + 1) - (i + 1)) % L
        out[i] = num * pow(den, L - 2, L) % L
    return out


def recover_secret(shares, t):  # poly.go:182-208 over the first t shares by index
    pts = dict(sorted(shares)[:t])
    if len(pts) < t:
        raise ValueError("share: not enough shares to recover secret")
    lam = _lagrange_at_zero(list(pts))
    return sum(lam[i] * v for i, v in pts.items()) % L


def recover_commit(shares, t):  # poly.go:449-476
    pts = dict(sorted(shares)[:t])
    if len(pts) < t:
        raise ValueError("share: not enough good public shares to reconstruct secret commitment")
    lam = _lagrange_at_zero(list(pts))
    acc = O.IDENTITY
    for i, v in pts.items():
        acc = O.add(acc, O.mul_int(lam[i], O.decode(v)))
    return O.encode(acc)


def recover_pri_poly(shares, t):  # poly.go:260-283: the coefficients of the interpolating polynomial
    pts = dict(sorted(shares)[:t])
    if len(pts) != t:
        raise ValueError("share: not enough shares to recover private polynomial")
    acc = [0] * t
    for j, yj in pts.items():
        basis, den = [1], 1
        for m in pts:
            if m == j:
                continue
            basis = [((basis[k - 1] if k else 0) - (m + 1) * (basis[k] if k < len(basis) else 0)) % L for k in range(len(basis) + 1)]
            den = den * ((j + 1) - (m + 1)) % L
        f = yj * pow(den, L - 2, L) % L
        acc = [(a + f * b) % L for a, b in zip(acc, basis)]
    return acc


# ------------------------------------------------------------------------------------------------------ structs.go
class Node:
    def __init__(self, Index, Public):
        self.Index, self.Public = Index, Public


class DistKeyShare:
    def __init__(self, Commits, Share):
        self.Commits, self.Share = Commits, Share  # Share: (I, V)


class Result:
    def __init__(self, QUAL, Key):
        self.QUAL, self.Key = QUAL, Key


class Deal:
    def __init__(self, ShareIndex, EncryptedShare):
        self.ShareIndex, self.EncryptedShare = ShareIndex, EncryptedShare


class Response:
    def __init__(self, DealerIndex, Status):
        self.DealerIndex, self.Status = DealerIndex, Status


class Justification:
    def __init__(self, ShareIndex, Share):
        self.ShareIndex, self.Share = ShareIndex, Share


def _u32(i):
    return struct.pack(">I", i)


class DealBundle:
    def __init__(self, DealerIndex, Deals, Public, SessionID, Signature=b""):
        self.DealerIndex, self.Deals, self.Public, self.SessionID, self.Signature = DealerIndex, Deals, Public, SessionID, Signature

    def Hash(self):  # structs.go:114-147
        self.Deals = sorted(self.Deals, key=lambda d: d.ShareIndex)
        data = _u32(self.DealerIndex) + b"".join(self.Public or [])
        for d in self.Deals:
            data += _u32(d.ShareIndex) + d.EncryptedShare
        return hashlib.sha256(data + self.SessionID).digest()


class ResponseBundle:
    def __init__(self, ShareIndex, Responses, SessionID, Signature=b""):
        self.ShareIndex, self.Responses, self.SessionID, self.Signature = ShareIndex, Responses, SessionID, Signature

    def Hash(self):  # structs.go:180-207
        self.Responses = sorted(self.Responses, key=lambda r: r.DealerIndex)
        data = _u32(self.ShareIndex)
        for r in self.Responses:
            data += _u32(r.DealerIndex) + bytes([1 if r.Status == Success else 0])
        return hashlib.sha256(data + self.SessionID).digest()


class JustificationBundle:
    def __init__(self, DealerIndex, Justifications, SessionID, Signature=b""):
        self.DealerIndex, self.Justifications, self.SessionID, self.Signature = DealerIndex, Justifications, SessionID, Signature

    def Hash(self):  # structs.go:245-271
        self.Justifications = sorted(self.Justifications, key=lambda j: j.ShareIndex)
        data = _u32(self.DealerIndex)
        for j in self.Justifications:
            data += _u32(j.ShareIndex) + le(j.Share)
        return hashlib.sha256(data + self.SessionID).digest()


def verify_packet(c, p):  # structs.go:293-348
    dealers = c.NewNodes if c.OldNodes is None else c.OldNodes
    nodes, index = (c.NewNodes, p.ShareIndex) if isinstance(p, ResponseBundle) else (dealers, p.DealerIndex)
    pub = [n.Public for n in nodes if n.Index == index]
    if not pub:
        return False
    try:
        c.Auth.Verify(pub[0], p.Hash(), p.Signature)
    except ValueError:
        return False
    return True


# ------------------------------------------------------------------------------------------------------ status.go
class StatusMatrix(dict):
    def __init__(self, dealers, holders, status):
        super().__init__((d.Index, {h.Index: status for h in holders}) for d in dealers)

    def all_true(self, dealer):
        return Complaint not in self[dealer].values()

    def complete(self):
        return all(self.all_true(d) for d in self)


def MinimumT(n):
    return (n >> 1) + 1


class Config:
    def __init__(self, **kw):
        self.Longterm = self.OldNodes = self.PublicCoeffs = self.NewNodes = self.Share = self.Reader = self.Nonce = self.Auth = self.Rand = None
        self.Threshold = self.OldThreshold = 0
        self.FastSync = False
        self.__dict__.update(kw)

    def copy(self):
        return Config(**self.__dict__)

    def CheckForDuplicates(self):  # dkg.go:1189-1208
        for nodes in (self.OldNodes, self.NewNodes):
            idx = [n.Index for n in nodes or []]
            if len(set(idx)) != len(idx):
                raise ValueError("found duplicate in nodes list")


def _find_pub(nodes, pub):
    for n in nodes or []:
        if n.Public == pub:
            return n.Index, True
    return 0, False


def _included(nodes, index):
    return any(n.Index == index for n in nodes or [])


class DistKeyGenerator:
    def sign(self, p):
        return self.c.Auth.Sign(self.c.Longterm, p.Hash())

    def Deals(self):  # dkg.go:356-397
        if not self.canIssue:
            raise ValueError("new members can't issue deals")
        if self.state != InitPhase:
            raise ValueError("dkg not in the initial state")
        deals = []
        for node in self.c.NewNodes:
            si = pri_eval(self.dpriv, node.Index)
            if self.canReceive and self.nidx == node.Index:
                self.validShares[self.oidx] = si
                self.allPublics[self.oidx] = self.dpub
                self.statuses[self.oidx][self.nidx] = Success
                continue
            cipher = EO.encrypt(le(pick(self.c.Rand)), node.Public, le(si))
            if cipher is None:
                raise ValueError("invalid Ed25519 curve point")
            deals.append(Deal(node.Index, cipher))
        self.state = DealPhase
        b = DealBundle(self.oidx, deals, list(self.dpub), self.c.Nonce)
        b.Signature = self.sign(b)
        return b

    def ProcessDeals(self, bundles):  # dkg.go:403-569
        c = self.c
        if self.canIssue and self.state != DealPhase:
            raise ValueError("processdeals can only be called after producing shares")
        if self.canReceive and not self.canIssue and self.state != InitPhase:
            raise ValueError("processdeals can only be called once")
        if not self.canReceive:
            self.state = ResponsePhase
            return None
        seen = set()
        for bundle in bundles:
            if bundle is None:
                continue
            if self.canIssue and bundle.DealerIndex == self.oidx:
                continue
            if not _included(c.OldNodes, bundle.DealerIndex):
                continue
            if bundle.SessionID != c.Nonce:
                self.evicted.append(bundle.DealerIndex)
                continue
            if bundle.Public is None or len(bundle.Public) != c.Threshold:
                self.evicted.append(bundle.DealerIndex)
                continue
            if bundle.DealerIndex in seen:
                self.evicted.append(bundle.DealerIndex)
                continue
            seen.add(bundle.DealerIndex)
            self.allPublics[bundle.DealerIndex] = bundle.Public
            for deal in bundle.Deals:
                if not _included(c.NewNodes, deal.ShareIndex):
                    self.evicted.append(bundle.DealerIndex)
                    break
                if deal.ShareIndex != self.nidx:
                    continue
                buff, st = EO.decrypt(le(self.long) if isinstance(self.long, int) else self.long, deal.EncryptedShare)
                if st != 0 or len(buff) != 32:
                    continue
                if any(O.decode(p) is None for p in bundle.Public) or pub_eval(bundle.Public, self.nidx) != O.mul_base(buff):
                    continue
                if self.isResharing and pub_eval(self.olddpub, bundle.DealerIndex) != bundle.Public[0]:
                    continue
                self.statuses[bundle.DealerIndex][deal.ShareIndex] = Success
                self.validShares[bundle.DealerIndex] = int.from_bytes(buff, "little")
        for dealer in c.OldNodes:
            nidx, found = _find_pub(c.NewNodes, dealer.Public)
            if found:
                self.statuses[dealer.Index][nidx] = Success
        responses = []
        for node in c.OldNodes:
            if node.Index in self.evicted:
                continue
            if self.statuses[node.Index][self.nidx] == Success:
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

    def ProcessResponses(self, bundles):  # dkg.go:581-752
        if not self.canReceive and self.state != DealPhase:
            raise ValueError("phase")
        elif self.state != ResponsePhase:
            raise ValueError("phase")
        out = self._responses(bundles)
        try:
            self.checkIfEvicted(ResponsePhase)
        except ErrEvicted as e:  # Go returns (res, jb, ErrEvicted): the values travel with the error
            e.result, e.bundle = out
            raise
        return out

    def _responses(self, bundles):
        c = self.c
        if not c.FastSync and len(bundles) == 0 and self.canReceive and self.statuses.complete():
            return self.computeResult(), None
        authors, complaint = [], False
        for bundle in bundles:
            if bundle is None or (self.canIssue and bundle.ShareIndex == self.nidx) or not _included(c.NewNodes, bundle.ShareIndex):
                continue
            if bundle.SessionID != c.Nonce:
                self.evictedHolders.append(bundle.ShareIndex)
                continue
            for r in bundle.Responses:
                if not _included(c.OldNodes, r.DealerIndex) or (not c.FastSync and r.Status == Success):
                    self.evictedHolders.append(bundle.ShareIndex)
                    continue
                self.statuses[r.DealerIndex][bundle.ShareIndex] = r.Status
                complaint |= r.Status == Complaint
                authors.append(bundle.ShareIndex)
        if c.FastSync:
            sent = authors + self.evictedHolders
            for n in c.NewNodes:
                if not (self.canReceive and self.nidx == n.Index) and n.Index not in sent:
                    self.evictedHolders.append(n.Index)
        if not complaint and self.statuses.complete():
            self.state = FinishPhase
            return (self.computeResult(), None) if self.canReceive else (None, None)
        for n in c.OldNodes:
            if list(self.statuses[n.Index].values()).count(Complaint) >= c.Threshold:
                self.evicted.append(n.Index)
        self.state = JustifPhase
        if not self.canIssue:
            return None, None
        justs = []
        for idx in sorted(self.statuses[self.oidx]):
            if self.statuses[self.oidx][idx] == Complaint:
                justs.append(Justification(idx, pri_eval(self.dpriv, idx)))
                self.statuses[self.oidx][idx] = Success
        if not justs:
            return None, None
        b = JustificationBundle(self.oidx, justs, c.Nonce)
        b.Signature = self.sign(b)
        return None, b

    def ProcessJustifications(self, bundles):  # dkg.go:759-889
        c = self.c
        if not self.canReceive:
            return None
        if self.state != JustifPhase:
            raise ValueError("phase")
        seen = set()
        for bundle in bundles or []:
            if bundle is None:
                continue
            if bundle.DealerIndex in seen:
                self.evicted.append(bundle.DealerIndex)
                continue
            if (self.canIssue and bundle.DealerIndex == self.oidx) or not _included(c.OldNodes, bundle.DealerIndex) or bundle.DealerIndex in self.evicted:
                continue
            if bundle.SessionID != c.Nonce:
                self.evicted.append(bundle.DealerIndex)
                continue
            seen.add(bundle.DealerIndex)
            for j in bundle.Justifications:
                if not _included(c.NewNodes, j.ShareIndex):
                    self.evicted.append(bundle.DealerIndex)
                    continue
                pub = self.allPublics.get(bundle.DealerIndex)
                if pub is None:
                    self.evicted.append(bundle.DealerIndex)
                    break
                if any(O.decode(p) is None for p in pub) or base_mul(j.Share) != pub_eval(pub, j.ShareIndex):
                    self.evicted.append(bundle.DealerIndex)
                    continue
                if self.isResharing and pub_eval(self.olddpub, bundle.DealerIndex) != pub[0]:
                    self.evicted.append(bundle.DealerIndex)
                    continue
                self.statuses[bundle.DealerIndex][j.ShareIndex] = Success
                if j.ShareIndex == self.nidx:
                    self.validShares[bundle.DealerIndex] = j.Share
        self.checkIfEvicted(JustifPhase)
        good = sum(1 for n in c.OldNodes if n.Index not in self.evicted and self.statuses.all_true(n.Index))
        target = c.OldThreshold if self.isResharing else c.Threshold
        if good < target:
            self.state = FinishPhase
            raise ValueError("process-justifications: only %d/%d valid deals - dkg abort" % (good, target))
        return self.computeResult()

    def computeResult(self):  # dkg.go:891-1071
        c = self.c
        self.state = FinishPhase
        for i in self.evicted:
            for k in self.statuses[i]:
                self.statuses[i][k] = Complaint
        if not self.isResharing:
            share, pub, nodes = 0, None, []
            for n in c.OldNodes:
                if not self.statuses.all_true(n.Index) or n.Index in self.evictedHolders:
                    continue
                share = (share + self.validShares[n.Index]) % L
                p = self.allPublics[n.Index]
                pub = list(p) if pub is None else [O.encode(O.add(O.decode(a), O.decode(b))) for a, b in zip(pub, p)]
                nodes.append(n)
            if pub is None:
                raise ValueError("BUG: final public polynomial is nil")
            return Result(nodes, DistKeyShare(pub, (self.nidx, share)))
        shares, coeffs = [], {}
        for n in c.OldNodes:
            if self.statuses.all_true(n.Index):
                coeffs[n.Index] = self.allPublics[n.Index]
                shares.append((n.Index, self.validShares[n.Index]))
        private = (self.nidx, recover_pri_poly(shares, self.oldT)[0])
        final = [recover_commit([(j, coeffs[j][i]) for j in coeffs], self.oldT) for i in range(self.newT)]
        if pub_eval(final, private[0]) != base_mul(private[1]):
            raise ValueError("dkg: share do not correspond to public polynomial ><")
        qual = [n for n in c.NewNodes
                if not any(not self.statuses.all_true(o.Index) and o.Public == n.Public for o in c.OldNodes) and n.Index not in self.evictedHolders]
        if len(qual) < c.Threshold:
            raise ValueError("dkg: too many uncompliant new participants")
        return Result(qual, DistKeyShare(final, private))

    def checkIfEvicted(self, phase):  # dkg.go:1080-1106
        if self.isResharing and phase == ResponsePhase:
            if not self.canReceive:
                return
            arr, index = self.evictedHolders, self.nidx
        else:
            if not self.canIssue:
                return
            arr, index = self.evicted, self.oidx
        if index in arr:
            raise ErrEvicted()


def NewDistKeyHandler(c):  # dkg.go:218-354
    if not c.NewNodes and not c.OldNodes:
        raise ValueError("dkg: can't run with empty node list")
    if c.Nonce is None or len(c.Nonce) != 32:
        raise ValueError("dkg: invalid nonce length")
    if c.Auth is None:
        raise ValueError("dkg: need authentication scheme")
    resharing = c.Share is not None or c.PublicCoeffs is not None
    if resharing and (not c.OldNodes or c.OldThreshold == 0):
        raise ValueError("dkg: resharing config needs old nodes and old threshold")
    pub = base_mul(c.Longterm)
    oidx, oldPresent = _find_pub(c.OldNodes, pub)
    nidx, newPresent = _find_pub(c.NewNodes, pub)
    if not oldPresent and not newPresent:
        raise ValueError("dkg: public key not found in old list or new list")
    d = DistKeyGenerator()
    d.newT = c.Threshold or MinimumT(len(c.NewNodes))
    d.canReceive, d.canIssue, secret = newPresent, False, None
    if not resharing and newPresent:
        secret = pick(c.Reader)
        c.OldNodes = c.NewNodes
        oidx, oldPresent = _find_pub(c.OldNodes, pub)
        d.canIssue = True
    elif c.Share is not None:
        secret = c.Share.Share[1]
        d.canIssue = True
    c.CheckForDuplicates()
    d.dpriv = [secret if secret is not None else pick(c.Rand)] + [pick(c.Rand) for _ in range(1, c.Threshold)]
    d.dpub = [base_mul(a) for a in d.dpriv]
    d.olddpub, d.oldT = None, 0
    if resharing and newPresent:
        if c.PublicCoeffs is None:
            c.PublicCoeffs = c.Share.Commits
        d.olddpub, d.oldT = c.PublicCoeffs, len(c.PublicCoeffs)
    if c.FastSync:
        d.statuses = StatusMatrix(c.OldNodes, c.NewNodes, Complaint)
    else:
        d.statuses = StatusMatrix(c.OldNodes, c.NewNodes, Success)
        if d.canReceive:
            for n in c.OldNodes:
                d.statuses[n.Index][nidx] = Complaint
    d.state, d.long, d.isResharing, d.oidx, d.nidx, d.c = InitPhase, c.Longterm, resharing, oidx, nidx, c
    d.validShares, d.allPublics, d.evicted, d.evictedHolders = {}, {}, [], []
    return d
