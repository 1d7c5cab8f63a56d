"""The reference's DKG scenarios (dkg_test.go, dkg_vartime_test.go) written once over a small kit, so that the same
scenario drives the sequential oracle (tests/_dkg_oracle.py) and the product (kyber_amd/share/dkg.py) under the same
random streams.  A scenario returns its transcript -- every bundle as bytes (with its Hash() and signature), every
node's eviction lists and statuses, every result -- which the host and GPU tests compare between the two, and it checks
testResults' property (dkg_test.go:104-139) on the results in integers."""
import hashlib

from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests import _dkg_oracle as DO

L = O.L


class OracleKit:
    impl = DO

    def scalar(self, x):
        return x

    def point(self, b):
        return b

    def pt(self, p):
        return p

    def sc(self, s):
        return DO.le(s)

    def stream(self, tag):
        return blake2xb.New(tag).Read

    def auth(self, tag):
        return DO.Scheme(blake2xb.New(tag).Read)

    def config(self, **kw):
        return DO.Config(**kw)

    def share(self, res):
        return res.Key.Share[0], res.Key.Share[1]

    def statuses(self, d):
        return {k: dict(v) for k, v in d.statuses.items()}


class ProductKit:
    def __init__(self):
        from kyber_amd.group import edwards25519 as ed
        from kyber_amd.share import dkg
        from kyber_amd.sign import schnorr

        self.impl, self.ed, self.schnorr, self.suite = dkg, ed, schnorr, ed.NewSuite()

    def scalar(self, x):
        return self.ed.Scalar(DO.le(x))

    def point(self, b):
        return self.ed.Point(b)

    def pt(self, p):
        return p.MarshalBinary()

    def sc(self, s):
        return s.MarshalBinary()

    def stream(self, tag):
        return blake2xb.New(tag)

    def auth(self, tag):
        return self.schnorr.NewScheme(self.suite, rand=blake2xb.New(tag))

    def config(self, **kw):
        return self.impl.Config(Suite=self.suite, **kw)

    def share(self, res):
        return res.Key.Share.I, int.from_bytes(res.Key.Share.V.MarshalBinary(), "little")

    def statuses(self, d):
        return {k: dict(v) for k, v in d.statuses.items()}


class TestNode:
    def __init__(self, kit, name, index):
        self.Index = index
        self.priv_int = int.from_bytes(hashlib.sha512(b"dkg node " + name).digest(), "little") % L
        self.Private, self.Public = kit.scalar(self.priv_int), kit.point(O.mul_base(DO.le(self.priv_int)))
        self.dkg = self.res = None


def nodes(kit, tag, n, first=0):
    return [TestNode(kit, tag + b" %d" % (first + i), first + i) for i in range(n)]


def node_list(kit, tns):
    return [kit.impl.Node(t.Index, t.Public) for t in tns]


def setup(kit, tag, tns, conf, coeffs=None):
    nonce = hashlib.sha256(b"nonce " + tag).digest()
    for t in tns:
        c = conf.copy()
        c.Longterm, c.Nonce = t.Private, nonce
        who = tag + b" node %d" % t.Index
        c.Reader, c.Rand, c.Auth = kit.stream(b"reader " + who), kit.stream(b"rand " + who), kit.auth(b"auth " + who)
        if coeffs is not None:
            if t.res is not None:
                c.Share = t.res.Key
            else:
                c.PublicCoeffs = coeffs
        t.dkg = kit.impl.NewDistKeyHandler(c)


class Transcript(list):
    def __init__(self, kit):
        super().__init__()
        self.kit = kit

    def bundle(self, b):
        if b is None:
            return self.append(None)
        k, h = self.kit, b.Hash()  # (Hash() sorts the bundle's entries first)
        if hasattr(b, "Deals"):
            body = (b.DealerIndex, [(d.ShareIndex, bytes(d.EncryptedShare)) for d in b.Deals], [k.pt(p) for p in b.Public])
        elif hasattr(b, "Responses"):
            body = (b.ShareIndex, [(r.DealerIndex, r.Status) for r in b.Responses])
        else:
            body = (b.DealerIndex, [(j.ShareIndex, k.sc(j.Share)) for j in b.Justifications])
        self.append((type(b).__name__, body, bytes(b.SessionID), h, bytes(b.Signature)))

    def node(self, t):
        d = t.dkg
        self.append(("node", t.Index, list(d.evicted), list(d.evictedHolders), self.kit.statuses(d), d.state))

    def result(self, res):
        k = self.kit
        self.append(None if res is None else ("result", [(n.Index, k.pt(n.Public)) for n in res.QUAL],
                                              [k.pt(p) for p in res.Key.Commits], k.share(res)))


def check_results(kit, thr, results):
    """testResults (dkg_test.go:104-139): every result holds the same thr commits and the same QUAL; every share is the
    public polynomial's evaluation; any thr shares interpolate to the secret whose commitment is Commits[0]"""
    assert results
    commits = [kit.pt(p) for p in results[0].Key.Commits]
    assert len(commits) == thr
    qual = [(n.Index, kit.pt(n.Public)) for n in results[0].QUAL]
    shares = []
    for r in results:
        assert [kit.pt(p) for p in r.Key.Commits] == commits and [(n.Index, kit.pt(n.Public)) for n in r.QUAL] == qual
        i, v = kit.share(r)
        assert DO.pub_eval(commits, i) == DO.base_mul(v)
        shares.append((i, v))
    assert len(shares) >= thr
    for rot in range(len(shares) - thr + 1):
        assert DO.base_mul(DO.recover_secret(shares[rot:rot + thr], thr)) == commits[0]
    assert [DO.base_mul(a) for a in DO.recover_pri_poly(shares, thr)] == commits


def run_dkg(kit, tr, tag, tns, conf, dm=None, rm=None, jm=None):
    """RunDKG (dkg_test.go:145-206)"""
    I = kit.impl
    setup(kit, tag, tns, conf)
    deals = [t.dkg.Deals() for t in tns]
    for b in deals:
        tr.bundle(b)
    if dm:
        deals = dm(deals)
    resps = []
    for t in tns:
        r = t.dkg.ProcessDeals(deals)
        tr.bundle(r)
        if r is not None:
            resps.append(r)
    if rm:
        resps = rm(resps)
    justifs, results = [], []
    for t in tns:
        try:
            res, just = t.dkg.ProcessResponses(resps)
        except I.ErrEvicted as e:  # (RunDKG keeps what came back next to the error)
            res, just = e.result, e.bundle
            tr.append(("evicted", t.Index))
        tr.node(t)
        tr.bundle(just)
        if res is not None:
            results.append(res)
        elif just is not None:
            justifs.append(just)
    if justifs:
        if jm:
            justifs = jm(justifs)
        for t in tns:
            try:
                res = t.dkg.ProcessJustifications(justifs)
            except I.ErrEvicted:
                tr.append(("evicted", t.Index))
                continue
            tr.node(t)
            assert res is not None
            results.append(res)
    for r in results:
        tr.result(r)
    return results


def _by_holder(tns, results, kit, skip=(0,)):
    return [r for t in tns if t.Index not in skip for r in results if kit.share(r)[0] == t.Index]


def full(kit, tr, fast=False, n=5, thr=5, tag=b"full"):
    tns = nodes(kit, tag, n)
    results = run_dkg(kit, tr, tag, tns, kit.config(NewNodes=node_list(kit, tns), Threshold=thr, FastSync=fast))
    assert len(results) == n
    check_results(kit, thr, results)
    return tns, results


def full_fast(kit, tr):
    full(kit, tr, fast=True, tag=b"fullfast")


def threshold(kit, tr):
    n, thr = 5, 4
    tns = nodes(kit, b"thr", n)

    def dm(deals):
        deals = deals[1:]
        deals[0].Deals[2].EncryptedShare = b"Another one bites the dust"
        return deals

    def rm(resp):
        assert all(b.ShareIndex != 0 for b in resp)
        assert any(r.DealerIndex == 0 for b in resp for r in b.Responses) and any(r.DealerIndex == 1 for b in resp for r in b.Responses)
        return resp

    def jm(justs):
        assert {0, 1} <= {b.DealerIndex for b in justs}
        return justs

    results = run_dkg(kit, tr, b"thr", tns, kit.config(NewNodes=node_list(kit, tns), Threshold=thr), dm, rm, jm)
    filtered = _by_holder(tns, results, kit)
    assert all(q.Index != 0 for r in filtered for q in r.QUAL)
    check_results(kit, thr, filtered)


def too_many_complaints(kit, tr):
    n, thr = 5, 3
    tns = nodes(kit, b"tmc", n)

    def dm(deals):
        for i in range(thr + 1):
            deals[0].Deals[i].EncryptedShare = b"Another one bites the dust"
        return deals

    results = run_dkg(kit, tr, b"tmc", tns, kit.config(NewNodes=node_list(kit, tns), Threshold=thr), dm)
    filtered = _by_holder(tns, results, kit)
    assert all(q.Index != 0 for r in filtered for q in r.QUAL)
    check_results(kit, thr, filtered)


def nonce_invalid_eviction(kit, tr):
    n, thr = 7, 4
    tns = nodes(kit, b"nie", n)

    def dm(deals):
        deals[0].SessionID = b"Beat It"
        deals[1].Public = [kit.point(O.mul_base(DO.le(1000 + i))) for i in range(thr)]
        return deals

    def rm(resp):
        for b in resp:
            assert all(r.DealerIndex != 0 for r in b.Responses)
            if b.ShareIndex == 2:
                b.SessionID = b"Billie Jean"
        return resp

    def jm(just):
        assert len(just) == 1
        just[0].SessionID = b"Free"
        return just

    results = run_dkg(kit, tr, b"nie", tns, kit.config(NewNodes=node_list(kit, tns), Threshold=thr), dm, rm, jm)
    filtered = [r for r in results if kit.share(r)[0] not in (0, 1, 2)]
    assert all(q.Index not in (0, 1, 2) for r in filtered for q in r.QUAL)
    check_results(kit, thr, filtered)


def invalid_response(kit, tr):
    I = kit.impl
    n, thr = 6, 3
    tns = nodes(kit, b"ir", n)
    setup(kit, b"ir", tns, kit.config(NewNodes=node_list(kit, tns), Threshold=thr))
    deals = [t.dkg.Deals() for t in tns][1:]
    resps = []
    for t in tns:
        r = t.dkg.ProcessDeals(deals)
        tr.bundle(r)
        assert (r is None) == (t.Index == 0)
        if r is not None:
            resps.append(r)
    resps[1].Responses[0].DealerIndex = 1000
    resps[2].Responses[0].Status = I.Success
    justifs = []
    for i, t in enumerate(tns):
        try:
            res, just = t.dkg.ProcessResponses(resps)
            assert i != 0 and res is None
        except I.ErrEvicted as e:
            assert i == 0
            just = e.bundle
        tr.node(t)
        tr.bundle(just)
        if just is not None:
            justifs.append(just)
    results = []
    for t in tns:
        if t.Index in (0, 2, 3):
            continue
        res = t.dkg.ProcessJustifications(justifs)
        tr.node(t)
        tr.result(res)
        assert all(q.Index not in (0, 2, 3) for q in res.QUAL)
        results.append(res)
    check_results(kit, thr, results)


def self_eviction_dealer(kit, tr):
    I = kit.impl
    n, thr = 5, 3
    tns = nodes(kit, b"sed", n)
    tns[3].Index = 53
    lst = node_list(kit, tns)
    setup(kit, b"sed", tns, kit.config(NewNodes=lst, Threshold=thr, FastSync=True))
    evict = lst[0].Index
    deals = [b for t, b in [(t, t.dkg.Deals()) for t in tns] if t.Index != evict]
    resps = [r for r in (t.dkg.ProcessDeals(deals) for t in tns) if r is not None]
    for r in resps:
        tr.bundle(r)
    for t in tns:
        try:
            t.dkg.ProcessResponses(resps)
            assert t.Index != evict and evict in t.dkg.evicted
        except I.ErrEvicted:
            assert t.Index == evict
        tr.node(t)


def nonce_invalid_and_absent_auth(kit, tr):
    I = kit.impl
    tns = nodes(kit, b"nonce", 5)
    base = dict(NewNodes=node_list(kit, tns), Threshold=5, FastSync=True, Longterm=tns[0].Private,
                Reader=kit.stream(b"r"), Rand=kit.stream(b"s"))
    assert I.NewDistKeyHandler(kit.config(Nonce=bytes(32), Auth=kit.auth(b"a"), **base)) is not None
    for bad in (dict(Nonce=b"that's some bad nonce", Auth=kit.auth(b"a")), dict(Nonce=bytes(32), Auth=None)):
        try:
            I.NewDistKeyHandler(kit.config(**bad, **base))
        except ValueError:
            continue
        raise AssertionError("NewDistKeyHandler must refuse %r" % (bad,))


def config_duplicate_and_minimum_t(kit, tr):
    I = kit.impl
    lst = [I.Node(i, None) for i in range(5)]
    lst[2].Index = lst[1].Index
    for kw in (dict(OldNodes=lst), dict(NewNodes=lst)):
        try:
            kit.config(**kw).CheckForDuplicates()
        except ValueError:
            continue
        raise AssertionError("duplicate indices must be refused")
    assert [I.MinimumT(n) for n in (10, 6, 4, 3, 2, 7, 8, 9)] == [6, 4, 3, 2, 2, 4, 5, 5]


def _reshare(kit, tr, tag, tns, lst, thr, new_tns, new_t, fast, mangle=None):
    """the second half of TestDKGResharing / TestDKGSkipIndex / TestSelfEvictionShareHolder: old holders deal to the new
    group; returns the nodes' outcomes of ProcessResponses"""
    I = kit.impl
    conf = kit.config(NewNodes=node_list(kit, new_tns), OldNodes=lst, Threshold=new_t, OldThreshold=thr, FastSync=fast)
    setup(kit, tag + b" reshare", new_tns, conf, coeffs=tns[0].res.Key.Commits)
    deals = [t.dkg.Deals() for t in new_tns if t.res is not None]
    for b in deals:
        tr.bundle(b)
    resps = []
    for t in new_tns:
        r = t.dkg.ProcessDeals(deals)
        if r is not None and mangle:
            mangle(t, r)
        tr.bundle(r)
        if r is not None:
            resps.append(r)
    assert resps
    out = []
    for t in new_tns:
        try:
            out.append(t.dkg.ProcessResponses(resps))
        except I.ErrEvicted:
            out.append("evicted")
        tr.node(t)
    return out


def resharing(kit, tr, fast=False, tag=b"reshare"):
    n, thr = 5, 4
    tns, results = full(kit, tr, n=n, thr=thr, tag=tag)
    for t, r in zip(tns, results):
        t.res = r
    lst = node_list(kit, tns)
    new_tns = tns[:n - 1] + nodes(kit, tag + b" new", 6, first=n - 1)
    new_t = thr + 4
    out = _reshare(kit, tr, tag, tns, lst, thr, new_tns, new_t, fast)
    assert all(o == (None, None) for o in out)  # the absent old node can justify nothing
    results = [t.dkg.ProcessJustifications(None) for t in new_tns]
    for r in results:
        tr.result(r)
    check_results(kit, new_t, results)
    assert [kit.pt(results[0].Key.Commits[0])] == [kit.pt(tns[0].res.Key.Commits[0])]  # the distributed key did not move


def resharing_fast(kit, tr):
    resharing(kit, tr, fast=True, tag=b"resharefast")


def skip_index(kit, tr):
    n, thr = 5, 4
    tns = nodes(kit, b"skip", n)
    tns[1].Index = 53
    lst = node_list(kit, tns)
    results = run_dkg(kit, tr, b"skip", tns, kit.config(NewNodes=lst, Threshold=thr))
    check_results(kit, thr, results)
    for t, r in zip(tns, results):
        t.res = r
    new_tns = [t for i, t in enumerate(tns) if i != 2] + [TestNode(kit, b"skip new %d" % i, n + i) for i in range(6) if i != 2]
    new_t = thr + 5 - 1
    out = _reshare(kit, tr, b"skip", tns, lst, thr, new_tns, new_t, False)
    assert all(o == (None, None) for o in out)
    results = [t.dkg.ProcessJustifications(None) for t in new_tns]
    for r in results:
        tr.result(r)
    check_results(kit, new_t, results)


def self_eviction_share_holder(kit, tr):
    n, thr = 5, 4
    tns, results = full(kit, tr, n=n, thr=thr, tag=b"sesh")
    for t, r in zip(tns, results):
        t.res = r
    new_tns = tns + [TestNode(kit, b"sesh new %d" % i, n + 1 + i) for i in range(5)]
    evict = new_tns[-1].Index

    def mangle(t, r):
        if t.Index == evict:
            r.SessionID = b"That looks so wrong"

    out = _reshare(kit, tr, b"sesh", tns, node_list(kit, tns), thr, new_tns, thr + 4, True, mangle)
    for t, o in zip(new_tns, out):
        assert evict in t.dkg.evictedHolders and (o == "evicted") == (t.Index == evict)


SCENARIOS = {"TestDKGFull": full, "TestDKGThreshold": threshold, "TestDKGFullFast": full_fast, "TestDKGSkipIndex": skip_index,
             "TestDKGNonceInvalid+TestDKGAbsentAuth": nonce_invalid_and_absent_auth,
             "TestDKGNonceInvalidEviction": nonce_invalid_eviction, "TestDKGInvalidResponse": invalid_response,
             "TestDKGTooManyComplaints": too_many_complaints, "TestConfigDuplicate+TestMinimumT": config_duplicate_and_minimum_t,
             "TestSelfEvictionDealer": self_eviction_dealer, "TestSelfEvictionShareHolder": self_eviction_share_holder,
             "TestDKGResharing": resharing, "TestDKGResharingFast": resharing_fast}


def run(kit, name):
    tr = Transcript(kit)
    SCENARIOS[name](kit, tr)
    return list(tr)
