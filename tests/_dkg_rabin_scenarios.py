"""The scenarios of the reference's share/dkg/rabin/dkg_test.go, restated once over a kit -- the product
(kyber_amd.share.dkg_rabin) or the oracle (tests/_dkg_rabin_oracle.py) -- so that both leave a transcript of bytes and error
strings under the same random stream.  dkg_test.go's fixtures: 7 participants, t = 4 (`nbParticipants/2 + 1`), keys from one
stream; `fullExchange` is the whole deal / response exchange, `gen_dist_secret` what dss_test.go's genDistSecret does on
top of it (secret commits, then DistKeyShare)."""
from tests._vss_scenarios import OracleKit, ProductKit, random_bytes

N, T = 7, 4


class Kit:
    def __init__(self, oracle: bool):
        self.oracle = oracle
        self.K = OracleKit("rabin") if oracle else ProductKit("rabin")
        if oracle:
            from tests import _dkg_rabin_oracle as M
        else:
            from kyber_amd.share import dkg_rabin as M
        self.M = M

    def new(self, S, longterm, pubs, t):
        return self.M.DistKeyGenerator(S, longterm, list(pubs), t)

    def approved(self, r):
        return r.StatusApproved if self.oracle else r.Approved

    def enc(self, v):
        return self.K.enc(v)

    def new_deal(self, sid, sec, rnd, t, commits):
        if self.oracle:
            from tests import _vss_oracle as VO

            return VO.RabinDeal(sid, sec, rnd, t, commits)
        from kyber_amd.share.vss import rabin

        return rabin.Deal(sid, sec, rnd, t, commits)

    def pri_share(self, i, v):
        if self.oracle:
            from tests import _vss_oracle as VO

            return VO.PriShare(i, v)
        from kyber_amd.share import poly

        return poly.PriShare(i, v)

    def plus_one(self, w, v):
        from oracle import ed25519 as O

        return (v + 1) % O.L if self.oracle else w.S.Scalar().Add(v, w.S.Scalar().One())

    def recover_secret(self, w, shares, n):
        """share.RecoverSecret(suite, shares, n, n), TestDistKeyShare's last step"""
        if self.oracle:
            from tests import _dkg_oracle as DO

            return DO.recover_secret([(s.I, s.V) for s in shares], n)
        from kyber_amd.share import poly

        return poly.recover_secret(w.S, shares, n, n)


class World:
    def __init__(self, kit, seed=b"dkg_test.go", n=N, t=T):
        self.kit, self.n, self.t = kit, n, t
        self.S = kit.K.stream(seed)
        self.secrets = [kit.K.pick(self.S) for _ in range(n)]
        self.pubs = [kit.K.base_mul(x) for x in self.secrets]

    def gen(self):  # dkgGen
        return [self.kit.new(self.S, x, self.pubs, self.t) for x in self.secrets]


def err(f, *a):
    try:
        return f(*a), None
    except (ValueError, RuntimeError) as e:
        return None, type(e).__name__ + ": " + str(e)


def full_exchange(dkgs, log=None):
    """fullExchange (dkg_test.go): every deal to its receiver, every response to every other participant"""
    resps = []
    for d in dkgs:
        deals = d.Deals()
        for i in sorted(deals):
            resps.append(dkgs[i].ProcessDeal(deals[i]))
    for r in resps:
        for d in dkgs:
            if r.Response.Index == d.index:
                continue  # (the issuer of a response has it already)
            j = d.ProcessResponse(r)
            assert j is None
    if log is not None:
        log.append(("responses", len(resps)))


def gen_dist_secret(kit, world):
    """dss_test.go's genDistSecret: a full exchange, the secret commits to everyone, then every DistKeyShare"""
    dkgs = world.gen()
    full_exchange(dkgs)
    scs = [d.SecretCommits() for d in dkgs]
    for sc in scs:
        for d in dkgs:
            if d.index != sc.Index:
                assert d.ProcessSecretCommits(sc) is None
    return dkgs, [d.DistKeyShare() for d in dkgs]


def dks_bytes(kit, dks):
    return ([kit.enc(c) for c in dks.Commitments()], dks.PriShare().I, kit.enc(dks.PriShare().V))


# ------------------------------------------------------------------------------------------------------- the scenarios
def new_dist_key_generator(kit):  # TestDKGNewDistKeyGenerator
    w = World(kit)
    d, e = err(kit.new, w.S, w.secrets[0], w.pubs, w.t)
    stranger = kit.K.pick(w.S)
    return [("good", e, d.index, kit.enc(d.pub)), ("stranger", err(kit.new, w.S, stranger, w.pubs, w.t)[1])]


def deal(kit):  # TestDKGDeal
    w = World(kit)
    d = w.gen()[0]
    deals = d.Deals()
    out = [("deals", sorted(deals), sorted(d.verifiers), [x.Index for x in deals.values()])]
    out += [("cipher", i, bytes(deals[i].Deal.Cipher), kit.enc(deals[i].Deal.DHKey), bytes(deals[i].Deal.Signature)) for i in sorted(deals)]
    again = d.Deals()  # our own deal is processed once
    out.append(("again", sorted(again), sorted(d.verifiers)))
    return out


def process_deal(kit):  # TestDKGProcessDeal
    w = World(kit)
    dkgs = w.gen()
    d0, d1 = dkgs[0], dkgs[1]
    deals = d0.Deals()
    out = []
    good = deals[1]
    good.Index = w.n + 1
    out.append(("index", err(d1.ProcessDeal, good)[1]))
    good.Index = 0
    cipher = good.Deal.Cipher
    good.Deal.Cipher = cipher[:10] + bytes([cipher[10] ^ 1]) + cipher[11:]
    out.append(("cipher", err(d1.ProcessDeal, good)[1], sorted(d1.verifiers)))
    good.Deal.Cipher = cipher
    r, e = err(d1.ProcessDeal, good)
    out.append(("good", e, r.Index, r.Response.Index, kit.approved(r.Response), bytes(r.Response.SessionID), bytes(r.Response.Signature),
                sorted(d1.verifiers)))
    out.append(("twice", err(d1.ProcessDeal, good)[1]))
    return out


def _h(kit, w, obj):
    return obj.Hash() if kit.oracle else obj.Hash(w.S)


def _flip(sig, tag):
    """randomBytes(len(sig)) of the reference: other bytes of the same length, the same for both kits"""
    return random_bytes(tag, len(sig))


def _set_approved(kit, r, v):
    if kit.oracle:
        r.StatusApproved = v
    else:
        r.Approved = v


def _without(d, attr, key, f, *a):
    """f(*a) with d.<attr>[key] taken out, as the reference deletes a verifier or a commitment and puts it back"""
    table = getattr(d, attr)
    kept = table.pop(key)
    try:
        return err(f, *a)
    finally:
        table[key] = kept


def process_response(kit):  # TestDKGProcessResponse, as written: a wrong deal, its complaint, the justification
    w = World(kit)
    dkgs = w.gen()
    dkg, rec = dkgs[0], dkgs[1]
    zero = 0 if kit.oracle else w.S.Scalar().Zero()
    deal = dkg.dealer.PlaintextDeal(1)
    good = deal.RndShare.V
    deal.RndShare.V = zero  # give a wrong deal
    encD = dkg.Deals()[1]
    resp, e = err(rec.ProcessDeal, encD)
    out = [("complaint", e, resp.Index, resp.Response.Index, kit.approved(resp.Response), bytes(resp.Response.SessionID), bytes(resp.Response.Signature))]
    deal.RndShare.V = good
    out.append(("no verifier", _without(dkg, "verifiers", 0, dkg.ProcessResponse, resp)))
    sig = resp.Response.Signature
    resp.Response.Signature = _flip(sig, b"response")
    out.append(("invalid response", err(dkg.ProcessResponse, resp)))
    resp.Response.Signature = sig
    j, e = err(dkg.ProcessResponse, resp)  # valid complaint from our deal
    out.append(("justification", e, j.Index, j.Justification.Index, bytes(j.Justification.SessionID), bytes(j.Justification.Signature),
                bytes(j.Justification.Deal.Marshal())))
    # a complaint about another peer's deal
    dkg2 = dkgs[2]
    deal21 = dkg2.dealer.PlaintextDeal(1)
    good21 = deal21.RndShare.V
    deal21.RndShare.V = zero
    deals2 = dkg2.Deals()
    resp12, e = err(rec.ProcessDeal, deals2[1])
    out.append(("complaint 12", e, resp12.Index, kit.approved(resp12.Response), bytes(resp12.Response.Signature)))
    deal21.RndShare.V = good21
    deals2 = dkg2.Deals()
    r, e = err(dkg.ProcessDeal, deals2[0])
    out.append(("deal 2 -> 0", e, r.Index, kit.approved(r.Response), bytes(r.Response.Signature)))
    out.append(("response from 1", err(dkg.ProcessResponse, resp12)))
    j, e = err(dkg2.ProcessResponse, resp12)  # the dealer justifies
    out.append(("justification 2", e, j.Index, j.Justification.Index, bytes(j.Justification.Signature), bytes(j.Justification.Deal.Marshal())))
    _set_approved(kit, resp12.Response, False)  # (all is local: the dealer changed the response it was handed)
    out.append(("process justification", err(dkg.ProcessJustification, j)))
    out.append(("no verifier for it", _without(dkg, "verifiers", j.Index, dkg.ProcessJustification, j)))
    return out


def secret_commits(kit):  # TestDKGSecretCommits
    w = World(kit)
    dkgs = w.gen()
    out = [("early", err(dkgs[0].SecretCommits)[1], err(dkgs[0].DistKeyShare)[1], dkgs[0].Certified(), dkgs[0].Finished())]
    full_exchange(dkgs, out)
    out.append(("qual", [d.QUAL() for d in dkgs], [d.Certified() for d in dkgs]))
    dkg, dkg2 = dkgs[0], dkgs[1]
    sc = dkg.SecretCommits()
    out.append(("sc", sc.Index, [kit.enc(c) for c in sc.Commitments], bytes(sc.SessionID), bytes(sc.Signature), bytes(_h(kit, w, sc))))
    out.append(("own signature", err(kit.K.verify, dkg.pub, _h(kit, w, sc), sc.Signature)[1]))
    good_i = sc.Index
    sc.Index = w.n + 1
    out.append(("index", err(dkg2.ProcessSecretCommits, sc)))
    sc.Index = good_i
    out.append(("not in qual", _without(dkg2, "verifiers", 0, dkg2.ProcessSecretCommits, sc)))
    sig = sc.Signature
    sc.Signature = _flip(sig, b"secret commits")
    out.append(("signature", err(dkg2.ProcessSecretCommits, sc)))
    sc.Signature = sig
    sid = sc.SessionID
    sc.SessionID = _flip(sid, b"session")
    out.append(("session", err(dkg2.ProcessSecretCommits, sc)))
    sc.SessionID = sid
    point = sc.Commitments[0]  # wrong commitments, signed by their dealer
    sc.Commitments[0] = kit.K.null()
    sc.Signature = kit.K.sign(w.S, w.secrets[0], _h(kit, w, sc))
    cc, e = err(dkg2.ProcessSecretCommits, sc)
    out.append(("complaint", e, cc.Index, cc.DealerIndex, bytes(cc.Signature), bytes(cc.Deal.Marshal()), 0 in dkg2.commitments))
    sc.Commitments[0], sc.Signature = point, sig
    out.append(("good", err(dkg2.ProcessSecretCommits, sc), 0 in dkg2.commitments))
    return out


def _all_secret_commits(dkgs, receivers):
    scs = [d.SecretCommits() for d in dkgs]
    for sc in scs:
        for d in receivers:
            assert d.ProcessSecretCommits(sc) is None  # (a participant's own included, as in the reference)
    return scs


def complaint_commits(kit):  # TestDKGComplaintCommits, and two steps it does not have (marked)
    w = World(kit)
    dkgs = w.gen()
    full_exchange(dkgs)
    scs = _all_secret_commits(dkgs, dkgs)
    wrong = kit.M.SecretCommits(scs[0].Index, list(scs[0].Commitments), scs[0].SessionID)
    wrong.Commitments[0] = kit.K.null()
    wrong.Signature = kit.K.sign(w.S, w.secrets[0], _h(kit, w, wrong))
    cc, e = err(dkgs[1].ProcessSecretCommits, wrong)
    out = [("cc", e, cc.Index, cc.DealerIndex, bytes(cc.Signature), bytes(cc.Deal.Marshal()))]
    dkg2 = dkgs[2]
    good_i = cc.Index
    cc.Index = w.n
    out.append(("issuer", err(dkg2.ProcessComplaintCommits, cc)))
    cc.Index = good_i
    out.append(("issuer not in qual (not in the reference)", _without(dkg2, "verifiers", 1, dkg2.ProcessComplaintCommits, cc)))
    sig = cc.Signature
    cc.Signature = _flip(sig, b"complaint commits")
    out.append(("signature", err(dkg2.ProcessComplaintCommits, cc)))
    cc.Signature = sig
    out.append(("no verifier", _without(dkg2, "verifiers", 0, dkg2.ProcessComplaintCommits, cc)))
    good_deal = cc.Deal  # "deal does not verify": a copy of the same fields, which DOES verify -- the reference's error
    cc.Deal = kit.new_deal(good_deal.SessionID, good_deal.SecShare, good_deal.RndShare, good_deal.T, good_deal.Commitments)
    out.append(("copied deal", err(dkg2.ProcessComplaintCommits, cc)))  # is the next check's: the secret commits pass
    moved = kit.pri_share(good_deal.RndShare.I, kit.plus_one(w, good_deal.RndShare.V))
    cc.Deal = kit.new_deal(good_deal.SessionID, good_deal.SecShare, moved, good_deal.T, good_deal.Commitments)
    cc.Signature = kit.K.sign(w.S, w.secrets[1], _h(kit, w, cc))
    out.append(("deal that does not verify (not in the reference)", err(dkg2.ProcessComplaintCommits, cc)))
    cc.Deal, cc.Signature = good_deal, sig
    out.append(("no commitments", _without(dkg2, "commitments", 0, dkg2.ProcessComplaintCommits, cc)))
    out.append(("secret commits pass", err(dkg2.ProcessComplaintCommits, cc)))
    return out


def reconstruct_commits(kit):  # TestDKGReconstructCommits
    w = World(kit)
    dkgs = w.gen()
    full_exchange(dkgs)
    _all_secret_commits(dkgs, dkgs[2:])

    def reconstruct_of(d):
        deal = d.verifiers[0].Deal()
        rc = kit.M.ReconstructCommits(deal.SessionID, d.index, 0, deal.SecShare)
        rc.Signature = kit.K.sign(w.S, w.secrets[d.index], _h(kit, w, rc))
        return rc

    rc = reconstruct_of(dkgs[1])
    out = [("rc", rc.Index, rc.DealerIndex, rc.Share.I, kit.enc(rc.Share.V), bytes(rc.SessionID), bytes(rc.Signature))]
    dkg2 = dkgs[2]
    dkg2.reconstructed[0] = True
    out.append(("reconstructed already", err(dkg2.ProcessReconstructCommits, rc), sorted(dkg2.pendingReconstruct)))
    del dkg2.reconstructed[0]
    out.append(("not invalidated", err(dkg2.ProcessReconstructCommits, rc)))
    del dkg2.commitments[0]
    rc.Index = w.n
    out.append(("index", err(dkg2.ProcessReconstructCommits, rc)))
    rc.Index = 1
    sig = rc.Signature
    rc.Signature = _flip(sig, b"reconstruct")
    out.append(("signature", err(dkg2.ProcessReconstructCommits, rc)))
    rc.Signature = sig
    out.append(("good", err(dkg2.ProcessReconstructCommits, rc), [p.Index for p in dkg2.pendingReconstruct[0]], dkg2.Finished()))
    out.append(("again", err(dkg2.ProcessReconstructCommits, rc), len(dkg2.pendingReconstruct[0])))
    for d in dkgs[2:]:
        rc = reconstruct_of(d)
        if dkg2.reconstructed.get(0):
            break
        sid = rc.SessionID
        rc.SessionID = _flip(sid, b"reconstruct session")  # (the signature does not cover it)
        out.append(("session", d.index, err(dkg2.ProcessReconstructCommits, rc)))
        rc.SessionID = sid
        out.append(("share", d.index, err(dkg2.ProcessReconstructCommits, rc), bool(dkg2.reconstructed.get(0))))
    com = dkg2.commitments[0]
    out.append(("recovered", bool(dkg2.reconstructed.get(0)), kit.enc(com[0] if kit.oracle else com.Commit()), kit.enc(dkgs[0].dealer.SecretCommit()),
                dkg2.Finished(), 0 in dkg2.pendingReconstruct))
    return out


def set_timeout(kit):  # TestSetTimeout: responses stop at EnoughApprovals; nobody is in QUAL before the timeout, everybody after
    w = World(kit)
    dkgs = w.gen()
    resps = []
    for d in dkgs:
        deals = d.Deals()
        for i in sorted(deals):
            r = dkgs[i].ProcessDeal(deals[i])
            assert kit.approved(r.Response)
            resps.append(r)
    for r in resps:
        for d in dkgs:
            if not d.verifiers[r.Index].EnoughApprovals():
                if r.Response.Index == d.index:
                    continue
                assert d.ProcessResponse(r) is None
    out = [("before", [d.QUAL() for d in dkgs], [d.Certified() for d in dkgs])]
    for d in dkgs:
        d.SetTimeout()
    out.append(("after", [d.QUAL() for d in dkgs], [d.Certified() for d in dkgs]))
    return out


def dist_key_share(kit):  # TestDistKeyShare
    w = World(kit)
    dkgs = w.gen()
    full_exchange(dkgs)
    last, scs = dkgs[-1], []
    for i, d in enumerate(dkgs[:-1]):
        sc = d.SecretCommits()
        scs.append(sc)
        for j, d2 in enumerate(dkgs[:-1]):
            if i != j:
                assert d2.ProcessSecretCommits(sc) is None
    out = [("before the commitments", err(last.DistKeyShare), last.Finished())]
    for sc in scs:
        assert last.ProcessSecretCommits(sc) is None
    sc = last.SecretCommits()
    for d in dkgs[:-1]:
        assert d.ProcessSecretCommits(sc) is None
        out.append(("sizes", d.index, len(d.QUAL()), len(d.commitments)))
    out.append(("one missing", _without(last, "commitments", 0, last.DistKeyShare)))
    out.append(("finished", [d.Finished() for d in dkgs]))
    dkss = [d.DistKeyShare() for d in dkgs]
    out.append(("keys", [dks_bytes(kit, k) for k in dkss]))
    secret = kit.recover_secret(w, [k.PriShare() for k in dkss], w.n)
    out.append(("secret", kit.enc(secret), kit.enc(kit.K.base_mul(secret)), kit.enc(dkss[0].Public())))
    return out


# dkg_test.go's nine tests, one function each
SCENARIOS = {"new_dist_key_generator": new_dist_key_generator, "deal": deal, "process_deal": process_deal, "process_response": process_response,
             "secret_commits": secret_commits, "complaint_commits": complaint_commits, "reconstruct_commits": reconstruct_commits,
             "set_timeout": set_timeout, "dist_key_share": dist_key_share}
