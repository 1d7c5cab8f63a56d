"""kyber_amd.share.dkg without a GPU: the product modules through the reference's scenarios with every engine call
answered by a host stand-in over the oracles (as tests/test_callers_host.py does for share/poly), against the sequential
restatement tests/_dkg_oracle.py under the same random streams: bundles (their Hash(), ciphertexts and signatures),
statuses, eviction lists and results equal byte for byte; and the engine is asked ONCE per phase."""
import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as E
from tests import _dkg_cases as DC
from tests import _dkg_scenarios as S
from tests import _ecies_oracle as EO


def _rows(x):
    x = bytes(x) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8).tobytes()
    return [x[i:i + 32] for i in range(0, len(x), 32)]


def _arr(bs):
    return np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(len(bs), 32)


@pytest.fixture
def calls(monkeypatch):
    """the engine replaced by the oracles; returns the log of fused calls"""
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.share import poly

    log = []

    def seal(r, pubs, msgs):
        log.append("seal")
        r, pubs = _rows(r), _rows(pubs)
        pubs = pubs * len(r) if len(pubs) == 1 else pubs
        out = [EO.encrypt(a, p, m) for a, p, m in zip(r, pubs, msgs)]
        return [c or bytes(len(m) + 48) for c, m in zip(out, msgs)], np.array([c is None for c in out], dtype=np.uint8)

    def open_(privs, ctx):
        log.append("open")
        privs = _rows(privs)
        res = [EO.decrypt(x, c) for x, c in zip(privs * len(ctx) if len(privs) == 1 else privs, ctx)]
        return [m or b"" for m, _ in res], np.array([s for _, s in res], dtype=np.uint8)

    def deal_check(pl, idx, shares, commits, m, t):
        log.append("deal_check")
        shares, commits = _rows(shares), _rows(commits)
        bad = [any(E.decode(c) is None for c in commits[k * t:(k + 1) * t]) for k in range(m)]
        ok = [0 if bad[k] else DC.expected_ok(s, commits[k * t:(k + 1) * t], i) for k, i, s in zip(pl, idx, shares)]
        return np.array(ok, dtype=np.uint8), np.array(bad, dtype=np.uint8)

    def mul_base(scalars, vartime=False, uniform=False):
        return _arr([E.mul_base(s) for s in _rows(scalars)])

    def mul_same_base(scal, base):
        pt = E.encode(E.B) if base is None else bytes(base)
        return _arr([E.mul(s, pt, vartime=True) for s in _rows(scal)])

    def msm(scal, pts):
        acc = E.IDENTITY
        for s, p in zip(_rows(scal), _rows(pts)):
            acc = E.add(acc, E.mul_int(int.from_bytes(s, "little"), E.decode(p)))
        return np.frombuffer(E.encode(acc), dtype=np.uint8), np.zeros(len(_rows(scal)), dtype=np.uint8)

    def batch_add(a, b):
        out = [E.encode(E.add(E.decode(x), E.decode(y))) for x, y in zip(_rows(a), _rows(b))]
        return _arr(out), np.zeros(len(out), dtype=np.uint8)

    def poly_eval(commits, indices):
        log.append("poly_eval")
        c = _rows(commits)
        return _arr([DC.eval_commits(c, i) for i in indices]), np.zeros(len(c), dtype=np.uint8)

    for name, f in (("batch_ecies_seal", seal), ("batch_ecies_open", open_), ("batch_deal_check", deal_check),
                    ("batch_mul_base", mul_base), ("poly_eval", poly_eval)):
        monkeypatch.setattr(ed, name, f)
    monkeypatch.setattr(poly, "_ops", lambda group: (mul_same_base, msm, 32))
    monkeypatch.setattr(poly, "_add_op", lambda group: batch_add)
    return log


@pytest.mark.parametrize("name", sorted(S.SCENARIOS))
def test_product_equals_the_oracle_byte_for_byte(calls, name):
    got = S.run(S.ProductKit(), name)
    want = S.run(S.OracleKit(), name)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, g, w)


def test_one_engine_call_per_phase(calls):
    kit = S.ProductKit()
    tns = S.nodes(kit, b"calls", 5)
    S.setup(kit, b"calls", tns, kit.config(NewNodes=S.node_list(kit, tns), Threshold=3))
    del calls[:]
    deals = [t.dkg.Deals() for t in tns]
    assert calls == ["seal"] * 5
    deals[1].Deals[0].EncryptedShare = b"not a ciphertext of any share!!" * 2  # dealer 1 (index 1) to holder 0
    deals.append(deals[2])  # a duplicate dealer
    del calls[:]
    resp = tns[0].dkg.ProcessDeals(deals)
    assert calls == ["open", "deal_check"]
    assert [(r.DealerIndex, r.Status) for r in resp.Responses] == [(1, kit.impl.Complaint)] and tns[0].dkg.evicted == [2]
    resps = [resp] + [t.dkg.ProcessDeals(deals) for t in tns[1:]]
    justs = []
    for t in tns:
        try:
            _, j = t.dkg.ProcessResponses([r for r in resps if r is not None])
        except kit.impl.ErrEvicted as e:
            j = e.bundle
        if j is not None:
            justs.append(j)
    del calls[:]
    res = tns[0].dkg.ProcessJustifications(justs)
    assert calls == ["deal_check"] and res is not None and 2 not in [n.Index for n in res.QUAL]


def test_verify_packets_is_one_batch_call(calls, monkeypatch):
    from kyber_amd.sign import schnorr

    kit = S.ProductKit()
    tns = S.nodes(kit, b"packets", 4)
    conf = kit.config(NewNodes=S.node_list(kit, tns), Threshold=3)
    S.setup(kit, b"packets", tns, conf)
    deals = [t.dkg.Deals() for t in tns]
    deals[2].Signature = deals[1].Signature
    seen = []

    def verify(pubs, msgs, sigs):
        seen.append(len(sigs))
        sch = S.DO.Scheme(None)
        out = []
        for p, m, s in zip(pubs, msgs, sigs):
            try:
                sch.Verify(p, m, s)
                out.append(True)
            except ValueError:
                out.append(False)
        return np.array(out)

    monkeypatch.setattr(schnorr, "batch_verify_with_checks", verify)
    assert kit.impl.verify_packets(tns[0].dkg.c, deals) == [True, True, False, True] and seen == [4]
    kit.impl.VerifyPacketSignature(tns[0].dkg.c, deals[0])
    with pytest.raises(ValueError):
        kit.impl.VerifyPacketSignature(tns[0].dkg.c, deals[2])
    assert _lib.ST_ECIES_AUTH == EO.ST_ECIES_AUTH
