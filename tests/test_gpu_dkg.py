"""kyber_amd.share.dkg on the GPU: the reference's scenarios through the product modules on the device, equal to the
sequential restatement tests/_dkg_oracle.py under the same random streams (bundles byte for byte, results and eviction
lists equal); and one node's view of a DKG of 129 dealers with threshold 65 and four planted faults, against the composed
standing calls (PubPoly.Check, per-element Decrypt) and testResults' property -- the Python oracle needs minutes at that
size and is not asked."""
import hashlib

import pytest

from tests import _dkg_scenarios as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(S.SCENARIOS))
def test_product_on_the_device_equals_the_oracle(name):
    got = S.run(S.ProductKit(), name)
    want = S.run(S.OracleKit(), name)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i)


def test_one_nodes_view_at_129_dealers_with_planted_faults():
    from kyber_amd.encrypt import ecies
    from kyber_amd.share import poly

    kit = S.ProductKit()
    I, g = kit.impl, kit.suite
    n, thr = 129, 65
    tns = S.nodes(kit, b"big", n)
    S.setup(kit, b"big", tns, kit.config(NewNodes=S.node_list(kit, tns), Threshold=thr))
    deals = [t.dkg.Deals() for t in tns]  # 129 seal calls
    me = tns[0]
    # a bad share, a bad ciphertext, a wrong session id, a duplicate dealer
    wrong = g.Scalar().Add(tns[5].dkg.dpriv.Eval(0).V, g.Scalar().One())
    assert deals[5].Deals[0].ShareIndex == 0
    deals[5].Deals[0].EncryptedShare = ecies.Encrypt(g, me.Public, wrong.MarshalBinary())
    deals[6].Deals[0].EncryptedShare = hashlib.shake_256(b"garbage").digest(80)
    deals[8].SessionID = b"another session"
    deals.append(deals[7])
    resp = me.dkg.ProcessDeals(deals)
    assert me.dkg.evicted == [8, 7]
    assert [(r.DealerIndex, r.Status) for r in resp.Responses] == [(5, I.Complaint), (6, I.Complaint)]
    # the composed standing calls, dealer by dealer
    for b in deals[1:n]:
        k = b.DealerIndex
        try:
            sh = g.Scalar().UnmarshalBinary(ecies.Decrypt(g, me.Private, b.Deals[0].EncryptedShare))
            good = poly.PubPoly(g, None, b.Public).Check(poly.PriShare(0, sh))
        except ValueError:
            good = False
        assert good == (k not in (5, 6)), k
        if k not in (7, 8):
            assert (me.dkg.statuses.Get(k, 0) == I.Success) == good, k
            assert (k in me.dkg.validShares) == good
    res, just = me.dkg.ProcessResponses([resp])
    assert res is None and just is None and me.dkg.evicted == [8, 7]
    justs = []
    for k in (5, 6):
        tns[k].dkg.ProcessDeals(deals)
        _, j = tns[k].dkg.ProcessResponses([resp])
        assert [x.ShareIndex for x in j.Justifications] == [0]
        justs.append(j)
    res = me.dkg.ProcessJustifications(justs)
    qual = [q.Index for q in res.QUAL]
    assert qual == [i for i in range(n) if i not in (7, 8)]
    # testResults' property for this node: its share is the summed polynomial's evaluation, the sum over QUAL
    assert len(res.Key.Commits) == thr
    assert poly.PubPoly(g, None, res.Key.Commits).Check(res.Key.Share)
    want = sum(int.from_bytes(tns[k].dkg.dpriv.Eval(0).V.MarshalBinary(), "little") for k in qual) % S.L
    assert int.from_bytes(res.Key.Share.V.MarshalBinary(), "little") == want
    secret = sum(int.from_bytes(tns[k].dkg.dpriv.coeffs[0].MarshalBinary(), "little") for k in qual) % S.L
    assert res.Key.Commits[0].MarshalBinary() == g.Point().Mul(kit.scalar(secret), None).MarshalBinary()
