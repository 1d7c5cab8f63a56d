"""kyber_amd/sign/cosi.py on the GPU: the reference's scenarios (TestCoSi at its four shapes with its policies and its
short signature, TestMask at 17 keys) through the package, eddsa's verification of sig[:64] under AggregatePublic, and
VerifyBatch with planted rejects against the oracle's messages."""
import hashlib

import pytest

from oracle import ed25519 as O
from tests import _cosi_cases as CC
from tests import _cosi_oracle as CO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import cosi, eddsa

    return ed, cosi, eddsa


def scalar(ed, x: int):
    return ed.Scalar().SetBytes((x % O.L).to_bytes(32, "little"))


def msg_of(err):
    return None if err is None else str(err)


@pytest.mark.parametrize("n,f", CC.SCENARIOS)
def test_testcosi(pkg, n, f):
    """cosi_test.go:69-158"""
    ed, cosi, eddsa = pkg
    suite = ed.NewSuite()
    privates, pubs, message, want_sig, _ = CC.scenario(n, f)
    publics = [ed.Point().UnmarshalBinary(p) for p in pubs]
    signers = list(range(n - f))
    masks = [cosi.NewMask(suite, publics, publics[i]) for i in signers]
    randoms = [scalar(ed, CC._h("scenario", n, f, 0, i)) for i in signers]
    V = [suite.Point().Mul(v, None) for v in randoms]
    aggV, agg_mask = cosi.AggregateCommitments(suite, V, [m.Mask() for m in masks])
    for m in masks:
        m.SetMask(agg_mask)
    c = [cosi.Challenge(suite, aggV, m.AggregatePublic, message) for m in masks]
    r = [cosi.Response(suite, scalar(ed, privates[i]), randoms[i], c[i]) for i in signers]
    aggr = cosi.AggregateResponses(suite, r)
    policy = None if f == 0 else cosi.NewThresholdPolicy(n - f)
    for m in masks:
        sig = cosi.Sign(suite, aggV, aggr, m)
        assert sig == want_sig  # the oracle's protocol run, byte for byte
        with pytest.raises(cosi.CosiError, match="signature too short"):
            cosi.Verify(suite, publics, message, sig[:10], policy)
        cosi.Verify(suite, publics, message, sig, policy)
        # a cosignature without its mask is an EdDSA signature under the aggregate key (cosi_test.go:152-156)
        assert eddsa.batch_verify_with_checks([m.AggregatePublic.MarshalBinary()], [message], [sig[:64]]).all()
        if f:
            with pytest.raises(cosi.CosiError, match="the policy is not fulfilled"):
                cosi.Verify(suite, publics, message, sig)
    v, Vc = cosi.Commit(suite)
    assert Vc.MarshalBinary() == O.mul_base(v.MarshalBinary())


def test_testmask(pkg):
    """cosi_test.go:160-212"""
    ed, cosi, _ = pkg
    suite = ed.NewSuite()
    n = 17
    pubs = [CC.plain_key(300 + i).enc for i in range(n)]
    publics = [ed.Point(p) for p in pubs]
    masks = [cosi.NewMask(suite, publics, publics[i]) for i in range(n)]
    aggr = masks[0].Mask()
    for m in masks[1:]:
        aggr = cosi.AggregateMasks(aggr, m.Mask())
    masks[0].SetMask(aggr)
    assert masks[0].CountEnabled() == n
    with pytest.raises(cosi.CosiError, match="key not found"):
        masks[0].KeyEnabled(masks[0].AggregatePublic)
    assert all(masks[0].KeyEnabled(p) for p in publics)
    assert masks[0].AggregatePublic.MarshalBinary() == CO.aggregate(pubs, aggr)[0]
    masks[0].SetBit(5, False)
    assert masks[0].AggregatePublic.MarshalBinary() == CO.aggregate(pubs, masks[0].Mask())[0]
    out, cnt = cosi.Mask.aggregate_batch(publics, [m.Mask() for m in masks])
    assert list(cnt) == [n - 1] + [1] * (n - 1)
    assert out[1:].tobytes() == b"".join(pubs[1:]) and out[0].tobytes() == masks[0].AggregatePublic.MarshalBinary()


@pytest.mark.parametrize("name", ["5", "17", "64"])
def test_verifybatch_with_planted_rejects(pkg, name):
    ed, cosi, _ = pkg
    suite = ed.NewSuite()
    rs = CC.rows(name)
    pubs = [CO.canon(p) for p in CC.publics(CC.keys_of(name))]
    publics = [ed.Point(p) for p in pubs]
    msgs = [r.msg for r in rs] + [CC.MESSAGE] * 4
    sigs = [r.sig + r.mask for r in rs] + [rs[0].sig[:10], rs[0].sig, rs[0].sig + rs[0].mask + b"\0", CC.not_a_point() + rs[0].sig[32:40]]
    thold = len(pubs) // 2
    for policy, opolicy in ((None, None), (cosi.NewThresholdPolicy(thold), CO.NewThresholdPolicy(thold))):
        got = [msg_of(e) for e in cosi.VerifyBatch(suite, publics, msgs, sigs, policy)]
        want = [CO.Verify(pubs, m, s, opolicy) for m, s in zip(msgs, sigs)]
        assert got == want
    assert want[-4:] == ["signature too short", "mismatching mask lengths", "mismatching mask lengths", "unmarshalling of commitment failed"]
    assert {None, "the policy is not fulfilled", "recreated response is different from signature"} <= set(want)


def test_a_sha256_suite_through_the_composed_path(pkg):
    ed, cosi, _ = pkg
    suite = ed.NewSuite()
    n, f = 5, 2
    kp = [CC.plain_key(100 + i) for i in range(n)]
    sig = CO.cosign([k.a for k in kp], [k.enc for k in kp], list(range(n - f)), CC.MESSAGE,
                    [CC._h("sha256", i) % O.L for i in range(n - f)], hashlib.sha256)
    publics = [ed.Point(k.enc) for k in kp]
    got = cosi.VerifyBatch(suite, publics, [CC.MESSAGE, CC.MESSAGE + b"x"], [sig, sig], cosi.NewThresholdPolicy(3), hash=hashlib.sha256)
    assert [msg_of(e) for e in got] == [None, "recreated response is different from signature"]
    assert msg_of(cosi.VerifyBatch(suite, publics, [CC.MESSAGE], [sig], cosi.NewThresholdPolicy(3))[0]) is not None
