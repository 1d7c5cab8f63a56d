"""tests/_cosi_oracle.py pinned, without the product: the reference prints no CoSi bytes, so the pins are its own EdDSA
vectors -- cosi_test.go:152-156: a cosignature without its mask is an EdDSA signature under the aggregate key -- and its
test scenarios.  Also: the labelled table holds what it promises."""
import pytest

from oracle import ed25519 as O
from tests import _cosi_cases as CC
from tests import _cosi_oracle as CO
from tests import _ed_verify_oracle as VO


def test_sign_input_is_one_roster_of_1024_keys_each_row_under_its_one_bit_mask():
    pubs, msgs, sigs = CC.sign_input_roster()
    for i in range(0, 1024):
        one = CC.mask_of(1024, [i])
        assert CO.Verify(pubs, msgs[i], sigs[i] + one, CO.NewThresholdPolicy(1)) is None, i
        assert CO.aggregate(pubs, one) == (pubs[i], 1)
        other = CC.mask_of(1024, [(i + 1) % 1024])
        assert CO.Verify(pubs, msgs[i], sigs[i] + other, CO.NewThresholdPolicy(1)) == "recreated response is different from signature", i


def test_rfc8032_rows_with_a_roster_of_one():
    for pub, msg, sig in VO.rfc8032():
        assert CO.Verify([pub], msg, sig + b"\x01") is None
        assert CO.Verify([pub], msg, sig + b"\x00") == "recreated response is different from signature"
        assert CO.Verify([pub], msg + b"x", sig + b"\x01") == "recreated response is different from signature"


@pytest.mark.parametrize("n,f", CC.SCENARIOS)
def test_testcosi(n, f):
    """cosi_test.go:69-158"""
    _, pubs, msg, sig, thold = CC.scenario(n, f)
    policy = None if thold is None else CO.NewThresholdPolicy(thold)
    assert len(sig) == 64 + CO.mask_len(n)
    assert CO.Verify(pubs, msg, sig[:10], policy) == "signature too short"
    assert CO.Verify(pubs, msg, sig, policy) is None
    m = CO.Mask(pubs)
    m.SetMask(sig[64:])
    assert m.CountEnabled() == n - f
    assert VO.verify_with_checks(m.AggregatePublic, msg, sig[:64]) == (True, VO.OK)  # eddsa.Verify under the aggregate key
    if f:
        assert CO.Verify(pubs, msg, sig, None) == "the policy is not fulfilled"  # the complete policy
        assert CO.Verify(pubs, msg, sig, CO.NewThresholdPolicy(n - f + 1)) == "the policy is not fulfilled"


def test_the_error_strings_in_their_order():
    _, pubs, msg, sig, _ = CC.scenario(5, 0)
    bad_v = CC.not_a_point()
    assert CO.Verify(None, msg, sig) == "no public keys provided"
    assert CO.Verify(pubs, None, sig) == "no message provided"
    assert CO.Verify(pubs, msg, None) == "no signature provided"
    assert CO.Verify(pubs, msg, sig[:31]) == "signature too short"
    assert CO.Verify(pubs, msg, bad_v) == "unmarshalling of commitment failed"  # before the second length check
    assert CO.Verify(pubs, msg, sig[:63]) == "signature too short"
    assert CO.Verify(pubs, msg, sig[:64]) == "mismatching mask lengths"
    assert CO.Verify(pubs, msg, sig + b"\0") == "mismatching mask lengths"
    assert CO.Verify(pubs, msg, bad_v + sig[32:]) == "unmarshalling of commitment failed"
    assert CO.Verify(pubs, msg + b"x", sig) == "recreated response is different from signature"


def test_testmask():
    """cosi_test.go:160-212"""
    n = 17
    pubs = [CC.plain_key(300 + i).enc for i in range(n)]
    masks = [CO.Mask(pubs, pubs[i]) for i in range(n)]
    aggr = masks[0].Mask()
    for m in masks[1:]:
        aggr = CO.AggregateMasks(aggr, m.Mask())
    masks[0].SetMask(aggr)
    assert masks[0].CountEnabled() == n and masks[0].CountTotal() == n and masks[0].Len() == 3
    with pytest.raises(CO.CosiError, match="key not found"):
        masks[0].KeyEnabled(masks[0].AggregatePublic)
    assert all(masks[0].KeyEnabled(p) for p in pubs)
    assert masks[0].AggregatePublic == CO.aggregate(pubs, aggr)[0]
    masks[0].SetBit(3, False)
    assert not masks[0].IndexEnabled(3) and masks[0].CountEnabled() == n - 1
    assert masks[0].AggregatePublic == CO.aggregate(pubs, masks[0].Mask())[0]
    for call in (lambda: masks[0].SetBit(n, True), lambda: masks[0].IndexEnabled(n)):
        with pytest.raises(CO.CosiError, match="index out of range"):
            call()
    with pytest.raises(CO.CosiError, match="mismatching mask lengths"):
        masks[0].SetMask(aggr[:2])
    with pytest.raises(CO.CosiError, match="key not found"):
        CO.Mask(pubs, CC.plain_key(999).enc)


def test_the_aggregate_is_the_sum_by_the_reference_s_additions():
    """SetMask's incremental Add / Sub and the plain affine sum agree with aggregate() on a roster with the special keys"""
    keys = CC.publics(CC.roster(17))
    for label, mask in CC.masks_of(17):
        m = CO.Mask(keys)
        m.SetMask(mask[:3])
        acc = O.IDENTITY
        for j in CO.enabled(mask, 17):
            acc = O.add(acc, O.decode(keys[j]))
        assert CO.aggregate(keys, mask) == (O.encode(acc), m.CountEnabled()) and m.AggregatePublic == O.encode(acc), label


def test_the_table_holds_what_it_promises():
    """every label has an accepted and a rejected row where both can be constructed; the masks cover both sides of the
    complement rule, stray bits and every single bit; the special keys are what they claim"""
    verdicts = {}
    for name in CC.NAMES:
        rs, ex = CC.rows(name), CC.expected(name)
        for r, e in zip(rs, ex):
            verdicts.setdefault(r.label.split("/")[0], set()).add(e[0])
            if name == "bad5":
                assert e == (0, bytes(32), e[2], CO.ST_BAD_POINT)
            else:
                assert e[3] == 0 and e[2] == len(CO.enabled(r.mask, int(name)))
        if name != "bad5":
            m = int(name)
            singles = [r.mask for r in rs if r.label == "honest/single"]
            assert singles == [CC.mask_of(m, [j]) for j in range(m)]
            counts = {e[2] for r, e in zip(rs, ex)}
            assert {0, m, m // 2, m // 2 + 1} <= counts
            assert bool(m & 7) == any(r.label.startswith("honest/stray") for r in rs)
    for label in ("honest", "r+l", "r+15l", "identity-V", "msg-len"):
        assert verdicts[label] == {1}, label
    for label in ("mask-bit-flipped", "r-altered", "msg-altered", "V-not-a-point", "msg-len-altered", "undecodable-key"):
        assert verdicts[label] == {0}, label
    keys = CC.roster(9)
    t8 = O.decode(keys[2].enc)
    assert O.mul_int(8, t8) == O.IDENTITY and O.mul_int(4, t8) != O.IDENTITY
    assert O.decode(keys[1].enc) == O.decode(keys[7].enc) == O.decode(keys[8].enc) == O.IDENTITY
    assert keys[7].enc != CO.canon(keys[7].enc) and keys[8].enc != CO.canon(keys[8].enc)  # y >= p; "-0"
    assert keys[4].enc == keys[0].enc and CO.padd(O.decode(keys[5].enc), O.decode(keys[6].enc)) == O.IDENTITY
    assert O.mul_int(O.L, O.decode(keys[3].enc)) != O.IDENTITY and O.decode(CC.bad_roster()[2].enc) is None
