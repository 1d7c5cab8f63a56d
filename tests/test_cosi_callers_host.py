"""kyber_amd/sign/cosi.py and kyber_amd/sign/policy.py without a GPU: the engine calls they make (batch_mask_aggregate,
batch_cosi_verify, and the point arithmetic of the sequential path: batch_mul, batch_mul_base, batch_add, batch_mul2)
are replaced by the oracle behind the wrappers' signatures, as tests/test_proof_callers_host.py does it; everything else
is the product's code.  Checked: the reference's scenarios, every error string in its order, batch against sequential,
the fused against the composed path, and a SHA-256 suite through the composed path."""
import hashlib

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _cosi_cases as CC
from tests import _cosi_oracle as CO

CALLS = []  # the engine calls the product made, by name


def _rows(x, width=32):
    a = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=np.uint8)
    return a.reshape(-1, width)


def _pts(rows):
    return np.frombuffer(b"".join(r or bytes(32) for r in rows), dtype=np.uint8).reshape(-1, 32).copy()


def _masks(masks):
    return [bytes(x) for x in masks] if isinstance(masks, (list, tuple)) else [bytes(r.tobytes()) for r in np.asarray(masks)]


def stand_ins(monkeypatch):
    from kyber_amd.group import edwards25519 as ed

    def mul1(s, p):
        return O.mul(s.tobytes(), p.tobytes())

    def batch_mul(scalars, points, vartime=False, uniform=False):
        CALLS.append("batch_mul")
        vals = [mul1(s, p) for s, p in zip(_rows(scalars), _rows(points))]
        return _pts(vals), np.array([v is None for v in vals], dtype=np.uint8)

    def batch_mul_base(scalars, vartime=False, uniform=False):
        CALLS.append("batch_mul_base")
        return _pts([O.mul_base(s.tobytes()) for s in _rows(scalars)])

    def batch_add(a, b):
        CALLS.append("batch_add")
        out = []
        for x, y in zip(_rows(a), _rows(b)):
            p, q = O.decode(x.tobytes()), O.decode(y.tobytes())
            out.append(None if p is None or q is None else O.encode(CO.padd(p, q)))
        return _pts(out), np.array([v is None for v in out], dtype=np.uint8)

    def batch_mul2(a, P, b, Q, vartime=False):
        CALLS.append("batch_mul2")
        out = []
        for s, p, t, q in zip(_rows(a), _rows(P), _rows(b), _rows(Q)):
            x, y = mul1(s, p), mul1(t, q)
            out.append(None if x is None or y is None else O.encode(CO.padd(O.decode(x), O.decode(y))))
        return _pts(out), np.array([v is None for v in out], dtype=np.uint8)

    def batch_mask_aggregate(roster, masks):
        CALLS.append("batch_mask_aggregate")
        pubs = [r.tobytes() for r in _rows(roster)]
        if any(len(m) != CO.mask_len(len(pubs)) for m in _masks(masks)):  # the wrapper's own check of a list of masks
            raise ValueError("mismatching mask lengths")
        res = [CO.abi_mask_aggregate(pubs, m) for m in _masks(masks)]
        return _pts([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.uint32), np.array([r[2] for r in res], dtype=np.uint8)

    def batch_cosi_verify(roster, msgs, sigs, masks, want_agg=False):
        CALLS.append("batch_cosi_verify")
        pubs = [r.tobytes() for r in _rows(roster)]
        res = [CO.abi_cosi_verify(pubs, bytes(msg), bytes(s), m) for msg, s, m in zip(msgs, sigs, _masks(masks))]
        return (np.array([r[0] for r in res], dtype=np.uint8), _pts([r[1] for r in res]) if want_agg else None,
                np.array([r[2] for r in res], dtype=np.uint32), np.array([r[3] for r in res], dtype=np.uint8))

    for f in (batch_mul, batch_mul_base, batch_add, batch_mul2, batch_mask_aggregate, batch_cosi_verify):
        monkeypatch.setattr(ed, f.__name__, f)
    from kyber_amd.sign import cosi

    del CALLS[:]
    return ed, cosi


def msg_of(err):
    return None if err is None else str(err)


def points(ed, encs):
    return [ed.Point(bytes(e)) for e in encs]


def scalar(ed, x: int):
    return ed.Scalar().SetBytes((x % O.L).to_bytes(32, "little"))


@pytest.mark.parametrize("n,f", CC.SCENARIOS)
def test_testcosi_through_the_product(monkeypatch, n, f):
    """cosi_test.go:69-158 with the product's functions, and byte for byte the oracle's signature"""
    ed, cosi = stand_ins(monkeypatch)
    suite = ed.NewSuite()
    privates, pubs, message, want_sig, thold = CC.scenario(n, f)
    publics = points(ed, pubs)
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
        assert sig == want_sig
        with pytest.raises(cosi.CosiError, match="signature too short"):
            cosi.Verify(suite, publics, message, sig[:10], policy)
        cosi.Verify(suite, publics, message, sig, policy)
        assert CO.Verify(pubs, message, sig, None if f == 0 else CO.NewThresholdPolicy(n - f)) is None
        assert m.CountEnabled() == n - f and m.CountTotal() == n
        if f:
            with pytest.raises(cosi.CosiError, match="the policy is not fulfilled"):
                cosi.Verify(suite, publics, message, sig)


def test_commit_draws_from_the_given_stream(monkeypatch):
    ed, cosi = stand_ins(monkeypatch)
    suite = ed.NewSuite()
    v, V = cosi.Commit(suite, lambda k: bytes(range(k)))
    assert V.MarshalBinary() == O.mul_base(v.MarshalBinary()) and v._int() == int.from_bytes(bytes(range(64)), "little") % O.L


def test_testmask_through_the_product(monkeypatch):
    """cosi_test.go:160-212"""
    ed, cosi = stand_ins(monkeypatch)
    suite = ed.NewSuite()
    n = 17
    pubs = [CC.plain_key(300 + i).enc for i in range(n)]
    publics = points(ed, pubs)
    masks = [cosi.NewMask(suite, publics, publics[i]) for i in range(n)]
    aggr = masks[0].Mask()
    for m in masks[1:]:
        aggr = cosi.AggregateMasks(aggr, m.Mask())
    masks[0].SetMask(aggr)
    assert masks[0].CountEnabled() == n and masks[0].Len() == 3 and masks[0].Mask() == aggr
    with pytest.raises(cosi.CosiError, match="key not found"):
        masks[0].KeyEnabled(masks[0].AggregatePublic)
    assert all(masks[0].KeyEnabled(p) for p in publics)
    assert masks[0].AggregatePublic.MarshalBinary() == CO.aggregate(pubs, aggr)[0]
    masks[0].SetBit(3, False)
    assert not masks[0].IndexEnabled(3) and masks[0].CountEnabled() == n - 1
    assert masks[0].AggregatePublic.MarshalBinary() == CO.aggregate(pubs, masks[0].Mask())[0]
    stray = bytearray(aggr)
    stray[-1] |= 0xFE  # bits at or above n: SetMask's loop never looks at them
    masks[1].SetMask(bytes(stray))
    assert masks[1].Mask() == aggr and masks[1].CountEnabled() == n
    for call in (lambda: masks[0].SetBit(n, True), lambda: masks[0].IndexEnabled(n)):
        with pytest.raises(cosi.CosiError, match="index out of range"):
            call()
    with pytest.raises(cosi.CosiError, match="mismatching mask lengths"):
        masks[0].SetMask(aggr[:2])
    with pytest.raises(cosi.CosiError, match="mismatching mask lengths"):
        cosi.AggregateMasks(aggr, aggr[:2])
    with pytest.raises(cosi.CosiError, match="key not found"):
        cosi.NewMask(suite, publics, ed.Point(CC.plain_key(999).enc))


def test_every_error_string_in_its_order(monkeypatch):
    ed, cosi = stand_ins(monkeypatch)
    suite = ed.NewSuite()
    _, pubs, message, sig, _ = CC.scenario(5, 0)
    publics = points(ed, pubs)
    bad_v = CC.not_a_point()
    cases = [
        ((None, message, sig), "no public keys provided"),
        ((publics, None, sig), "no message provided"),
        ((publics, message, None), "no signature provided"),
        ((publics, message, sig[:31]), "signature too short"),
        ((publics, message, bad_v), "unmarshalling of commitment failed"),  # before the second length check
        ((publics, message, sig[:63]), "signature too short"),
        ((publics, message, sig[:64]), "mismatching mask lengths"),
        ((publics, message, sig + b"\0"), "mismatching mask lengths"),
        ((publics, message, bad_v + sig[32:]), "unmarshalling of commitment failed"),
        ((publics, message + b"x", sig), "recreated response is different from signature"),
        ((publics, message, sig[:64] + b"\x0f"), "recreated response is different from signature"),  # before the policy
        ((publics, message, sig), None),
    ]
    for (p, m, s), want in cases:
        assert msg_of(cosi.VerifyBatch(suite, p, [m], [s])[0]) == want, want
        assert CO.Verify(None if p is None else pubs, m, s) == want, want
    # one batch of all of them: one fused call, and the same answers
    del CALLS[:]
    got = cosi.VerifyBatch(suite, publics, [c[0][1] for c in cases[1:]], [c[0][2] for c in cases[1:]])
    assert [msg_of(e) for e in got] == [c[1] for c in cases[1:]]
    assert CALLS.count("batch_cosi_verify") == 1
    for args, want in (((None, publics[0], message), "no commitment provided"), ((publics[0], publics[0], None), "no message provided")):
        with pytest.raises(cosi.CosiError, match=want):
            cosi.Challenge(suite, *args)
    one = scalar(ed, 1)
    for args, want in (((None, one, one), "no private key provided"), ((one, None, one), "no random scalar provided"),
                       ((one, one, None), "no challenge provided")):
        with pytest.raises(cosi.CosiError, match=want):
            cosi.Response(suite, *args)
    with pytest.raises(cosi.CosiError, match="no responses provided"):
        cosi.AggregateResponses(suite, None)
    mask = cosi.NewMask(suite, publics)
    for args, want in (((None, one, mask), "no commitment provided"), ((publics[0], None, mask), "no response provided"),
                       ((publics[0], one, None), "no mask provided")):
        with pytest.raises(cosi.CosiError, match=want):
            cosi.Sign(suite, *args)
    with pytest.raises(cosi.CosiError, match="mismatching lengths of commitment and mask slices"):
        cosi.AggregateCommitments(suite, publics[:2], [b"\0"])


@pytest.mark.parametrize("name", ["9", "17"])
def test_batch_against_sequential_and_fused_against_composed(monkeypatch, name):
    ed, cosi = stand_ins(monkeypatch)
    suite = ed.NewSuite()
    rs, ex = CC.rows(name), CC.expected(name)
    pubs = CC.publics(CC.keys_of(name))
    publics = [ed.Point(CO.canon(p)) for p in pubs]  # kyber.Point objects hold decoded points
    canon_pubs = [p.enc for p in publics]
    sigs = [r.sig + r.mask for r in rs]
    thold = len(pubs) // 2
    for policy, opolicy in ((None, None), (cosi.NewThresholdPolicy(thold), CO.NewThresholdPolicy(thold))):
        del CALLS[:]
        got = [msg_of(e) for e in cosi.VerifyBatch(suite, publics, [r.msg for r in rs], sigs, policy)]
        assert CALLS.count("batch_cosi_verify") == 1 and "batch_mask_aggregate" not in CALLS[:1]
        want = [CO.Verify(canon_pubs, r.msg, s, opolicy) for r, s in zip(rs, sigs)]
        assert got == want
        assert [g is None or g == "the policy is not fulfilled" for g in got] == [bool(e[0]) for e in ex]
        for i in range(0, len(rs), 7):  # Verify is VerifyBatch of one
            assert msg_of(cosi.VerifyBatch(suite, publics, [rs[i].msg], [sigs[i]], policy)[0]) == want[i]
    assert {None, "the policy is not fulfilled", "recreated response is different from signature"} <= set(want)
    del CALLS[:]
    ok, cnt, st = cosi._verify_batch_composed(b"".join(canon_pubs), [r.msg for r in rs], [r.sig for r in rs], [r.mask for r in rs])
    assert CALLS == ["batch_mask_aggregate", "batch_mul2"]
    assert list(ok) == [e[0] for e in ex] and list(cnt) == [e[2] for e in ex] and not st.any()


def test_a_sha256_suite_takes_the_composed_path(monkeypatch):
    ed, cosi = stand_ins(monkeypatch)
    suite = ed.NewSuite()
    n, f = 5, 2
    kp = [CC.plain_key(100 + i) for i in range(n)]
    privates, pubs = [k.a for k in kp], [k.enc for k in kp]
    signers = list(range(n - f))
    sig = CO.cosign(privates, pubs, signers, CC.MESSAGE, [CC._h("sha256", i) % O.L for i in signers], hashlib.sha256)
    publics = points(ed, pubs)
    policy = cosi.NewThresholdPolicy(n - f)
    for hash in (hashlib.sha256, "sha256"):
        del CALLS[:]
        got = cosi.VerifyBatch(suite, publics, [CC.MESSAGE, CC.MESSAGE + b"x", CC.MESSAGE], [sig, sig, sig[:40]], policy, hash=hash)
        assert [msg_of(e) for e in got] == [None, "recreated response is different from signature", "signature too short"]
        assert "batch_cosi_verify" not in CALLS and CALLS[:2] == ["batch_mask_aggregate", "batch_mul2"]
    assert CO.Verify(pubs, CC.MESSAGE, sig, CO.NewThresholdPolicy(n - f), hashlib.sha256) is None
    assert msg_of(cosi.VerifyBatch(suite, publics, [CC.MESSAGE], [sig], policy)[0]) == "recreated response is different from signature"
    for hash in (None, hashlib.sha512, "sha512"):  # SHA-512 by any of its names is the fused call
        del CALLS[:]
        cosi.VerifyBatch(suite, publics, [CC.MESSAGE], [sig], policy, hash=hash)
        assert CALLS[0] == "batch_cosi_verify"
    c256 = cosi.Challenge(suite, publics[0], publics[1], b"m", hash=hashlib.sha256)
    assert c256._int() == CO.challenge_int(pubs[0], pubs[1], b"m", hashlib.sha256)


def test_aggregate_batch_is_one_call(monkeypatch):
    ed, cosi = stand_ins(monkeypatch)
    rs, ex = CC.rows("17"), CC.expected("17")
    publics = [ed.Point(CO.canon(p)) for p in CC.publics(CC.keys_of("17"))]
    del CALLS[:]
    out, cnt = cosi.Mask.aggregate_batch(publics, [r.mask for r in rs])
    assert CALLS == ["batch_mask_aggregate"]
    assert [o.tobytes() for o in out] == [e[1] for e in ex] and list(cnt) == [e[2] for e in ex]
    with pytest.raises(cosi.CosiError, match="mismatching mask lengths"):
        cosi.Mask.aggregate_batch(publics, [b"\0\0"])
    with pytest.raises(cosi.CosiError, match="no public keys provided"):
        cosi.Mask.aggregate_batch([], [b""])


def test_policies():
    from kyber_amd.sign import cosi, policy

    class M:
        def __init__(self, on, total):
            self.on, self.total = on, total

        def CountEnabled(self):
            return self.on

        def CountTotal(self):
            return self.total

    assert policy.CompletePolicy().Check(M(5, 5)) and not policy.CompletePolicy().Check(M(4, 5))
    assert policy.NewThresholdPolicy(3).Check(M(3, 5)) and not policy.NewThresholdPolicy(3).Check(M(2, 5))
    assert policy.NewThresholdPolicy(0).Check(M(0, 5))
    assert (cosi.CompletePolicy, cosi.ThresholdPolicy, cosi.NewThresholdPolicy, cosi.Policy, cosi.ParticipationMask) == (
        policy.CompletePolicy, policy.ThresholdPolicy, policy.NewThresholdPolicy, policy.Policy, policy.ParticipationMask)
