"""kyber_amd.share.vss.pedersen, kyber_amd.share.vss.rabin and sign/schnorr's SignBatch without a GPU.  The four new engine calls are answered by the
lane programs themselves, compiled for the CPU (tests/vss_harness.cpp through tests/test_vss_host.py's entry points); the
standing calls the packages also make (mul_base, mul, add, unmarshal, commit, verify, deal_check) and deal_check2 by
stand-ins over the oracles, as tests/test_ecies_callers_host.py does.  Under test is the host logic: who is asked what and how often, in
which order the random stream is read, which errors are raised in which order -- every scenario of the reference's
two vss_test.go files, restated in tests/_vss_scenarios.py, must leave the transcript the sequential oracle leaves, byte for byte."""
import numpy as np
import pytest

from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _dkg_oracle as DO
from tests import _vss_scenarios as SC
from tests import test_vss_host as H


@pytest.fixture(scope="module")
def harness():
    return H.build_harness()


@pytest.fixture
def calls(monkeypatch, harness):
    """the engine behind kyber_amd.group.edwards25519 replaced; returns the count of calls per entry"""
    from kyber_amd.group import edwards25519 as ed

    count = {}

    def rows(x, w=32):
        x = bytes(np.ascontiguousarray(np.asarray(x, dtype=np.uint8)).tobytes()) if not isinstance(x, (bytes, bytearray)) else bytes(x)
        return [x[i:i + w] for i in range(0, len(x), w)]

    def arr(bs, w=32):
        return np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(-1, w).copy()

    def counted(name):
        def wrap(f):
            def g(*a, **k):
                count[name] = count.get(name, 0) + 1
                return f(*a, **k)
            return g
        return wrap

    @counted("vss_seal")
    def vss_seal(dh, k, priv, pub, pubs, ctx, msgs, ctx_len=32):
        keys, sigs, ciphers, st = H.seal(harness, bytes(dh), bytes(k), bytes(priv), bytes(pub), bytes(pubs), bytes(ctx), msgs, ctx_len=ctx_len)
        return arr(keys), arr(sigs, 64), ciphers, st

    @counted("vss_open")
    def vss_open(privs, keys, ctx, ciphers, ctx_len=32):
        slots, st = H.open_(harness, bytes(privs), bytes(keys), bytes(ctx), ciphers, ctx_len=ctx_len)
        return [s[:len(s) - 16] if not st[i] else b"" for i, s in enumerate(slots)], st

    @counted("schnorr_sign")
    def schnorr_sign(k, x, msgs):
        return arr(H.sign(harness, bytes(k), bytes(x), msgs), 64), np.zeros(len(msgs), dtype=np.uint8)

    @counted("deal_check")
    def deal_check(poly, idx, shares, commits, m, t):
        shares, commits = rows(shares), rows(commits)[:m * t]
        ok = [DC.expected_ok(s, commits[k * t:(k + 1) * t], i) for k, i, s in zip(poly, idx, shares)]
        return np.array(ok, dtype=np.uint8), np.zeros(m, dtype=np.uint8)

    @counted("verify")
    def verify(pubs, msgs, sigs, want_status=True):
        ok = []
        for p, m, s in zip(pubs, msgs, sigs):
            try:
                DO.Scheme(None).Verify(bytes(p), bytes(m), bytes(s))
                ok.append(1)
            except ValueError:
                ok.append(0)
        return np.array(ok, dtype=np.uint8), None

    def mul_base(scalars, vartime=False, uniform=False):
        return arr([O.mul_base(s) for s in rows(scalars)])

    def mul(scalars, points, vartime=False, uniform=False):
        out = [O.mul(s, p) for s, p in zip(rows(scalars), rows(points))]
        return arr([o or bytes(32) for o in out]), np.array([o is None for o in out], dtype=np.uint8)

    def add(a, b):
        return arr([O.encode(O.add(O.decode(x), O.decode(y))) for x, y in zip(rows(a), rows(b))]), np.zeros(len(rows(a)), dtype=np.uint8)

    def unmarshal(points):
        dec = [O.decode(p) for p in rows(points)]
        return arr([O.encode(d) if d is not None else bytes(32) for d in dec]), np.array([d is None for d in dec], dtype=np.uint8)

    def commit(scalars, base=None, vartime=False, uniform=False):
        return arr([O.mul(s, bytes(base)) if base is not None else O.mul_base(s) for s in rows(scalars)])

    @counted("deal_check2")
    def deal_check2(poly, idx, f, g, commits, H, m, t):
        from tests import _vss_oracle as VO

        f, g, commits, H = rows(f), rows(g), rows(commits)[:m * t], rows(H)
        ok = [VO.deal_check2(a, b, commits[k * t:(k + 1) * t], H[k if len(H) > 1 else 0], i) or 0 for k, i, a, b in zip(poly, idx, f, g)]
        return np.array(ok, dtype=np.uint8), np.zeros(m, dtype=np.uint8)

    for name, f in (("batch_deal_check2", deal_check2), ("batch_vss_seal", vss_seal), ("batch_vss_open", vss_open), ("batch_schnorr_sign", schnorr_sign),
                    ("batch_deal_check", deal_check), ("batch_verify", verify), ("batch_mul_base", mul_base), ("batch_mul", mul),
                    ("batch_add", add), ("batch_unmarshal", unmarshal), ("commit", commit)):
        monkeypatch.setattr(ed, name, f)
    return count


@pytest.fixture(scope="module")
def oracle_transcripts():
    """the oracle's transcript of every scenario, computed once"""
    K = SC.OracleKit()
    return {name: f(K) for name, f in SC.SCENARIOS.items()}


@pytest.mark.parametrize("name", list(SC.SCENARIOS))
def test_scenario_leaves_the_oracles_transcript(calls, oracle_transcripts, name):
    assert SC.SCENARIOS[name](SC.ProductKit()) == oracle_transcripts[name]


@pytest.fixture(scope="module")
def rabin_transcripts():
    K = SC.OracleKit("rabin")
    return {name: f(K) for name, f in SC.RABIN_SCENARIOS.items()}


@pytest.mark.parametrize("name", list(SC.RABIN_SCENARIOS))
def test_rabin_scenario_leaves_the_oracles_transcript(calls, rabin_transcripts, name):
    assert SC.RABIN_SCENARIOS[name](SC.ProductKit("rabin")) == rabin_transcripts[name]


def test_rabin_batch_entries_make_one_engine_call_each(calls):
    K = SC.ProductKit("rabin")
    w = SC.World(K)
    dealer, verifiers = w.genAll()
    calls.clear()
    deals = dealer.EncryptedDeals()
    assert calls == {"vss_seal": 1} and len(dealer.hkdfContext) == 128
    calls.clear()
    resps = K.process_deals(verifiers, deals)
    assert all(r.Approved for r in resps)
    assert calls == {"verify": 1, "vss_open": 1, "deal_check2": 1, "schnorr_sign": 1}
    calls.clear()
    assert K.process_responses(dealer, resps) == [None] * 7
    assert calls == {"verify": 1}
    assert dealer.DealCertified() and dealer.EnoughApprovals()


def test_batch_entries_make_one_engine_call_each(calls):
    K = SC.ProductKit()
    w = SC.World(K)
    dealer, verifiers = w.genAll()
    calls.clear()
    deals = dealer.EncryptedDeals()
    assert calls == {"vss_seal": 1}
    calls.clear()
    resps = K.process_deals(verifiers, deals)
    assert all(r.StatusApproved for r in resps)
    assert calls == {"verify": 1, "vss_open": 1, "deal_check": 1, "schnorr_sign": 1}
    calls.clear()
    assert K.process_responses(dealer, resps) == [None] * 7
    assert calls == {"verify": 1}
    assert dealer.DealCertified()


def test_sign_batch_draws_as_sequential_signs_do(calls):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import schnorr

    g = ed.NewSuite()
    privs = [g.Scalar().Pick(blake2xb.New(b"signer %d" % i)) for i in range(5)]
    msgs = [b"", b"a", bytes(47), bytes(range(48)), b"deal" * 40]
    seq_stream, batch_stream = blake2xb.New(b"nonces"), blake2xb.New(b"nonces")
    seq = [schnorr.Sign(g, p, m, rand=seq_stream) for p, m in zip(privs, msgs)]
    calls.clear()
    assert schnorr.SignBatch(g, privs, msgs, rand=batch_stream) == seq and calls == {"schnorr_sign": 1}
    assert seq_stream.Read(16) == batch_stream.Read(16)  # both streams stand at the same place
    streams = [blake2xb.New(b"own %d" % i) for i in range(5)]
    own = schnorr.SignBatch(g, privs, msgs, rand=streams)  # a stream per signer
    assert own == [schnorr.Sign(g, p, m, rand=blake2xb.New(b"own %d" % i)) for i, (p, m) in enumerate(zip(privs, msgs))]
    one = schnorr.SignBatch(g, privs[0], msgs, rand=blake2xb.New(b"one"))
    s = blake2xb.New(b"one")
    assert one == [schnorr.Sign(g, privs[0], m, rand=s) for m in msgs]
    assert schnorr.SignBatch(g, [], []) == []
    with pytest.raises(ValueError):
        schnorr.SignBatch(g, privs[:2], msgs)
    sk = DO.Scheme(None)
    for p, m, sig in zip(privs, msgs, seq):
        sk.Verify(O.mul_base(p.v), m, sig)
