"""kyber_amd.sign.dss without a GPU.  The two new engine calls are answered by the lane programs themselves, compiled for
the CPU (tests/dss_harness.cpp through tests/test_dss_host.py's entry points); the standing calls the package also makes
(mul_base, mul, add, msm, verify) by stand-ins over the oracles, as tests/test_vss_callers_host.py does.  Under test is the
host logic: who is asked what and how often, in which order the random stream is read, which errors are raised in which
order -- every scenario of the reference's dss_test.go (TestDSSNew, TestDSSPartialSigs step by step, TestDSSSignature,
TestOutOfIndex) must leave what the sequential oracle (tests/_dss_oracle.py) leaves, byte for byte, under the same stream.

The distributed keys come from genDistSecret's full Rabin exchange (kyber_amd.share.dkg_rabin on the product's side,
tests/_dkg_rabin_oracle.py on the oracle's; 7 participants, t = 4), as in the reference: their commitments are sums of the
dealers' polynomials."""
import numpy as np
import pytest

from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests import _dkg_oracle as DO
from tests import _dkg_rabin_scenarios as DK
from tests import _dss_oracle as D
from tests import _ed_verify_oracle as V
from tests import test_dss_host as H
from tests.test_dkg_rabin_host import calls as dkg_calls, vss_calls  # noqa: F401  (fixtures: share/vss's and share/poly's stand-ins)
from tests.test_vss_callers_host import harness  # noqa: F401

N, T = 7, 4


@pytest.fixture(scope="module")
def dss_harness():
    return H.build_harness()


@pytest.fixture
def calls(monkeypatch, dss_harness, dkg_calls):
    """the engine behind kyber_amd.group.edwards25519 replaced; returns the count of calls per entry"""
    from kyber_amd.group import edwards25519 as ed

    count, harness = dkg_calls, dss_harness

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

    @counted("dss_check")
    def dss_check(participants, long_commits, rand_commits, msgs, sess, idx, Vs, sids, sigs):
        return H.check(harness, bytes(participants), bytes(long_commits), bytes(rand_commits), msgs, sess, idx, bytes(Vs), bytes(sids), bytes(sigs))

    @counted("dss_partial")
    def dss_partial(priv, index, alpha, beta, k, long_commits, rand_commits, msgs):
        return H.partial(harness, bytes(priv), index, bytes(alpha), bytes(beta), bytes(k), bytes(long_commits), bytes(rand_commits), msgs)

    @counted("verify")
    def verify(pubs, msgs, sigs, want_status=True):
        ok = [int(V.verify_with_checks(bytes(p), bytes(m), bytes(s))[0]) for p, m, s in zip(pubs, msgs, sigs)]
        st = [V.abi_status(bytes(p), bytes(m), bytes(s)) for p, m, s in zip(pubs, msgs, sigs)]
        return np.array(ok, dtype=np.uint8), (np.array(st, dtype=np.uint8) if want_status else None)

    def mul_base(scalars, vartime=False, uniform=False):
        return arr([O.mul_base(s) for s in rows(scalars)])

    def mul(scalars, points, vartime=False, uniform=False):
        out = [O.mul(s, p) for s, p in zip(rows(scalars), rows(points))]
        return arr([o or bytes(32) for o in out]), np.array([o is None for o in out], dtype=np.uint8)

    def add(a, b):
        return arr([O.encode(O.add(O.decode(x), O.decode(y))) for x, y in zip(rows(a), rows(b))]), np.zeros(len(rows(a)), dtype=np.uint8)

    def msm(scalars, points):
        acc = O.IDENTITY
        for s, p in zip(rows(scalars), rows(points)):
            acc = O.add(acc, O.mul_int(int.from_bytes(s, "little"), O.decode(p)))
        return np.frombuffer(O.encode(acc), dtype=np.uint8).copy(), np.zeros(1, dtype=np.uint8)

    for name, f in (("batch_dss_check", dss_check), ("batch_dss_partial", dss_partial), ("batch_verify", verify), ("batch_mul_base", mul_base),
                    ("batch_mul", mul), ("batch_add", add), ("msm", msm)):
        monkeypatch.setattr(ed, name, f)
    return count


# ------------------------------------------------------------------------------------- the two worlds, from one stream
_KEYS = {}


def _keys(oracle: bool, seed: bytes, nmsg: int):
    """dss_test.go's fixtures: n key pairs, then genDistSecret -- a FULL Rabin exchange, 7 participants with t = 4 -- once
    for the long-term key and once per message for the random keys; computed once per (kit, seed, nmsg)"""
    if (oracle, seed, nmsg) not in _KEYS:
        kit = DK.Kit(oracle)
        w = DK.World(kit, seed, N, T)
        longs = DK.gen_dist_secret(kit, w)[1]
        randoms = [DK.gen_dist_secret(kit, w)[1] for _ in range(nmsg)]
        _KEYS[oracle, seed, nmsg] = (w, longs, randoms)
    return _KEYS[oracle, seed, nmsg]


class OracleWorld:
    def __init__(self, seed=b"dss scenarios", nmsg=1):
        w, longs, randoms = _keys(True, seed, nmsg)
        self.secrets, self.pubs = w.secrets, w.pubs
        self.longs = [D.DistKeyShare(k.Commitments(), D.PriShare(k.PriShare().I, k.PriShare().V)) for k in longs]
        self.randoms = [[D.DistKeyShare(k.Commitments(), D.PriShare(k.PriShare().I, k.PriShare().V)) for k in r] for r in randoms]
        self.read = blake2xb.New(seed + b" nonces").Read  # what the signatures draw from, after the key generation

    def dss(self, i, msg=b"hello", b=0, read=None):
        return D.DSS(read or self.read, self.secrets[i], self.pubs, self.longs[i], self.randoms[b][i], msg, T)


class ProductWorld:
    def __init__(self, seed=b"dss scenarios", nmsg=1):
        w, self.longs, self.randoms = _keys(False, seed, nmsg)
        self.suite, self.secrets, self.pubs = w.S, w.secrets, w.pubs
        self.rand = blake2xb.New(seed + b" nonces")

    def dss(self, i, msg=b"hello", b=0, rand=None):
        from kyber_amd.sign import dss

        return dss.NewDSS(self.suite, self.secrets[i], self.pubs, self.longs[i], self.randoms[b][i], msg, T, rand=rand or self.rand)


def _err(f, *a):
    try:
        f(*a)
        return None
    except ValueError as e:
        return str(e)


def _ps_bytes(ps):
    v = ps.Partial.V
    return (ps.Partial.I, D.sc(v) if isinstance(v, int) else v.MarshalBinary(), bytes(ps.SessionID), bytes(ps.Signature))


def test_the_two_worlds_deal_the_same_keys(calls):
    o, p = OracleWorld(), ProductWorld()
    assert [x.MarshalBinary() for x in p.pubs] == o.pubs
    for a, b in zip(o.longs + o.randoms[0], p.longs + p.randoms[0]):
        assert a.Commitments() == [c.MarshalBinary() for c in b.Commitments()]
        assert D.sc(a.PriShare().V) == b.PriShare().V.MarshalBinary() and a.PriShare().I == b.PriShare().I


def test_dss_new(calls):  # TestDSSNew
    from kyber_amd.sign import dss

    o, p = OracleWorld(), ProductWorld()
    d = p.dss(0)
    assert d.index == 0 and d.sessionID == o.dss(0).sessionID
    stranger = p.suite.Scalar().Pick(blake2xb.New(b"stranger"))
    want = _err(D.DSS, None, DO.pick(blake2xb.New(b"stranger").Read), o.pubs, o.longs[0], o.randoms[0][0], b"hello", T)
    got = _err(dss.NewDSS, p.suite, stranger, p.pubs, p.longs[0], p.randoms[0][0], b"hello", T)
    assert got == want == "dss: public key not found in list of participants"


def _partial_sigs_scenario(world, restate):
    """TestDSSPartialSigs, step by step in the reference's order (plus a wrong session id); returns the transcript"""
    out = []
    d0, d1 = world.dss(0), world.dss(1)
    ps0 = d0.PartialSig()
    out.append(("ps0", _ps_bytes(ps0), len(d0.partials)))
    ps0 = d0.PartialSig()  # a second time: a fresh nonce, the same share, the list unaffected
    out.append(("second own partial", _ps_bytes(ps0), len(d0.partials)))
    # wrong index
    good_i = ps0.Partial.I
    ps0.Partial.I = 100
    out.append(("index", _err(d1.ProcessPartialSig, ps0)))
    ps0.Partial.I = good_i
    # wrong signature
    good_sig = ps0.Signature
    ps0.Signature = restate(b"\x01" * 64)
    out.append(("signature", _err(d1.ProcessPartialSig, ps0)))
    ps0.Signature = good_sig
    # invalid partial sig: V = 0, signed again by its owner
    good_v = ps0.Partial.V
    ps0.Partial.V = world.zero()
    ps0.Signature = world.sign(0, ps0)
    out.append(("partial", _err(d1.ProcessPartialSig, ps0), _ps_bytes(ps0)))
    ps0.Partial.V, ps0.Signature = good_v, good_sig
    # wrong session id, signed again
    good_sid = ps0.SessionID
    ps0.SessionID = b"\x7f" + good_sid[1:]
    ps0.Signature = world.sign(0, ps0)
    out.append(("session", _err(d1.ProcessPartialSig, ps0)))
    ps0.SessionID, ps0.Signature = good_sid, good_sig
    # fine, then already received
    out.append(("good", _err(d1.ProcessPartialSig, ps0), len(d1.partials)))
    out.append(("duplicate", _err(d1.ProcessPartialSig, ps0)))
    out.append(("not enough", d1.EnoughPartialSig(), _err(d1.Signature)))
    for i in range(2, N):
        out.append(("more", i, _err(d1.ProcessPartialSig, world.dss(i).PartialSig())))
    out.append(("enough", d1.EnoughPartialSig(), len(d1.partials)))
    ps1 = d1.PartialSig()
    out.append(("own", _err(d1.ProcessPartialSig, ps1), len(d1.partials), d1.Signature()))
    return out


def _bind(world, oracle: bool):
    if oracle:
        world.zero = lambda: 0
        world.sign = lambda i, ps: DO.Scheme(world.read).Sign(world.secrets[i], ps.Hash())
    else:
        from kyber_amd.sign import schnorr

        world.zero = lambda: world.suite.Scalar().Zero()
        world.sign = lambda i, ps: schnorr.Sign(world.suite, world.secrets[i], ps.Hash(world.suite), world.rand)
    return world


def test_dss_partial_sigs_step_by_step(calls):
    want = _partial_sigs_scenario(_bind(OracleWorld(), True), bytes)
    got = _partial_sigs_scenario(_bind(ProductWorld(), False), bytes)
    assert got == want
    assert [w[1] for w in want if w[0] in ("index", "signature", "partial", "session", "good", "duplicate", "own")] == [
        "dss: partial signature with invalid index", "schnorr: invalid signature", "dss: partial signature not valid",
        "dss: session id do not match", None, "dss: partial signature already received from peer",
        "dss: partial signature already received from peer"]
    assert ("not enough", False, "dkg: not enough partial signatures to sign") in want and ("enough", True, N - 1) in want
    assert all(w[2] is None for w in want if w[0] == "more")
    o = OracleWorld()
    assert V.verify_with_checks(o.longs[0].Commitments()[0], b"hello", want[-1][3]) == (True, V.OK)


def _signature_scenario(world, verify):
    """TestDSSSignature: every participant issues, every participant processes, every signature is the same and verifies"""
    dsss = [world.dss(i) for i in range(N)]
    pss = [d.PartialSig() for d in dsss]
    errs = [_err(d.ProcessPartialSig, ps) for i, d in enumerate(dsss) for j, ps in enumerate(pss) if i != j]
    sigs = [d.Signature() for d in dsss]
    for s in sigs:
        verify(world.longs[0], b"hello", s)
    return [_ps_bytes(ps) for ps in pss], errs, sigs


def test_dss_signature(calls):
    from kyber_amd.sign import dss

    want = _signature_scenario(OracleWorld(), lambda k, m, s: D.Verify(k.Commitments()[0], m, s))
    got = _signature_scenario(ProductWorld(), lambda k, m, s: dss.Verify(k.Public(), m, s))
    assert got == want and len(set(want[2])) == 1 and want[1] == [None] * (N * (N - 1))
    # dss_test.go:133-135: an EdDSA signature of the message under the distributed public key (the standing eddsa oracle)
    assert V.verify_with_checks(OracleWorld().longs[0].Commitments()[0], b"hello", want[2][0]) == (True, V.OK)
    for i, v, sid, sig in want[0]:  # every PartialSig.Signature passes schnorr.Verify
        assert V.verify_with_checks(OracleWorld().pubs[i], D.partial_hash(v, i, sid), sig)[0]


def test_out_of_index(calls):  # TestOutOfIndex
    from kyber_amd.sign import dss
    from kyber_amd.share import poly as share

    o, p = OracleWorld(), ProductWorld()
    d = p.dss(0)
    ps = dss.PartialSig(share.PriShare(100, p.suite.Scalar().One()), d.sessionID, bytes(64))
    want = _err(o.dss(0).ProcessPartialSig, D.PartialSig(D.PriShare(100, 1), d.sessionID, bytes(64)))
    assert _err(d.ProcessPartialSig, ps) == want == D.ErrInvalidSignatureIndex == str(dss.ErrInvalidSignatureIndex)
    assert [str(e) for e in dss.process_partial_sigs([(d, ps)])] == [want]


# ---------------------------------------------------------------------------------------------------- the batch entries
MSGS = [b"", b"hello", bytes(range(200))]


def test_partial_sig_batch_equals_the_loop_in_one_call(calls):
    from kyber_amd.sign import dss

    loop, batch = ProductWorld(nmsg=3), ProductWorld(nmsg=3)
    for i in (0, 5):
        seq = [loop.dss(i, m, b).PartialSig() for b, m in enumerate(MSGS)]
        calls.clear()
        nodes = [batch.dss(i, m, b) for b, m in enumerate(MSGS)]
        got = dss.PartialSigBatch(nodes)
        assert calls.get("dss_partial") == 1 and "verify" not in calls
        assert [_ps_bytes(p) for p in got] == [_ps_bytes(p) for p in seq]
        assert all(len(d.partials) == 1 and d.signed for d in nodes)
    assert loop.rand.Read(16) == batch.rand.Read(16)  # both streams stand at the same place
    assert dss.PartialSigBatch([]) == []
    # the oracle's transcript under the same stream
    o, fresh = OracleWorld(nmsg=3), ProductWorld(nmsg=3)
    assert [_ps_bytes(o.dss(0, m, b).PartialSig()) for b, m in enumerate(MSGS)] == [
        _ps_bytes(p) for p in dss.PartialSigBatch([fresh.dss(0, m, b) for b, m in enumerate(MSGS)])]


def _pairs(world, receiver):
    """every other participant's partial of three sessions for `receiver`, with rejects and a duplicate planted"""
    from kyber_amd.sign import dss, schnorr
    from kyber_amd.share import poly as share

    g = world.suite
    nodes = [world.dss(receiver, m, b) for b, m in enumerate(MSGS)]
    pairs = []
    for b, m in enumerate(MSGS):
        for j in range(N):
            if j != receiver:
                pairs.append((nodes[b], world.dss(j, m, b).PartialSig()))
    d, ps = pairs[2]
    pairs.insert(5, (d, ps))  # a duplicate of an accepted one
    moved = dss.PartialSig(share.PriShare(ps.Partial.I, g.Scalar().Add(ps.Partial.V, g.Scalar().One())), ps.SessionID)
    moved.Signature = schnorr.Sign(g, world.secrets[ps.Partial.I], moved.Hash(g), world.rand)
    pairs.insert(0, (d, moved))  # rejected for its V BEFORE the good one arrives: no duplicate then
    d2, ps2 = pairs[9]
    pairs[9] = (d2, dss.PartialSig(ps2.Partial, ps2.SessionID, ps2.Signature[:40] + bytes([ps2.Signature[40] ^ 1]) + ps2.Signature[41:]))
    d3, ps3 = pairs[12]
    pairs[12] = (d3, dss.PartialSig(share.PriShare(N, ps3.Partial.V), ps3.SessionID, ps3.Signature))
    d4, ps4 = pairs[15]
    other = dss.PartialSig(ps4.Partial, b"\x55" * 32)
    other.Signature = schnorr.Sign(g, world.secrets[ps4.Partial.I], other.Hash(g), world.rand)
    pairs[15] = (d4, other)
    pairs.append((d4, dss.PartialSig(ps4.Partial, b"short", ps4.Signature)))  # a session id of another length: the sequential way
    own = nodes[1].PartialSig()
    pairs.append((nodes[1], own))  # our own: already received
    return nodes, pairs


def test_process_partial_sigs_equals_the_loop_in_one_call(calls):
    from kyber_amd.sign import dss

    loop_nodes, loop_pairs = _pairs(ProductWorld(nmsg=3), 3)
    want = [_err(d.ProcessPartialSig, ps) for d, ps in loop_pairs]
    nodes, pairs = _pairs(ProductWorld(nmsg=3), 3)
    calls.clear()
    got = dss.process_partial_sigs(pairs)
    assert calls.get("dss_check") == 1
    assert [None if e is None else str(e) for e in got] == want
    assert {w for w in want if w} == {"dss: partial signature not valid", "dss: partial signature already received from peer",
                                       "schnorr: invalid signature", "dss: partial signature with invalid index",
                                       "dss: session id do not match"}
    for a, b in zip(loop_nodes, nodes):
        assert [(p.I, p.V.MarshalBinary()) for p in a.partials] == [(p.I, p.V.MarshalBinary()) for p in b.partials]
        assert a.partialsIdx == b.partialsIdx
    assert dss.SignatureBatch(nodes) == [d.Signature() for d in loop_nodes]
    assert dss.process_partial_sigs([]) == []
