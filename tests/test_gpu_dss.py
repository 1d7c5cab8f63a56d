"""kyb_ed25519_dss_check and kyb_ed25519_dss_partial on the GPU, host and _dev entries, against the sequential oracle
(tests/_dss_oracle.py, on the labelled cases of tests/_dss_cases.py) and against the composed standing calls
(kyb_ed25519_verify, kyb_ed25519_schnorr_sign, kyb_ed25519_deal_check): the case table, batch sizes either side of the
wave and the block over one, three and 65 sessions with rejects planted at the first lane, the last lane and a block
edge, NULL status outputs, and sign/dss end to end over share/dkg/rabin."""
import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _dss_cases as K
from tests import _dss_oracle as D
from tests import _vss_oracle as VO
from tests.test_dss_host import run_cases, world_args

pytestmark = pytest.mark.gpu

NP, T = 7, 4
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


@pytest.fixture(scope="module")
def worlds():
    return K.worlds()


def _dev(x, dtype=np.uint8):
    import torch

    return torch.from_numpy(np.frombuffer(x, dtype=dtype).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=dtype)).cuda()


def _dev_msgs(msgs):
    return _dev(b"".join(msgs) or b"\0"), _dev(np.cumsum([0] + [len(m) for m in msgs]).astype(np.int64), np.int64)


def _dev_check(ed):
    """ed.batch_dss_check's signature, through the _dev entry"""

    def call(participants, long_commits, rand_commits, msgs, sess, idx, Vs, sids, sigs):
        import torch

        ok, st, sst = ed.batch_dss_check(_dev(participants), _dev(long_commits), _dev(rand_commits), _dev_msgs(msgs),
                                         _dev(np.asarray(sess, dtype=np.uint32).view(np.int32), np.int32),
                                         _dev(np.asarray(idx, dtype=np.uint32).view(np.int32), np.int32), _dev(Vs), _dev(sids), _dev(sigs))
        torch.cuda.synchronize()
        return ok.cpu().numpy(), st.cpu().numpy(), sst.cpu().numpy()

    return call


# ------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_check_on_the_case_table(ed, worlds, entry):
    call = ed.batch_dss_check if entry == "host" else _dev_check(ed)
    for w in worlds:
        rows = K.cases(w)
        ok, st, sst = run_cases(call, w, rows)
        for r, o, s in zip(rows, ok, st):
            assert (int(o), int(s)) == (int(r[6] == K.OK), r[6]), (w.name, r[0])
        assert list(sst) == w.sess_status(), w.name


def test_null_status_outputs_give_the_same_ok(ed, worlds):
    w = worlds[5]  # the world with a bad session: sess_status would be written
    rows = K.cases(w)
    want, _, _ = run_cases(ed.batch_dss_check, w, rows)
    pk, lc, rc, msgs = world_args(w)
    a = [np.frombuffer(x, dtype=np.uint8).copy() for x in (pk, lc, rc, b"".join(msgs), b"".join(r[3] for r in rows), b"".join(r[4] for r in rows),
                                                           b"".join(r[5] for r in rows))]
    off = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    se, ix = np.array([r[1] for r in rows], dtype=np.uint32), np.array([r[2] for r in rows], dtype=np.uint32)
    ok = np.full(len(rows), 0xEE, dtype=np.uint8)
    rc_ = _lib.load().kyb_ed25519_dss_check(len(rows), K.NP, a[0].ctypes.data, w.tl, a[1].ctypes.data, w.ns, w.tr, a[2].ctypes.data,
                                             a[3].ctypes.data, off.ctypes.data, se.ctypes.data, ix.ctypes.data, a[4].ctypes.data,
                                             a[5].ctypes.data, a[6].ctypes.data, ok.ctypes.data, None, None)
    assert rc_ == 0 and list(ok) == list(want)


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_partial_matches_the_oracle_schnorr_sign_and_verify(ed, worlds, entry):
    import torch

    for w in worlds:
        if w.name == "bad session":
            continue
        i = 6
        priv, alpha = DC.le(w.privs[i]), DC.le(w.alpha(i))
        beta = b"".join(DC.le(w.beta(b, i)) for b in range(w.ns))
        k = b"".join(w.nonce(b, i) for b in range(w.ns))
        _, lc, rc, msgs = world_args(w)
        if entry == "host":
            Vs, sids, sigs = ed.batch_dss_partial(priv, i, alpha, beta, k, lc, rc, msgs)
        else:
            Vs, sids, sigs = (x.cpu().numpy() for x in ed.batch_dss_partial(_dev(priv), i, _dev(alpha), _dev(beta), _dev(k), _dev(lc), _dev(rc),
                                                                            _dev_msgs(msgs)))
            torch.cuda.synchronize()
        got = [(bytes(Vs[b]), bytes(sids[b]), bytes(sigs[b])) for b in range(w.ns)]
        assert got == [w.honest(b, i) for b in range(w.ns)], w.name
        ms = [D.partial_hash(v, i, sid) for v, sid, _ in got]
        composed, _ = ed.batch_schnorr_sign(k, priv, ms)  # the same (k, priv, m) through the standing call
        assert [bytes(s) for s in composed] == [g[2] for g in got]
        ok, st = ed.batch_verify([w.participants[i]] * w.ns, ms, [g[2] for g in got])
        assert ok.all() and not st.any()


# -------------------------------------------------------------------------------------------- block edges and sessions
class Big:
    """np = 7, tl = tr = 4, 65 sessions; partial j belongs to session j % ns and signer j % 7"""

    def __init__(self):
        tag = b"dss gpu big"
        self.privs = [DC.scalar(tag + b" priv %d" % i) for i in range(NP)]
        self.pubs = [O.mul_base(DC.le(x)) for x in self.privs]
        self.long = [DC.scalar(tag + b" long %d" % k) for k in range(T)]
        self.rand = [[DC.scalar(tag + b" rand %d %d" % (b, k)) for k in range(T)] for b in range(65)]
        self.lc = [O.mul_base(DC.le(c)) for c in self.long]
        self.rc = [[O.mul_base(DC.le(c)) for c in row] for row in self.rand]
        self.msgs = [b"session %d " % b * (b % 5) for b in range(65)]
        self._honest = {}

    def honest(self, b, i):
        if (b, i) not in self._honest:
            k = DC.le(DC.scalar(b"dss gpu nonce %d %d" % (b, i)))
            h = D.hash_sig(self.rc[b][0], self.lc[0], self.msgs[b])
            v = DC.le((h * DC.eval_scalar(self.long, i) + DC.eval_scalar(self.rand[b], i)) % O.L)
            sid = D.session_id(self.lc, self.rc[b])
            self._honest[b, i] = (v, sid, VO.schnorr_sign(k, DC.le(self.privs[i]), D.partial_hash(v, i, sid), self.pubs[i]))
        return self._honest[b, i]

    def reject(self, kind, b, i):
        """(index, V, sid, sig, status) of one planted reject"""
        if (kind, b, i) not in self._honest:
            self._honest[kind, b, i] = self._reject(kind, b, i)
        return self._honest[kind, b, i]

    def _reject(self, kind, b, i):
        v, sid, sig = self.honest(b, i)
        if kind == K.INDEX:
            return NP, v, sid, sig, K.INDEX
        if kind == K.SIG:
            return i, v, sid, sig[:40] + bytes([sig[40] ^ 1]) + sig[41:], K.SIG
        k = DC.le(DC.scalar(b"dss gpu reject nonce %d %d" % (b, i)))
        if kind == K.SESSION:
            sid = sid[:5] + bytes([sid[5] ^ 0x10]) + sid[6:]
        else:
            v = DC.le((int.from_bytes(v, "little") + 1) % O.L)
        return i, v, sid, VO.schnorr_sign(k, DC.le(self.privs[i]), D.partial_hash(v, i, sid), self.pubs[i]), kind


@pytest.fixture(scope="module")
def big():
    return Big()


def _batch(big, ns, n, planted):
    """n partials, partial j of session j % ns and signer j % 7, with the rejects of `planted` ({lane: kind}) in place"""
    rows = []
    for j in range(n):
        b, i = j % ns, j % NP
        rows.append((b,) + big.reject(planted[j], b, i) if j in planted else (b, i) + big.honest(b, i) + (K.OK,))
    args = (b"".join(big.pubs), b"".join(big.lc), b"".join(b"".join(big.rc[b]) for b in range(ns)), big.msgs[:ns], [r[0] for r in rows],
            [r[1] for r in rows], b"".join(r[2] for r in rows), b"".join(r[3] for r in rows), b"".join(r[4] for r in rows))
    return rows, args


@pytest.mark.parametrize("ns", [1, 3, 65])
def test_block_edges_with_rejects_planted(ed, big, ns):
    """EACH reject -- index, signature, session id, share -- alone in its batch at the first lane, at the last lane and at
    both sides of the block edge (lanes 63 and 64), so that the bad element does not shift; host and _dev entries"""
    kinds = (K.INDEX, K.SIG, K.SESSION, K.PARTIAL)
    for n in SIZES:
        for kind in kinds:
            for lane in sorted({0, n - 1, min(63, n - 1), min(64, n - 1)}):
                rows, args = _batch(big, ns, n, {lane: kind})
                want = [kind if j == lane else K.OK for j in range(n)]
                assert [r[5] for r in rows] == want
                ok, st, sst = ed.batch_dss_check(*args)
                assert [int(s) for s in st] == want, (ns, n, kind, lane)
                assert [int(o) for o in ok] == [int(w == K.OK) for w in want] and not sst.any(), (ns, n, kind, lane)
                ok2, st2, _ = _dev_check(ed)(*args)
                assert list(ok2) == list(ok) and list(st2) == list(st), (ns, n, kind, lane)


@pytest.mark.parametrize("ns", [1, 3, 65])
def test_verdicts_are_those_of_verify_and_deal_check(ed, big, ns):
    """a batch with every kind of reject in it: the signature verdicts are kyb_ed25519_verify's on the same (key, m, sig),
    the share verdicts kyb_ed25519_deal_check's on the folded commitments the oracle computed"""
    kinds = (K.INDEX, K.SIG, K.SESSION, K.PARTIAL)
    folded = b"".join(b"".join(D.folded(big.lc, big.rc[b], big.msgs[b])) for b in range(ns))
    n = 257
    rows, args = _batch(big, ns, n, {p: kinds[q % 4] for q, p in enumerate((0, 1, 2, 3, 62, 63, 64, 65, 128, 129, 254, 255, 256))})
    ok, st, _ = ed.batch_dss_check(*args)
    assert [int(s) for s in st] == [r[5] for r in rows] and [int(o) for o in ok] == [int(r[5] == K.OK) for r in rows]
    inside = [r for r in rows if r[1] < NP]
    vok, vst = ed.batch_verify([big.pubs[r[1]] for r in inside], [D.partial_hash(r[2], r[1], r[3]) for r in inside], [r[4] for r in inside])
    for r, o, s in zip(inside, vok, vst):
        assert (int(o), int(s)) == ((0, 0) if r[5] == K.SIG else (1, 0)), (ns, r[5])
    reach = [r for r in rows if r[5] in (K.OK, K.PARTIAL)]
    dok, dst = ed.batch_deal_check([r[0] for r in reach], [r[1] for r in reach], b"".join(r[2] for r in reach), folded, ns, T)
    assert [int(o) for o in dok] == [int(r[5] == K.OK) for r in reach] and not dst.any()


# ------------------------------------------------------------------------------------------------------------ end to end
def test_dss_end_to_end_over_rabin_dkg(ed):
    """7 participants, t = 4, three messages: a Rabin DKG for the long-term key and one per message, all on the device
    (dss_test.go's genDistSecret), partial signatures issued and checked by the batch entries; every Signature() verifies
    under sign/eddsa against DistKeyShare.Public() and all participants produce the same 64 bytes"""
    from kyber_amd.sign import dss, eddsa
    from kyber_amd.util import blake2xb
    from tests import _dkg_rabin_scenarios as DK

    MSGS = [b"", b"hello", bytes(range(200))]
    N, T_ = DK.N, DK.T
    kit = DK.Kit(False)
    w = DK.World(kit, b"dss end to end", N, T_)
    longs = DK.gen_dist_secret(kit, w)[1]
    randoms = [DK.gen_dist_secret(kit, w)[1] for _ in MSGS]
    assert len({k.Public().MarshalBinary() for k in longs}) == 1

    def world_nodes(seed):
        rand = blake2xb.New(seed)
        return [[dss.NewDSS(w.S, w.secrets[i], w.pubs, longs[i], randoms[b][i], m, T_, rand=rand) for b, m in enumerate(MSGS)] for i in range(N)]

    nodes = world_nodes(b"nonces")
    partials = [dss.PartialSigBatch(nodes[i]) for i in range(N)]  # ONE engine call per signer
    for i in range(N):
        pairs = [(nodes[i][b], partials[j][b]) for b in range(len(MSGS)) for j in range(N) if j != i]
        assert dss.process_partial_sigs(pairs) == [None] * len(pairs)  # ONE engine call per receiver
    public = longs[0].Public()
    for b, m in enumerate(MSGS):
        sigs = dss.SignatureBatch([nodes[i][b] for i in range(N)])
        assert len(set(sigs)) == 1 and len(sigs[0]) == 64
        assert eddsa.batch_verify_with_checks([public.MarshalBinary()], [m], [sigs[0]])[0]
        dss.Verify(public, m, sigs[0])
        assert not eddsa.batch_verify_with_checks([public.MarshalBinary()], [m + b"x"], [sigs[0]])[0]
    # the loop gives the same bytes as the batch entries under the same stream
    seq = world_nodes(b"nonces")
    for i in range(N):
        for b in range(len(MSGS)):
            ps = seq[i][b].PartialSig()
            assert (ps.Partial.V.MarshalBinary(), ps.SessionID, ps.Signature) == (partials[i][b].Partial.V.MarshalBinary(), partials[i][b].SessionID,
                                                                                  partials[i][b].Signature)
