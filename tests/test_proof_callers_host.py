"""kyber_amd/proof/proof.py and kyber_amd/shuffle/biffle.py without a GPU: the three engine calls they make
(batch_lincomb, batch_fs_challenge, batch_unmarshal, and batch_add for biffle's differences) are replaced by the oracle
behind the wrappers' signatures, as tests/test_callers_host.py does for share/poly; everything else is the product's code.
Checked: the four printed proofs and the six strings, TestRep, every error message, proofs truncated at every 32-byte
boundary, trailing bytes, and the batch calls against the sequential ones."""
import numpy as np
import pytest

from kyber_amd.util import blake2xb as X
from oracle import ed25519 as O
from tests import _proof_cases as PC
from tests import _proof_oracle as PO
from tests import _shuffle_oracle as SO
from tests.test_proof_host import fs_challenge
from tests.test_proof_oracle import GOLD, example


def stand_ins(monkeypatch):
    from kyber_amd.group import edwards25519 as ed

    def batch_lincomb(scalars, own, shared, expect=None, want_out=True, vartime=False):
        n, k = scalars.shape[0], scalars.shape[1]
        ko = own.shape[1] if own is not None else 0
        mask = sum(1 << j for j, p in enumerate(shared) if p is None)
        sh = [bytes(32) if p is None else bytes(p) for p in shared]
        vals = [PC.value(ko, len(shared), mask, sh, [scalars[i, j].tobytes() for j in range(k)],
                         [own[i, j].tobytes() for j in range(ko)], vartime) for i in range(n)]
        out = np.frombuffer(b"".join(v or bytes(32) for v in vals), dtype=np.uint8).reshape(n, 32).copy()
        st = np.array([v is None for v in vals], dtype=np.uint8)
        ok = None
        if expect is not None:
            ok = np.array([PC.verdict(v, np.asarray(expect)[i].tobytes())[0] for i, v in enumerate(vals)], dtype=np.uint8)
        return (out if want_out else None), ok, st

    def batch_fs_challenge(names, data):
        data = np.asarray(data)
        name = lambda i: names if isinstance(names, (bytes, bytearray)) else names[i]
        c = b"".join(fs_challenge(bytes(name(i)), data[i].tobytes()) for i in range(data.shape[0]))
        return np.frombuffer(c, dtype=np.uint8).reshape(-1, 32).copy(), np.zeros(data.shape[0], dtype=np.uint8)

    def batch_unmarshal(points):
        pts = np.asarray(points).reshape(-1, 32)
        dec = [O.decode(p.tobytes()) for p in pts]
        out = np.frombuffer(b"".join(O.encode(d) if d else bytes(32) for d in dec), dtype=np.uint8).reshape(-1, 32).copy()
        return out, np.array([d is None for d in dec], dtype=np.uint8)

    def batch_add(a, b):
        pa, st_a = batch_unmarshal(a)
        pb, st_b = batch_unmarshal(b)
        out = [SO.padd(x.tobytes(), y.tobytes()) if not (s or t) else bytes(32) for x, y, s, t in zip(pa, pb, st_a, st_b)]
        return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 32).copy(), st_a | st_b

    for name, f in (("batch_lincomb", batch_lincomb), ("batch_fs_challenge", batch_fs_challenge), ("batch_unmarshal", batch_unmarshal),
                    ("batch_add", batch_add)):
        monkeypatch.setattr(ed, name, f)
    from kyber_amd.proof import hash as PH
    from kyber_amd.proof import proof as P

    return P, PH


def product_pred(P, p, choice, out=None):
    """the oracle's predicate tuples as the product's objects; ({oracle id: object}, choice map)"""
    out = {} if out is None else out
    obj = P.Rep(p[1], *[x for t in p[2] for x in t]) if p[0] == "rep" else (P.And if p[0] == "and" else P.Or)(
        *[product_pred(P, q, choice, out)[0] for q in p[1]])
    out[id(p)] = obj
    return obj, {out[k]: v for k, v in (choice or {}).items() if k in out}


def msg(err):
    return None if err is None else str(err)


def verify_one(P, PH, name, pred, pval, proof):
    try:
        PH.HashVerify(PH.Suite(X.New(b"v")), name, pred.Verifier(None, pval), proof)
    except PH.ProofError as e:
        return str(e)
    return None


@pytest.mark.parametrize("which", ["rep2", "or2", "hashProve1", "hashProve2"])
def test_the_printed_proofs(monkeypatch, which):
    P, PH = stand_ins(monkeypatch)
    name, opred, sval, pval, choice, rand = example(which)
    pred, ch = product_pred(P, opred, choice)
    assert pred.String() == PO.string(opred)
    proof = PH.HashProve(PH.Suite(rand), name, pred.Prover(None, sval, pval, ch))
    assert proof.hex() == GOLD[which]["proof"]
    assert verify_one(P, PH, name, pred, pval, proof) is None
    assert verify_one(P, PH, name, pred, pval, proof + b"trailing bytes are ignored") is None
    # the batch calls: n = 1, and the golden proof planted among others
    name, opred, sval, pval, choice, rand = example(which)
    assert P.HashProveBatch(name, pred, sval, pval, ch, [rand]) == [proof]
    rands = [X.New(b"other %d" % i) for i in range(2)] + [example(which)[5]] + [X.New(b"last")]
    proofs = P.HashProveBatch(name, pred, sval, pval, ch, rands)
    assert proofs[2] == proof and len(set(proofs)) == 4
    assert P.HashVerifyBatch(name, pred, pval, proofs) == [None] * 4
    if which == "hashProve1":
        wrong = GOLD[which]["wrong_name"].encode()
        assert verify_one(P, PH, wrong, pred, pval, proof) == GOLD[which]["wrong_name_error"] == P.ErrCommit
        assert [msg(e) for e in P.HashVerifyBatch([name, wrong, name, wrong], pred, pval, proofs)] == [None, P.ErrCommit, None, P.ErrCommit]
    # truncated at every 32-byte boundary; an undecodable commitment before the end wins
    for cut in range(0, len(proof), 32):
        want = PO.hash_verify(name, opred, pval, proof[:cut])
        assert want == SO.ERR_SHORT and verify_one(P, PH, name, pred, pval, proof[:cut]) == want, cut
    bad = PC.OFF_CURVE + proof[32:]
    for cut in (32, 64, len(proof)):
        assert verify_one(P, PH, name, pred, pval, bad[:cut]) == SO.ERR_POINT == PO.hash_verify(name, opred, pval, bad[:cut])
    got = P.HashVerifyBatch(name, pred, pval, [proof, proof[:-32], bad, proof + b"x", proof[:31]])
    assert [msg(e) for e in got] == [None, SO.ERR_SHORT, SO.ERR_POINT, None, SO.ERR_SHORT]


def test_strings_and_constructors(monkeypatch):
    P, _ = stand_ins(monkeypatch)
    s = GOLD["strings"]
    R, A, Or = P.Rep, P.And, P.Or
    assert R("X", "x", "B").String() == s["rep1"] and R("X", "x1", "B1", "x2", "B2").String() == s["rep3"]
    assert A(R("X", "x", "B"), R("Y", "y", "B")).String() == s["and1"] and A(R("X1", "x", "B1"), R("X2", "x", "B2")).String() == s["and2"]
    assert Or(R("X", "x", "B"), R("Y", "y", "B")).String() == s["or1"]
    assert Or(*[A(R(f"X[{i}]", "x", "B"), R("T", "x", "BT")) for i in range(3)]).String() == s["hashProve2"]
    with pytest.raises(ValueError, match="mismatched Scalar"):
        R("X", "x")


def test_rep_nested_predicate_and_every_tampered_field(monkeypatch):
    """TestRep (proof_test.go:13-67), then each 32-byte field of its proof tampered: the product's message is the oracle's,
    sequentially and in a batch"""
    P, PH = stand_ins(monkeypatch)
    opred, sval, pval, choice, rand = PO.rep_case()
    pred, ch = product_pred(P, opred, choice)
    proof = PH.HashProve(PH.Suite(rand), b"TEST", pred.Prover(None, sval, pval, ch))
    assert proof == PO.hash_prove(b"TEST", *PO.rep_case()[:4], PO.rep_case()[4])
    assert verify_one(P, PH, b"TEST", pred, pval, proof) is None
    tampered, want = [], []
    for at in range(0, len(proof), 32):
        t = bytearray(proof)
        t[at] ^= 1
        tampered.append(bytes(t))
        want.append(PO.hash_verify(b"TEST", opred, pval, bytes(t)))
        assert verify_one(P, PH, b"TEST", pred, pval, bytes(t)) == want[-1], at
    unreduced = proof[:-32] + (SO.le(proof[-32:]) + PO.L).to_bytes(32, "little")  # a response plus l: read raw, same product
    tampered.append(unreduced)
    want.append(PO.hash_verify(b"TEST", opred, pval, unreduced))
    assert want[-1] is None and {PO.ERR_COMMIT, PO.ERR_SUB} <= set(want)
    assert [msg(e) for e in P.HashVerifyBatch(b"TEST", pred, pval, tampered)] == want


def test_error_messages(monkeypatch):
    P, PH = stand_ins(monkeypatch)
    rand = X.New(b"errors")
    x = SO.pick(rand.Read)
    pval = {"B": PO.BASE, "X": SO.pmul(SO.sc(x), None), "Y": PO.point_pick(rand)}
    orp = P.Or(P.Rep("X", "x", "B"), P.Rep("Y", "y", "B"))
    prove = lambda pred, ch: PH.HashProve(PH.Suite(rand), b"T", pred.Prover(None, {"x": x}, pval, ch))
    with pytest.raises(PH.ProofError) as e:
        prove(orp, {})
    assert str(e.value) == "no choice of proof branch for OR-predicate X=x*B || Y=y*B"
    with pytest.raises(PH.ProofError) as e:
        prove(orp, {orp: 2})
    assert str(e.value).startswith(P.ErrNoChoice)
    with pytest.raises(PH.ProofError) as e:
        prove(P.And(orp), {orp: 0})
    assert str(e.value) == "can't have OR predicates within AND predicates"
    proof = prove(orp, {orp: 0})
    t = bytearray(proof)
    t[64] ^= 1
    assert verify_one(P, PH, b"T", orp, pval, bytes(t)) == "invalid proof: bad sub-challenges"
    t = bytearray(proof)
    t[-1] ^= 1
    assert verify_one(P, PH, b"T", orp, pval, bytes(t)) == "invalid proof: commit mismatch"
    assert verify_one(P, PH, b"T", P.And(orp), pval, proof) == P.ErrOrNestedVerify
    # respond's own message (proof.go:545) is reached only past commit, which rejects the same nesting first
    walk = P._Prover(orp, {"x": x}, {orp: 0}, lambda: 1, lambda *a: None)
    walk.commit(orp, None, None)
    with pytest.raises(PH.ProofError) as e:
        walk.respond(orp, 5, [None] * 3, lambda xs: None)
    assert str(e.value) == "OR predicates can't be nested in anything else"


@pytest.mark.parametrize("G", [None, "given"])
def test_biffle_sequential_and_batch_against_the_oracle(monkeypatch, G):
    P, PH = stand_ins(monkeypatch)
    from kyber_amd.shuffle import biffle as B

    setup = X.New(b"biffle host")
    if G is not None:
        G = PO.point_pick(setup)
    H = SO.pmul(SO.sc(SO.pick(setup.Read)), G)
    n = 5
    Xs, Ys = [], []
    for _ in range(n):
        pair = []
        for _ in range(2):
            r = SO.sc(SO.pick(setup.Read))
            pair.append((SO.pmul(r, G), SO.padd(SO.pmul(r, H), PO.point_pick(setup))))
        Xs.append([p[0] for p in pair])
        Ys.append([p[1] for p in pair])
    want = []
    for i in range(n):
        rand = X.New(b"pair %d" % i)
        Xbar, Ybar, prv = PO.biffle(G, H, Xs[i], Ys[i], rand)
        want.append((Xbar, Ybar, SO.hash_prove(b"Biffle", prv, rand.Read)))
    # sequential
    rand = X.New(b"pair 0")
    Xbar, Ybar, prv = B.Biffle(None, G, H, Xs[0], Ys[0], rand)
    proof = PH.HashProve(PH.Suite(rand), "Biffle", prv)
    assert (Xbar, Ybar, proof) == want[0]
    PH.HashVerify(PH.Suite(), "Biffle", B.BiffleVerifier(None, G, H, Xs[0], Ys[0], Xbar, Ybar), proof)
    # batch
    arr = lambda rows: np.frombuffer(b"".join(b"".join(r) for r in rows), dtype=np.uint8).reshape(len(rows), 2, 32).copy()
    Xb, Yb, proofs = B.BiffleBatch(G, H, arr(Xs), arr(Ys), [X.New(b"pair %d" % i) for i in range(n)])
    assert [([Xb[i, 0].tobytes(), Xb[i, 1].tobytes()], [Yb[i, 0].tobytes(), Yb[i, 1].tobytes()], proofs[i]) for i in range(n)] == want
    assert B.BiffleVerifyBatch(G, H, arr(Xs), arr(Ys), Xb, Yb, proofs) == [None] * n
    # TestInvalidBiffle: an output replaced
    Xb[3, 0] = np.frombuffer(SO.pmul(SO.sc(7), None), dtype=np.uint8)
    got = B.BiffleVerifyBatch(G, H, arr(Xs), arr(Ys), Xb, Yb, proofs)
    assert [msg(e) for e in got] == [None, None, None, P.ErrCommit, None]
    assert SO.hash_verify(b"Biffle", PO.biffle_verifier(G, H, Xs[3], Ys[3], [Xb[3, 0].tobytes(), want[3][0][1]], want[3][1]), proofs[3]) == PO.ERR_COMMIT
