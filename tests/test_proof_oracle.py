"""The sequential restatement of proof.go and biffle.go (tests/_proof_oracle.py) against what the reference's own tests
print (tests/golden/proof_examples.json: the four proofs of Example_rep2, Example_or2, Example_hashProve1 and
Example_hashProve2 and the six predicate strings), TestRep's nested predicate, TestBiffle and TestInvalidBiffle."""
import json
import os

import pytest

from kyber_amd.util import blake2xb as X
from tests import _proof_oracle as PO
from tests import _shuffle_oracle as SO

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proof_examples.json")))


def example(which):
    """(name, predicate, secrets, points, choice) of one printed example, under blake2xb.New("example") as the reference
    builds it; the stream is left where the prover's PriRand continues"""
    rand = X.New(b"example")
    x = SO.pick(rand.Read)
    Xp = SO.pmul(SO.sc(x), None)
    if which in ("rep2", "hashProve1"):
        return GOLD[which]["name"].encode(), PO.Rep("X", "x", "B"), {"x": x}, {"B": PO.BASE, "X": Xp}, None, rand
    if which == "or2":
        pred = PO.Or(PO.Rep("X", "x", "B"), PO.Rep("Y", "y", "B"))
        return b"TEST", pred, {"x": x}, {"B": PO.BASE, "X": Xp, "Y": PO.point_pick(rand)}, {id(pred): 0}, rand
    assert which == "hashProve2"  # hash_test.go:78-135: three random points first, then the key
    rand = X.New(b"example")
    ring = [PO.point_pick(rand) for _ in range(3)]
    x = SO.pick(rand.Read)
    ring[2] = SO.pmul(SO.sc(x), None)
    link_base = PO.point_pick(X.New(b"The Linkage Scope"))
    pts = {"B": PO.BASE, "BT": link_base, "T": SO.pmul(SO.sc(x), link_base)}
    for i, p in enumerate(ring):
        pts[f"X[{i}]"] = p
    pred = PO.Or(*[PO.And(PO.Rep(f"X[{i}]", "x", "B"), PO.Rep("T", "x", "BT")) for i in range(3)])
    return b"Hello World!", pred, {"x": x}, pts, {id(pred): 2}, rand


@pytest.mark.parametrize("which", ["rep2", "or2", "hashProve1", "hashProve2"])
def test_the_oracle_reproduces_and_verifies_the_printed_proofs(which):
    name, pred, sval, pval, choice, rand = example(which)
    proof = PO.hash_prove(name, pred, sval, pval, choice, rand)
    assert proof.hex() == GOLD[which]["proof"]
    assert PO.hash_verify(name, pred, pval, proof) is None
    if which == "hashProve1":
        assert PO.hash_verify(GOLD[which]["wrong_name"].encode(), pred, pval, proof) == GOLD[which]["wrong_name_error"]
    if which == "hashProve2":
        assert PO.string(pred) == GOLD["strings"]["hashProve2"]


def test_predicate_strings():
    R, A, Or = PO.Rep, PO.And, PO.Or
    s = GOLD["strings"]
    assert PO.string(R("X", "x", "B")) == s["rep1"]
    assert PO.string(R("X", "x1", "B1", "x2", "B2")) == s["rep3"]
    assert PO.string(A(R("X", "x", "B"), R("Y", "y", "B"))) == s["and1"]
    assert PO.string(A(R("X1", "x", "B1"), R("X2", "x", "B2"))) == s["and2"]
    assert PO.string(Or(R("X", "x", "B"), R("Y", "y", "B"))) == s["or1"]
    assert PO.string(A(Or(R("X", "x", "B"), R("Y", "y", "B")), R("Z", "z", "B"))) == "(X=x*B || Y=y*B) && Z=z*B"
    with pytest.raises(ValueError, match="mismatched Scalar"):
        R("X", "x")


def test_rep_nested_predicate():
    """TestRep (proof_test.go:13-67)"""
    pred, sval, pval, choice, rand = PO.rep_case()
    proof = PO.hash_prove(b"TEST", pred, sval, pval, choice, rand)
    assert PO.hash_verify(b"TEST", pred, pval, proof) is None
    assert PO.hash_verify(b"TEST", pred, pval, proof[:-32]) == SO.ERR_SHORT
    bad = bytearray(proof)
    bad[-1] ^= 1
    assert PO.hash_verify(b"TEST", pred, pval, bytes(bad)) == PO.ERR_COMMIT


def test_error_messages():
    R = PO.Rep
    rand = X.New(b"errors")
    x = SO.pick(rand.Read)
    pval = {"B": PO.BASE, "X": SO.pmul(SO.sc(x), None), "Y": PO.point_pick(rand)}
    orp = PO.Or(R("X", "x", "B"), R("Y", "y", "B"))
    with pytest.raises(PO.ProofError, match="no choice of proof branch for OR-predicate X=x\\*B \\|\\| Y=y\\*B"):
        PO.hash_prove(b"T", orp, {"x": x}, pval, {}, rand)
    with pytest.raises(PO.ProofError, match=PO.ERR_OR_IN_AND):
        PO.hash_prove(b"T", PO.And(orp), {"x": x}, pval, {id(orp): 0}, rand)
    proof = PO.hash_prove(b"T", orp, {"x": x}, pval, {id(orp): 0}, rand)
    assert PO.hash_verify(b"T", orp, pval, proof) is None
    bad = bytearray(proof)
    bad[64] ^= 1  # the first sub-challenge
    assert PO.hash_verify(b"T", orp, pval, bytes(bad)) == PO.ERR_SUB
    assert PO.hash_verify(b"T", PO.And(orp), pval, proof) == PO.ERR_OR_NESTED_V


@pytest.mark.parametrize("G", [None, "given"])
def test_biffle_and_invalid_biffle(G):
    """TestBiffle / TestInvalidBiffle (biffle_test.go): G = nil in the reference's test"""
    rand = X.New(b"biffle")
    if G is not None:
        G = PO.point_pick(rand)
    h = SO.pick(rand.Read)
    H = SO.pmul(SO.sc(h), G)
    pts = []
    for _ in range(2):
        r = SO.sc(SO.pick(rand.Read))
        pts.append((SO.pmul(r, G), SO.padd(SO.pmul(r, H), PO.point_pick(rand))))
    Xs, Ys = [p[0] for p in pts], [p[1] for p in pts]
    for _ in range(4):  # both bits
        Xbar, Ybar, prv = PO.biffle(G, H, Xs, Ys, rand)
        proof = SO.hash_prove(b"Biffle", prv, rand.Read)
        assert SO.hash_verify(b"Biffle", PO.biffle_verifier(G, H, Xs, Ys, Xbar, Ybar), proof) is None
        # TestInvalidBiffle: one output replaced
        Xbad = [SO.pmul(SO.sc(7), None), Xbar[1]]
        assert SO.hash_verify(b"Biffle", PO.biffle_verifier(G, H, Xs, Ys, Xbad, Ybar), proof) == PO.ERR_COMMIT
