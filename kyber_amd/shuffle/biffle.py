"""Host-side mirror of the reference's binary shuffle (shuffle/biffle.go), function for function, over the predicates
of kyber_amd/proof/proof.py:

  bifflePred, bifflePoints        biffle.go:11-46   -> _pred, _points
  Biffle, BiffleVerifier          biffle.go:49-91   -> Biffle, BiffleVerifier
  the same over n independent pairs of ciphertexts with shared G, H        -> BiffleBatch, BiffleVerifyBatch

Points are 32 bytes, or (n, 2, 32) arrays in the batch calls; G None is the standard base (biffle_test.go:41).  The
differences Xbar_i - X_j are one batch_add of negated points (a negation flips the sign bit of a canonical encoding
with x != 0; the engine's add decodes either)."""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed
from ..proof import hash as PH
from ..proof import proof as P
from ..util import blake2xb

L = ed.ORDER


def _pred():
    R = P.Rep
    and0 = P.And(R("Xbar0-X0", "beta0", "G"), R("Ybar0-Y0", "beta0", "H"), R("Xbar1-X1", "beta1", "G"), R("Ybar1-Y1", "beta1", "H"))
    and1 = P.And(R("Xbar0-X1", "beta1", "G"), R("Ybar0-Y1", "beta1", "H"), R("Xbar1-X0", "beta0", "G"), R("Ybar1-Y0", "beta0", "H"))
    return P.Or(and0, and1)


def _sub(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a[i] - b[i] on (n, 32) encodings: Point.Sub (point.go:225-233)"""
    neg = np.array(b, dtype=np.uint8, copy=True)
    neg[:, 31] ^= 0x80
    out, st = ed.batch_add(a, neg)
    if np.asarray(st).any():
        raise PH.ProofError(PH.ErrPoint)
    return np.asarray(out)


def _points(G, H, X, Y, Xbar, Ybar):
    """X, Y, Xbar, Ybar: (n, 2, 32) arrays"""
    pts = {"G": G, "H": H}
    for i in range(2):
        for j in range(2):
            pts[f"Xbar{i}-X{j}"] = _sub(np.ascontiguousarray(Xbar[:, i]), np.ascontiguousarray(X[:, j]))
            pts[f"Ybar{i}-Y{j}"] = _sub(np.ascontiguousarray(Ybar[:, i]), np.ascontiguousarray(Y[:, j]))
    return pts


def _pairs(x) -> np.ndarray:
    if isinstance(x, np.ndarray):
        return x.reshape(-1, 2, 32)
    return np.frombuffer(b"".join(bytes(e) for e in x), dtype=np.uint8).reshape(1, 2, 32).copy()


def _outputs(G, H, X, Y, bits, betas):
    """Xbar[i] = beta[i ^ bit] G + X[i ^ bit], Ybar likewise with H (biffle.go:65-71), over n pairs"""
    n = X.shape[0]
    one = np.zeros((n, 32), dtype=np.uint8)
    one[:, 0] = 1
    Xbar, Ybar = np.zeros_like(X), np.zeros_like(Y)
    for i in range(2):
        pi = [i ^ b for b in bits]
        beta = np.frombuffer(b"".join(P._sc(betas[k][pi[k]]) for k in range(n)), dtype=np.uint8).reshape(n, 32).copy()
        for base, src, dst in ((G, X, Xbar), (H, Y, Ybar)):
            own = np.ascontiguousarray(src[np.arange(n), pi])
            out, _, st = P.lincomb(n, [(beta, P._pt(base)), (one, own)])
            if np.asarray(st).any():
                raise PH.ProofError(PH.ErrPoint)
            dst[:, i] = np.asarray(out)
    return Xbar, Ybar


def _draw(rand):
    """the single-bit permutation (random.Bytes of one byte) and the two blinding factors, in the reference's order"""
    read = PH._reader(rand)
    bit = (rand.XORKeyStream(bytes(1))[0] if hasattr(rand, "XORKeyStream") else read(1)[0]) & 1
    return bit, [blake2xb.pick_int(read)[0] for _ in range(2)]


def Biffle(suite, G, H, X, Y, rand):
    """(Xbar, Ybar, prover) for two ciphertexts (X[i], Y[i]): biffle.go:49-81"""
    bit, beta = _draw(rand)
    Xs, Ys = _pairs(X), _pairs(Y)
    Xbar, Ybar = _outputs(G, H, Xs, Ys, [bit], [beta])
    pred = _pred()
    pts = {k: (v[0].tobytes() if isinstance(v, np.ndarray) else v) for k, v in _points(G, H, Xs, Ys, Xbar, Ybar).items()}
    prover = pred.Prover(suite, {"beta0": beta[0], "beta1": beta[1]}, pts, {pred: bit})
    return [Xbar[0, 0].tobytes(), Xbar[0, 1].tobytes()], [Ybar[0, 0].tobytes(), Ybar[0, 1].tobytes()], prover


def BiffleVerifier(suite, G, H, X, Y, Xbar, Ybar):
    """biffle.go:84-91"""
    pts = _points(G, H, _pairs(X), _pairs(Y), _pairs(Xbar), _pairs(Ybar))
    return _pred().Verifier(suite, {k: (v[0].tobytes() if isinstance(v, np.ndarray) else v) for k, v in pts.items()})


def BiffleBatch(G, H, X, Y, rands, protocolName="Biffle"):
    """(Xbar, Ybar, proofs) for n independent pairs with shared G, H: X, Y (n, 2, 32); rands one BLAKE2Xb stream per
    pair, which serves the bit, the blinding factors and the prover's private draws as suite.RandomStream() does in
    the reference's test.  Proof i equals HashProve of Biffle(...) under rands[i]."""
    X, Y = _pairs(X), _pairs(Y)
    draws = [_draw(r) for r in rands]
    bits, betas = [d[0] for d in draws], [d[1] for d in draws]
    Xbar, Ybar = _outputs(G, H, X, Y, bits, betas)
    pred = _pred()
    n = X.shape[0]
    col = lambda j: np.frombuffer(b"".join(P._sc(b[j]) for b in betas), dtype=np.uint8).reshape(n, 32).copy()
    proofs = P.HashProveBatch(protocolName, pred, {"beta0": col(0), "beta1": col(1)}, _points(G, H, X, Y, Xbar, Ybar),
                              [{pred: b} for b in bits], rands)
    return Xbar, Ybar, proofs


def BiffleVerifyBatch(G, H, X, Y, Xbar, Ybar, proofs, protocolName="Biffle"):
    """a list with None or the ProofError of each of the n pairs (proof.HashVerifyBatch)"""
    return P.HashVerifyBatch(protocolName, _pred(), _points(G, H, _pairs(X), _pairs(Y), _pairs(Xbar), _pairs(Ybar)), proofs)
