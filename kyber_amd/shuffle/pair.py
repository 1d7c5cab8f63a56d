"""The ElGamal pair shuffle of Neff, "Verifiable Mixing (Shuffling) of ElGamal Pairs", section 4 (shuffle/pair.go),
function for function over the batch engine:

  PairShuffle.Init      pair.go:105-124
  PairShuffle.Prove     pair.go:129-236   5k + 1 multiples of G, two k-term sums, the simple k-shuffle's 4k
                                          -> commits, two MSMs, scalar vectors on the host
  PairShuffle.Verify    pair.go:239-312   -> one batch_unmarshal over the transcript's points, the four challenges on the
                                             engine, SimpleShuffle.Verify, (33) as one same-base product and one batch_add,
                                             Phi1 and Phi2 as two MSMs of 2k terms
  Shuffle, Verifier     pair.go:318-377

G or H None is the standard base: Mul(s, nil) is the base-point multiplication and goes through mul_base, a given point
through mul_same_base.  alpha, sigma and tau come off the wire unreduced and multiply as such.  The B[i] of
pair.go:261-265 are dead code in the reference and are not computed.
"""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed
from ..proof import hash as H_
from . import _scalars as S
from .simple import SimpleShuffle

L = S.L
ErrInvalid = "invalid PairShuffleProof"


def _neg_points(P: np.ndarray) -> np.ndarray:
    """-P on the encodings: the other sign of x (Point.Sub negates the point exactly, point.go:209-221)"""
    out = P.copy()
    out[:, 31] ^= 0x80
    return out


def _msm(scalars, points, what: str) -> np.ndarray:
    return S.checked(ed.msm(np.ascontiguousarray(scalars), np.ascontiguousarray(points)), what).reshape(1, 32)


class PairShuffle:
    def Init(self, grp, k: int) -> "PairShuffle":
        if k <= 1:
            raise ValueError("can't shuffle permutation of size <= 1")
        self.grp, self.k = grp, int(k)
        self.pv6 = SimpleShuffle().Init(grp, k)
        return self

    def Prove(self, pi, G, H, beta, X, Y, rand, ctx) -> None:
        """pi: the permutation; beta: the blinding factors as integers; X, Y: (k, 32) points"""
        k = self.k
        if k != len(pi) or k != len(beta):
            raise ValueError("mismatched vector lengths")
        G, H = S.point(G), S.point(H)
        X, Y = S.points(X), S.points(Y)
        pi = [int(v) for v in pi]
        piinv = [0] * k
        for i in range(k):
            piinv[pi[i]] = i
        # P step 1: the private draws in the reference's order, then the commitments
        u, w, a, tau0, _nu, gamma = (S.ints(v) for v in ctx.PriRand(k, k, k, 1, 1, 1))
        tau0, gamma = tau0[0], gamma[0]
        wbetasum = (tau0 + sum(w[i] * beta[pi[i]] for i in range(k))) % L
        e = [gamma] + a + [gamma * a[pi[i]] for i in range(k)] + u + [gamma * w[i] for i in range(k)] + [wbetasum]
        m = S.mul_g(S.rows(e), G)  # Gamma, A, C, U, W and wbetasum G
        wu = S.rows(w[piinv[i]] - u[i] for i in range(k))
        Lambda1 = S.checked(ed.batch_add(_msm(wu, X, "X"), m[4 * k + 1:]), "Lambda1")
        Lambda2 = S.checked(ed.batch_add(_msm(wu, Y, "Y"), S.mul_g(S.rows([wbetasum]), H)), "Lambda2")
        ctx.Put(m[:4 * k + 1], Lambda1, Lambda2)
        # V step 2, P step 3
        rho = S.ints(ctx.PubRand(k))
        b = [(rho[i] - u[i]) % L for i in range(k)]
        ctx.Put(S.mul_g(S.rows(gamma * b[pi[i]] for i in range(k)), G))
        # V step 4, P step 5
        lam = S.ints(ctx.PubRand(1))[0]
        r = [(a[i] + lam * b[i]) % L for i in range(k)]
        s = [gamma * r[pi[i]] % L for i in range(k)]
        tau = (-tau0 + sum(b[i] * beta[i] for i in range(k))) % L
        ctx.Put(S.rows(w[i] + b[pi[i]] for i in range(k)), S.rows([tau]))
        # P, V step 6: the embedded simple k-shuffle
        self.pv6.Prove(G, gamma, r, s, rand, ctx)

    def Verify(self, G, H, X, Y, Xbar, Ybar, ctx) -> None:
        """raises ProofError with the reference's message"""
        k = self.k
        G, H = S.point(G), S.point(H)
        X, Y, Xbar, Ybar = (S.points(v) for v in (X, Y, Xbar, Ybar))
        if any(v.shape[0] != k for v in (X, Y, Xbar, Ybar)):
            raise ValueError("mismatched vector lengths")
        Gamma, _A, _C, _U, W, Lambda1, Lambda2 = ctx.Get(("P", 1), ("P", k), ("P", k), ("P", k), ("P", k), ("P", 1), ("P", 1))
        rho = ctx.PubRand(k)
        (D,) = ctx.Get(("P", k))
        ctx.PubRand(1)
        sigma, tau = ctx.Get(("S", k), ("S", 1))
        self.pv6.Verify(G, Gamma, ctx)  # its last Get decodes every point of the transcript
        # V step 7: (33), then (31), (32) against (34), (35)
        lhs = np.asarray(ed.commit(sigma, Gamma.tobytes()))
        rhs = S.checked(ed.batch_add(W, D), "W + D")
        if not (lhs == rhs).all():
            raise H_.ProofError(ErrInvalid)
        sr = np.concatenate([sigma, rho])
        Phi1 = _msm(sr, np.concatenate([Xbar, _neg_points(X)]), "X")
        Phi2 = _msm(sr, np.concatenate([Ybar, _neg_points(Y)]), "Y")
        want1 = S.checked(ed.batch_add(Lambda1, S.mul_g(tau, G)), "Lambda1")
        want2 = S.checked(ed.batch_add(Lambda2, S.mul_g(tau, H)), "Lambda2")
        if not (want1 == Phi1).all() or not (want2 == Phi2).all():
            raise H_.ProofError(ErrInvalid)


def _rand_uint64(read) -> int:
    return int.from_bytes(read(8), "big")  # random.Bits(64, false, rand), big-endian (pair.go:364-367)


def Shuffle(group, G, H, X, Y, rand):
    """(Xbar, Ybar, prover): a random permutation and fresh blinding factors from rand, the shuffled and re-randomised
    pairs, and the prover of their correctness (pair.go:318-361)."""
    X, Y = S.points(X), S.points(Y)
    k = X.shape[0]
    if k != Y.shape[0]:
        raise ValueError("X,Y vectors have inconsistent length")
    G, H = S.point(G), S.point(H)
    ps = PairShuffle().Init(group, k)
    read = H_._reader(rand)
    pi = list(range(k))
    for i in range(k - 1, 0, -1):
        j = _rand_uint64(read) % (i + 1)
        if j != i:
            pi[j], pi[i] = pi[i], pi[j]
    beta = H_.picks(rand, k)
    bp = beta[pi]
    Xbar = S.checked(ed.batch_add(S.mul_g(bp, G), X[pi]), "X")
    Ybar = S.checked(ed.batch_add(S.mul_g(bp, H), Y[pi]), "Y")
    beta = S.ints(beta)
    return Xbar, Ybar, lambda ctx: ps.Prove(pi, G, H, beta, X, Y, rand, ctx)


def Verifier(group, G, H, X, Y, Xbar, Ybar):
    """a Sigma-protocol verifier of the shuffle's correctness (pair.go:370-377)"""
    ps = PairShuffle().Init(group, len(S.points(X)))
    return lambda ctx: ps.Verify(G, H, X, Y, Xbar, Ybar, ctx)
