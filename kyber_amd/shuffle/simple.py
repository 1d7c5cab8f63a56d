"""The simple k-shuffle of Neff, "Verifiable Mixing (Shuffling) of ElGamal Pairs", section 3 (shuffle/simple.go),
function for function over the batch engine:

  SimpleShuffle.Init     simple.go:76-83
  SimpleShuffle.Prove    simple.go:91-173    4k multiples of g                         -> two commits; the scalar vectors
                                                                                          (running products, Div) on the host
  SimpleShuffle.Verify   simple.go:186-254   2k thver (two Muls and an Add each)       -> ONE kyb_ed25519_theta_check for the k
                                                                                          checks with per-element bases; the k
                                                                                          with batch-wide bases on the fixed-base calls
"""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed
from ..proof.hash import ProofError
from . import _scalars as S

L = S.L
ErrIncorrect = "incorrect SimpleShuffleProof"
ErrMalformed = "malformed SimpleShuffleProof"


class SimpleShuffle:
    def Init(self, grp, k: int) -> "SimpleShuffle":
        self.grp, self.k = grp, int(k)
        return self

    def Prove(self, G, gamma: int, x, y, rand, ctx) -> None:
        """x, y: the scalar vectors as integers, y a permutation of x times gamma.  rand is unused, as in the reference
        (the private draws come from the context)."""
        k = len(x)
        if k <= 1:
            raise ValueError("can't shuffle length 1 vector")
        if k != len(y):
            raise ValueError("mismatched vector lengths")
        G = S.point(G)
        XY = S.mul_g(S.rows(list(x) + list(y)), G)  # (4)
        ctx.Put(XY[:k], XY[k:])
        t = S.ints(ctx.PubRand(1))[0]
        gamma_t = gamma * t % L
        xhat = [(v - t) % L for v in x]  # (5)
        yhat = [(v - gamma_t) % L for v in y]  # (6)
        thlen = 2 * k - 1
        theta = S.ints(ctx.PriRand(thlen)[0])  # (7)
        e = [-theta[0] * yhat[0]]
        e += [theta[i - 1] * xhat[i] - theta[i] * yhat[i] for i in range(1, k)]
        e += [theta[i - 1] * gamma - theta[i] for i in range(k, thlen)]
        e.append(theta[thlen - 1] * gamma)
        ctx.Put(S.mul_g(S.rows(e), G))
        c = S.ints(ctx.PubRand(1))[0]
        yinv = S.inv_all(yhat)
        alpha = [0] * thlen
        runprod = c
        for i in range(k):  # (8)
            runprod = runprod * xhat[i] % L * yinv[i] % L
            alpha[i] = theta[i] + runprod
        gammainv = pow(gamma % L, L - 2, L)
        rungamma = c
        for i in range(1, k):
            rungamma = rungamma * gammainv % L
            alpha[thlen - i] = theta[thlen - i] + rungamma
        ctx.Put(S.rows(alpha))

    def Verify(self, G, Gamma, ctx) -> None:
        """raises ProofError; Gamma: 32 bytes (or a (1, 32) array that ctx.CheckPoints canonicalises)"""
        k = self.k
        thlen = 2 * k - 1
        if k <= 1:
            raise ProofError(ErrMalformed)
        G = S.point(G)
        X, Y = ctx.Get(("P", k), ("P", k))
        t = S.ints(ctx.PubRand(1))[0]
        (Theta,) = ctx.Get(("P", thlen + 1))
        c = ctx.PubRand(1)
        (alpha,) = ctx.Get(("S", thlen))
        check = getattr(ctx, "CheckPoints", None)
        if check is not None:  # every transcript point in one batch_unmarshal
            check()
        if X.shape[0] != k or Y.shape[0] != k or Theta.shape[0] != thlen + 1 or alpha.shape[0] != thlen:
            raise ProofError(ErrMalformed)
        Gamma = S.points(Gamma)
        negt = S.rows([-t])
        U = S.mul_g(negt, G)
        W = S.checked(ed.batch_mul(negt, Gamma), "Gamma")
        # step 5, the k checks on (Xhat_i, Yhat_i): a = (c, alpha_0 .. alpha_{k-2}), b = (alpha_0 .. alpha_{k-1})
        ok, st = ed.batch_theta_check(np.concatenate([c, alpha[:k - 1]]), X, U, alpha[:k], Y, W, Theta[:k])
        good = not np.asarray(st).any() and bool(np.asarray(ok).all())
        # the k checks on (Gamma, G): alpha_{i-1} Gamma - alpha_i G == Theta_i, the last with c for alpha_{2k-1}
        nb = S.rows([-v for v in S.ints(alpha[k:]) + S.ints(c)])
        lhs = S.checked(ed.batch_add(np.asarray(ed.commit(alpha[k - 1:], Gamma.tobytes())), S.mul_g(nb, G)), "Theta")
        good = good and bool((lhs == Theta[k:]).all())
        if not good:
            raise ProofError(ErrIncorrect)
