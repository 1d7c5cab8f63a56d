"""Shuffles of sequences of ElGamal pairs, section 5 of Neff's paper (shuffle/sequences.go), over the batch engine:

  SequencesShuffle        sequences.go:36-124    NQ x k re-randomisations        -> one commit and one batch_add per base
  GetSequenceVerifiable   sequences.go:155-190   4 x NQ x k (Mul + Add)          -> batch_mul with the scalar replicated,
                                                                                    batch_add
X[j][i]: sequence element j of pair i, as an (NQ, k, 32) array (or nested sequences of 32-byte encodings).
"""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed
from ..proof import hash as H_
from . import _scalars as S
from .pair import PairShuffle

L = S.L


def _grid(M) -> np.ndarray:
    if isinstance(M, np.ndarray):
        return np.ascontiguousarray(M, dtype=np.uint8).reshape(M.shape[0], -1, 32)
    return np.stack([S.points(row) for row in M])


def _assert_xy(X: np.ndarray, Y: np.ndarray) -> None:
    if X.shape[0] == 0 or X.shape[1] == 0:
        raise ValueError("invalid data: array X is empty")
    if Y.shape[0] == 0 or Y.shape[1] == 0:
        raise ValueError("invalid data: array Y is empty")
    if X.shape != Y.shape:
        raise ValueError("invalid data: arrays X and Y have a different size")


def _random_int(mod: int, read) -> int:
    """random.Int (rand.go:36-46): Bits(BitLen(mod), false) big-endian, redrawn until below mod"""
    bits = mod.bit_length()
    while True:
        b = bytearray(read((bits + 7) // 8))
        if bits & 7:
            b[0] &= 0xFF >> (8 - (bits & 7))
        v = int.from_bytes(b, "big")
        if v < mod:
            return v


def GetSequenceVerifiable(group, X, Y, Xbar, Ybar, e):
    """(XUp, YUp, XDown, YDown): the consolidated inputs and outputs sum_j e[j] * M[j][i]; e: NQ scalars as (NQ, 32) rows"""
    e = S.points(e)

    def fold(M):
        M = _grid(M)
        NQ, k = M.shape[0], M.shape[1]
        prod = S.checked(ed.batch_mul(np.repeat(e[:NQ], k, axis=0), M.reshape(NQ * k, 32)), "sequence").reshape(NQ, k, 32)
        acc = prod[0]
        for j in range(1, NQ):
            acc = S.checked(ed.batch_add(acc, prod[j]), "sequence")
        return np.ascontiguousarray(acc)

    return fold(X), fold(Y), fold(Xbar), fold(Ybar)


def SequencesShuffle(group, G, H, X, Y, rand):
    """(xBar, yBar, getProver): one permutation for all NQ sequences, a fresh blinding factor per element;
    getProver(e), e the verifier's NQ scalars as (NQ, 32) rows, returns the prover of the consolidated pair shuffle."""
    X, Y = _grid(X), _grid(Y)
    _assert_xy(X, Y)
    NQ, k = X.shape[0], X.shape[1]
    G, H = S.point(G), S.point(H)
    read = H_._reader(rand)
    pi = list(range(k))
    for i in range(k - 1, 0, -1):  # Fisher-Yates
        j = _random_int(i + 1, read)
        if j != i:
            pi[i], pi[j] = pi[j], pi[i]
    beta = H_.picks(rand, NQ * k).reshape(NQ, k, 32)  # beta[j][i], sequence by sequence
    bp = np.ascontiguousarray(beta[:, pi]).reshape(NQ * k, 32)
    xbar = S.checked(ed.batch_add(S.mul_g(bp, G), np.ascontiguousarray(X[:, pi]).reshape(NQ * k, 32)), "X").reshape(NQ, k, 32)
    ybar = S.checked(ed.batch_add(S.mul_g(bp, H), np.ascontiguousarray(Y[:, pi]).reshape(NQ * k, 32)), "Y").reshape(NQ, k, 32)
    bint = [S.ints(beta[j]) for j in range(NQ)]

    def getProver(e):
        e = S.points(e)
        if e.shape[0] != NQ:
            raise ValueError(f"len(e) must be equal to NQ: {e.shape[0]} != {NQ}")
        ps = PairShuffle().Init(group, k)
        ev = S.ints(e)

        def prover(ctx):
            beta2 = [sum(ev[j] * bint[j][i] for j in range(NQ)) % L for i in range(k)]
            XUp, YUp, _, _ = GetSequenceVerifiable(group, X, Y, xbar, ybar, e)
            ps.Prove(pi, G, H, beta2, XUp, YUp, rand, ctx)

        return prover

    return xbar, ybar, getProver
