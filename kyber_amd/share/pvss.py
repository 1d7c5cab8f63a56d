"""Host-side mirror of ``share/pvss`` (Schoenmakers' publicly verifiable secret sharing, pvss.go) on Ed25519, function for
function, over the batch engine:

  EncShares             pvss.go:51-92     PriPoly.Shares + Commit + NewDLEQProofBatch     -> scalar_poly_eval, commit, batch_mul
  computeGlobalChallenge pvss.go:94-149   n Horner loops of t (Mul + Add), one hash       -> ONE poly_eval; the hash on the host
  VerifyEncShare(Batch) pvss.go:154-194   n x Proof.Verify under one expected challenge   -> ONE kyb_ed25519_dleq_verify (expect_c,
                                                                                             H shared: h stride 0 is G's slot here)
  DecShare(Batch)       pvss.go:199-244   verify, x^-1 * sX, NewDLEQProof per share       -> dleq_verify, ONE batch_mul,
                                                                                             batch_mul for the proofs,
                                                                                             ONE kyb_ed25519_dleq_challenge
  VerifyDecShare(Batch) pvss.go:248-299   n x (hash, Pick over BLAKE2Xb, Proof.Verify)    -> ONE kyb_ed25519_dleq_verify with
                                                                                             KYB_F_DLEQ_FS (G shared)
  RecoverSecret         pvss.go:303-323   VerifyDecShareBatch + RecoverCommit             -> the above + share.recover_commit (one MSM)

Points and scalars cross this interface as 32 wire bytes (or the edwards25519 mirrors, which hold the same bytes).  The
randomness the reference takes from suite.RandomStream() -- the polynomial's coefficients and the proofs' nonces -- comes
from a caller-supplied stream (``util.blake2xb.XOF`` or any callable returning n bytes).  None of these functions has a host
fallback for the group work: without the engine they raise.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .._lib import ST_DLEQ_CHALLENGE
from ..group import edwards25519 as ed
from ..proof import dleq
from ..util import blake2xb
from . import poly

# the reference's errors (pvss.go:34-39), by name
ErrTooFewShares = "not enough shares to recover secret"
ErrDifferentLengths = "inputs of different lengths"
ErrEncVerification = "verification of encrypted share failed"
ErrDecVerification = "verification of decrypted share failed"
ErrGlobalChallengeVerification = "failed to verify global challenge"
ErrDecShareChallengeVerification = "failed to verify the share decryption challenge"


class PVSSError(ValueError):
    """carries one of the Err* strings above in .err"""

    def __init__(self, err: str):
        super().__init__("didn't verify: " + err)
        self.err = err


class PubVerShare:
    """pvss.PubVerShare (pvss.go:42-45): S = share.PubShare{I, V}, P = dleq.Proof"""

    __slots__ = ("S", "P")

    def __init__(self, S: poly.PubShare, P: dleq.Proof):
        self.S, self.P = S, P


_SUITE = ed.NewSuite()
_BASE = ed._BASE_ENC


def _b(p) -> bytes:
    return p.MarshalBinary() if hasattr(p, "MarshalBinary") else bytes(p)


def _rows(items) -> np.ndarray:
    return np.frombuffer(b"".join(_b(e) for e in items), dtype=np.uint8).reshape(len(items), 32)


def _share(i: int, v, proof: dleq.Proof) -> PubVerShare:
    return PubVerShare(poly.PubShare(i, ed.Point(bytes(v))), proof)


def EncShares(H, X, secret, t: int, rand):
    """(shares, pubPoly) of pvss.go:51-92: the encrypted shares s_i X_i of p(i), i < n = len(X), with their consistency
    proofs under one collective challenge, and the commitments of p with respect to H"""
    n = len(X)
    sc = secret if isinstance(secret, ed.Scalar) else ed.Scalar(_b(secret))
    pri = poly.PriPoly(_SUITE, [sc] + [ed.Scalar().Pick(rand) for _ in range(t - 1)])  # share/poly.go:56-67
    pri_shares = pri.Shares(n)
    pub = pri.Commit(ed.Point(_b(H)))
    values = _rows([s.V for s in pri_shares])
    proofs, _, sX = dleq.NewDLEQProofBatch(np.tile(np.frombuffer(_b(H), dtype=np.uint8), (n, 1)), _rows(X), values, rand)
    return [_share(pri_shares[i].I, sX[i], proofs[i]) for i in range(n)], pub


def computeCommitments(n: int, polyComs) -> np.ndarray:
    """X_i = sum_j (i + 1)^j C_j for i < n (pvss.go:94-114): the reference's Horner loop yields the points of
    PubPoly.Eval, so this is one poly_eval call"""
    out, st = ed.poly_eval(b"".join(_b(c) for c in polyComs), list(range(n)))
    if np.asarray(st).any():
        raise ValueError("share: invalid commitment")
    return np.asarray(out)


def computeGlobalChallenge(n: int, commit: poly.PubPoly, encShares) -> bytes:
    """Pick(XOF(SHA-256(coms || all S.V || all VG || all VH))) (pvss.go:116-149); the one hash stays on the host"""
    _, coms = commit.Info()
    h = hashlib.sha256()
    h.update(computeCommitments(n, coms).tobytes())
    for part in ([_b(e.S.V) for e in encShares], [e.P.VG for e in encShares], [e.P.VH for e in encShares]):
        h.update(b"".join(part))
    return blake2xb.pick(blake2xb.New(h.digest()).Read)


def _verify_enc(H, X, sH, challenges, encShares):
    """(ok, status) of VerifyEncShare for every element; challenges: one expected challenge, or one per element"""
    n = len(encShares)
    if len(X) != n or len(sH) != n:
        raise PVSSError(ErrDifferentLengths)
    if n == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint8)
    C = _rows([e.P.C for e in encShares])
    args = (_b(H), _rows(X), _rows(sH), _rows([e.S.V for e in encShares]), C, _rows([e.P.R for e in encShares]),
            _rows([e.P.VG for e in encShares]), _rows([e.P.VH for e in encShares]))
    if isinstance(challenges, (bytes, bytearray)) or hasattr(challenges, "MarshalBinary"):
        ok, st = ed.batch_dleq_verify(*args, expect_c=_b(challenges))
        return np.asarray(ok) != 0, np.asarray(st)
    if len(challenges) != n:
        raise PVSSError(ErrDifferentLengths)
    ok, st = ed.batch_dleq_verify(*args)  # one challenge per element: compared here, on the raw bytes (scalar.go:37-45)
    wrong = (C != _rows(challenges)).any(axis=1)
    st = np.where(wrong, ST_DLEQ_CHALLENGE, np.asarray(st)).astype(np.uint8)
    return (np.asarray(ok) != 0) & ~wrong, st


def VerifyEncShare(H, X, sH, expGlobalChallenge, encShare: PubVerShare) -> None:
    """pvss.go:154-163: raises PVSSError(ErrGlobalChallengeVerification | ErrEncVerification)"""
    ok, st = _verify_enc(H, [X], [sH], _b(expGlobalChallenge), [encShare])
    if st[0] == ST_DLEQ_CHALLENGE:
        raise PVSSError(ErrGlobalChallengeVerification)
    if not ok[0]:
        raise PVSSError(ErrEncVerification)


def VerifyEncShareBatch(H, X, sH, commit: poly.PubPoly, encShares):
    """(K, E) of pvss.go:168-194: the public keys and encrypted shares that verify under the global challenge"""
    if len(X) != len(sH) or len(sH) != len(encShares):
        raise PVSSError(ErrDifferentLengths)
    ok, _ = _verify_enc(H, X, sH, computeGlobalChallenge(len(X), commit, encShares), encShares)
    keep = np.flatnonzero(ok)
    return [X[i] for i in keep], [encShares[i] for i in keep]


def DecShares(H, X, sH, xs, expGlobalChallenges, encShares, rand):
    """(K, E, D): DecShare (pvss.go:199-217) for every element, each with its own private key xs[i] (the loop every
    caller of DecShare runs over its trustees), as a handful of engine calls: the encrypted shares are verified, the valid
    ones decrypted as x_i^-1 * sX_i by one batch_mul, and their decryption proofs made by NewDLEQProof's batch.  The
    nonces are drawn from rand in the order of the valid shares, as the loop would."""
    ok, _ = _verify_enc(H, X, sH, expGlobalChallenges, encShares)
    keep = [int(i) for i in np.flatnonzero(ok)]
    if not keep:
        return [], [], []
    x = [xs[i] if isinstance(xs[i], ed.Scalar) else ed.Scalar(_b(xs[i])) for i in keep]
    inv = _rows([ed.Scalar().Inv(s).v for s in x])  # host, like group/mod
    V, st = ed.batch_mul(inv, _rows([encShares[i].S.V for i in keep]), uniform=True)  # decryption: x^-1 * (xS)
    if np.asarray(st).any():
        raise ValueError("invalid Ed25519 curve point")
    V = np.asarray(V)
    m = len(keep)
    proofs, _, _ = dleq.NewDLEQProofs(np.tile(np.frombuffer(_BASE, dtype=np.uint8), (m, 1)), V, _rows([s.v for s in x]), rand)
    D = [_share(encShares[i].S.I, V[k], proofs[k]) for k, i in enumerate(keep)]
    return [X[i] for i in keep], [encShares[i] for i in keep], D


def DecShare(H, X, sH, x, expGlobalChallenge, encShare: PubVerShare, rand) -> PubVerShare:
    """pvss.go:199-217: verify the encrypted share, decrypt it and prove the decryption"""
    VerifyEncShare(H, X, sH, expGlobalChallenge, encShare)
    return DecShares(H, [X], [sH], [x], _b(expGlobalChallenge), [encShare], rand)[2][0]


def DecShareBatch(H, X, sH, x, expGlobalChallenges, encShares, rand):
    """(K, E, D) of pvss.go:222-244: one trustee's key x over a batch of shares, each with its own expected global
    challenge.  The one private key is inverted once, on the host."""
    if len(X) != len(sH) or len(sH) != len(encShares):
        raise PVSSError(ErrDifferentLengths)
    one = x if isinstance(x, ed.Scalar) else ed.Scalar(_b(x))
    return DecShares(H, X, sH, [one] * len(X), expGlobalChallenges, encShares, rand)


def _verify_dec(G, X, encShares, decShares):
    n = len(X)
    if len(encShares) != n or len(decShares) != n:
        raise PVSSError(ErrDifferentLengths)
    if n == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint8)
    ok, st = ed.batch_dleq_verify(_b(G), _rows([d.S.V for d in decShares]), _rows(X), _rows([e.S.V for e in encShares]),
                                  _rows([d.P.C for d in decShares]), _rows([d.P.R for d in decShares]),
                                  _rows([d.P.VG for d in decShares]), _rows([d.P.VH for d in decShares]), fiat_shamir=True)
    return np.asarray(ok) != 0, np.asarray(st)


def VerifyDecShare(G, X, encShare: PubVerShare, decShare: PubVerShare) -> None:
    """pvss.go:248-277: raises PVSSError(ErrDecShareChallengeVerification | ErrDecVerification)"""
    ok, st = _verify_dec(G, [X], [encShare], [decShare])
    if st[0] == ST_DLEQ_CHALLENGE:
        raise PVSSError(ErrDecShareChallengeVerification)
    if not ok[0]:
        raise PVSSError(ErrDecVerification)


def VerifyDecShareBatch(G, X, encShares, decShares) -> list:
    """pvss.go:281-299: the decrypted shares that verify -- n challenges and 2n equations in one engine call"""
    ok, _ = _verify_dec(G, X, encShares, decShares)
    return [decShares[i] for i in np.flatnonzero(ok)]


def RecoverSecret(G, X, encShares, decShares, t: int, n: int) -> ed.Point:
    """pvss.go:303-323: verify the decrypted shares, then Lagrange-interpolate the shared secret's commitment s*G"""
    D = VerifyDecShareBatch(G, X, encShares, decShares)
    if len(D) < t:
        raise PVSSError(ErrTooFewShares)
    return poly.recover_commit(_SUITE, [d.S for d in D], t, n)
