"""Host-side mirror of ``proof/dleq`` (dleq.go) for the Ed25519 group.

  Proof.Verify        dleq.go:160-172  vG == r*G + c*xG and vH == r*H + c*xH: four Point.Mul and two Point.Add per proof
                                       -> ONE engine call for a batch (edwards25519.batch_dleq_verify: both equations in
                                          one lane program, the verdict taken on canonical bytes, no square root for vG, vH)
  NewDLEQProof        dleq.go:41-82    -> batch_mul / batch_mul_base for the four points, batch_dleq_challenge for c
  NewDLEQProofBatch   dleq.go:87-154   -> the same points; the ONE collective challenge is a host hash over 4n encodings

The commitment nonces come from a caller-supplied stream (the reference draws them from suite.RandomStream()); x and v are
secrets, so their multiplications run under KYB_F_UNIFORM.  The challenge is Scalar.Pick over the suite's XOF, BLAKE2Xb
(util/blake2xb.py on the host, csrc/blake2xb.cuh on the device), pinned by two outputs the reference prints.

``batch_verify_composed`` keeps the earlier five-call path (mul2, mul2, unmarshal, unmarshal, compare on the host): the
yardstick of the tests and of tools/ed_dleq_probe.py.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .._buf import HOST
from ..group import edwards25519 as ed
from ..util import blake2xb

ErrDifferentLengths = "inputs of different lengths"
ErrInvalidProof = "invalid proof"


class DLEQError(ValueError):
    pass


class Proof:
    """dleq.Proof (dleq.go:33-38): challenge, response and the two commitments, each 32 wire bytes"""

    __slots__ = ("C", "R", "VG", "VH")

    def __init__(self, C: bytes, R: bytes, VG: bytes, VH: bytes):
        self.C, self.R, self.VG, self.VH = bytes(C), bytes(R), bytes(VG), bytes(VH)

    def Verify(self, G: bytes, H: bytes, xG: bytes, xH: bytes) -> None:  # dleq.go:160-172
        if not batch_verify(G, H, xG, xH, self.C, self.R, self.VG, self.VH)[0]:
            raise DLEQError("invalid. " + ErrInvalidProof)

    def __eq__(self, o):
        return isinstance(o, Proof) and (self.C, self.R, self.VG, self.VH) == (o.C, o.R, o.VG, o.VH)


def _rows(x, n=None) -> np.ndarray:
    if isinstance(x, (list, tuple)):
        x = b"".join(bytes(e) for e in x)
    return HOST.rows(x, 32)


def batch_verify(G, H, xG, xH, C, R, VG, VH) -> np.ndarray:
    """ok[i] = (Proof{C[i], R[i], VG[i], VH[i]}.Verify(suite, G[i], H[i], xG[i], xH[i]) == nil); every argument is
    n x 32 bytes.  An element with a point that does not decode is invalid."""
    ok, _ = ed.batch_dleq_verify(G, H, xG, xH, C, R, VG, VH)
    return np.asarray(ok) != 0


def batch_verify_composed(G, H, xG, xH, C, R, VG, VH, vartime: bool = False) -> np.ndarray:
    """batch_verify as five calls: each side as one Straus-Shamir chain (batch_mul2), the canonical re-encodings of VG and
    VH (batch_unmarshal), and the comparison on the host."""
    a, st_a = ed.batch_mul2(R, G, C, xG, vartime)
    b, st_b = ed.batch_mul2(R, H, C, xH, vartime)
    vg, st_g = ed.batch_unmarshal(VG)
    vh, st_h = ed.batch_unmarshal(VH)
    bad = (np.asarray(st_a) | np.asarray(st_b) | np.asarray(st_g) | np.asarray(st_h)) != 0
    same = (np.asarray(a) == np.asarray(vg)).all(axis=1) & (np.asarray(b) == np.asarray(vh)).all(axis=1)
    return same & ~bad


def _mul(scalars: np.ndarray, points: np.ndarray) -> np.ndarray:
    """scalars[i] * points[i] for secret scalars: the scanned ladder (KYB_F_UNIFORM)"""
    out, st = ed.batch_mul(scalars, points, uniform=True)
    if np.asarray(st).any():
        raise ValueError("invalid Ed25519 curve point")
    return np.asarray(out)


def _commitments(G, H, x, rand):
    """(n, x, v, xG, xH, vG, vH) of dleq.go:49-57 / 106-115 for n proofs: the nonces are picked in order from rand"""
    x = _rows(x)
    n = x.shape[0]
    G, H = _rows(G), _rows(H)
    if G.shape[0] != n or H.shape[0] != n:
        raise DLEQError("invalid: " + ErrDifferentLengths)
    v = np.frombuffer(b"".join(ed.Scalar().Pick(rand).v for _ in range(n)), dtype=np.uint8).reshape(n, 32)
    return n, x, v, _mul(x, G), _mul(x, H), _mul(v, G), _mul(v, H)


def _responses(x: np.ndarray, v: np.ndarray, c) -> list:
    """r = v - c x mod l (dleq.go:77-79); c: one challenge or one per proof"""
    le = lambda b: int.from_bytes(bytes(b), "little")
    cs = [le(c)] * len(x) if isinstance(c, (bytes, bytearray)) else [le(e) for e in c]
    return [((le(v[i]) - cs[i] * le(x[i])) % ed.ORDER).to_bytes(32, "little") for i in range(len(x))]


def NewDLEQProofs(G, H, x, rand):
    """n independent NewDLEQProof calls (dleq.go:41-82) as a batch: (proofs, xG, xH), each proof with its own challenge
    c_i = H(xG_i, xH_i, vG_i, vH_i), all n derived in one engine call.  G, H, x: n x 32 bytes."""
    n, x, v, xG, xH, vG, vH = _commitments(G, H, x, rand)
    c, st = ed.batch_dleq_challenge(xG, xH, vG, vH)
    if np.asarray(st).any():
        raise DLEQError("Scalar.Pick: rejection sampling exhausted")
    r = _responses(x, v, np.asarray(c))
    return [Proof(c[i], r[i], vG[i], vH[i]) for i in range(n)], xG, xH


def NewDLEQProof(G: bytes, H: bytes, x: bytes, rand):
    """(proof, xG, xH) of dleq.go:41-82 for the secret x and the bases G, H (32 wire bytes each)"""
    proofs, xG, xH = NewDLEQProofs(G, H, x, rand)
    return proofs[0], bytes(xG[0]), bytes(xH[0])


def collective_challenge(xG, xH, vG, vH) -> bytes:
    """Pick(XOF(SHA-256(all xG || all xH || all vG || all vH))) (dleq.go:117-142): one hash, on the host"""
    h = hashlib.sha256()
    for part in (xG, xH, vG, vH):
        h.update(np.ascontiguousarray(part).tobytes())
    return blake2xb.pick(blake2xb.New(h.digest()).Read)


def NewDLEQProofBatch(G, H, secrets, rand):
    """(proofs, xG, xH) of dleq.go:87-154: n proofs under ONE challenge computed over all input values"""
    n, x, v, xG, xH, vG, vH = _commitments(G, H, secrets, rand)
    c = collective_challenge(xG, xH, vG, vH)
    r = _responses(x, v, c)
    return [Proof(c, r[i], vG[i], vH[i]) for i in range(n)], xG, xH
