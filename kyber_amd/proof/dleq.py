"""Host-side mirror of ``proof/dleq`` verification (dleq.go:160-172 Proof.Verify) for the Ed25519 group.

The reference checks vG == r*G + c*xG and vH == r*H + c*xH with four Point.Mul and two Point.Add per proof; here a
batch is two engine calls (edwards25519.batch_mul2: each side as one Straus-Shamir chain) and the canonical
re-encodings of VG, VH (batch_unmarshal), because Point.Equal compares re-encodings (point.go:81-96).  Making proofs
(NewDLEQProof) is not mirrored: its challenge is Scalar.Pick over an XOF, and the reference holds no vector for it.
"""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed


def batch_verify(G, H, xG, xH, C, R, VG, VH) -> np.ndarray:
    """ok[i] = (Proof{C[i], R[i], VG[i], VH[i]}.Verify(suite, G[i], H[i], xG[i], xH[i]) == nil); every argument is
    n x 32 bytes.  An element with a point that does not decode is invalid."""
    a, st_a = ed.batch_mul2(R, G, C, xG)
    b, st_b = ed.batch_mul2(R, H, C, xH)
    vg, st_g = ed.batch_unmarshal(VG)
    vh, st_h = ed.batch_unmarshal(VH)
    bad = (np.asarray(st_a) | np.asarray(st_b) | np.asarray(st_g) | np.asarray(st_h)) != 0
    same = (np.asarray(a) == np.asarray(vg)).all(axis=1) & (np.asarray(b) == np.asarray(vh)).all(axis=1)
    return same & ~bad
