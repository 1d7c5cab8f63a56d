"""Host-side mirror of ``sign/schnorr`` verification (schnorr.go:84-160 VerifyWithChecks) for the Ed25519 group.

On this curve it is the engine call of ``sign/eddsa``: the reference hashes ``R.MarshalTo || public.MarshalTo || msg``
(schnorr.go:171-183), and MarshalTo of a point that passed IsCanonical returns the bytes it was decoded from, so the
hash is over the same bytes R || A || msg; the checks are the same set in another order (a verdict does not depend on
which failing check is met first); the equation is S*B == R + h*A; and the Ed25519 point type is no
``kyber.SubGroupElement``, so the IsInCorrectGroup branch (schnorr.go:121-123) is never taken.
tests/test_gpu_ed_verify.py holds this module against the oracle's restatement on the reference's vectors.
"""
from __future__ import annotations

import numpy as np

from . import eddsa


def batch_verify_with_checks(pubs, msgs, sigs) -> np.ndarray:
    """ok[i] = (schnorr.VerifyWithChecks(edwards25519, pubs[i], msgs[i], sigs[i]) == nil)."""
    return eddsa.batch_verify_with_checks(pubs, msgs, sigs)
