"""Host-side mirror of ``sign/policy.go``: the cosigning policies a verifier holds a participation mask against.

A ``ParticipationMask`` (policy.go:3-10) is anything with ``CountEnabled()`` and ``CountTotal()``; a ``Policy``
(policy.go:12-21) anything with ``Check(mask) -> bool``.  ``sign/cosi`` keeps its deprecated names as aliases of these."""
from __future__ import annotations


class ParticipationMask:
    """policy.go:3-10: the number of participants and of candidates (a protocol: any object with the two methods)"""

    def CountEnabled(self) -> int:  # pragma: no cover
        raise NotImplementedError

    def CountTotal(self) -> int:  # pragma: no cover
        raise NotImplementedError


class Policy:
    """policy.go:12-21 (a protocol: any object with Check)"""

    def Check(self, m) -> bool:  # pragma: no cover
        raise NotImplementedError


class CompletePolicy(Policy):
    """policy.go:23-32: every participant has cosigned"""

    def Check(self, m) -> bool:
        return m.CountEnabled() == m.CountTotal()


class ThresholdPolicy(Policy):
    """policy.go:34-50: at least ``thold`` participants have cosigned"""

    def __init__(self, thold: int):
        self.thold = int(thold)

    def Check(self, m) -> bool:
        return m.CountEnabled() >= self.thold


def NewThresholdPolicy(thold: int) -> ThresholdPolicy:
    return ThresholdPolicy(thold)
