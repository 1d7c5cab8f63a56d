"""Host-side mirror of the reference's ``shuffle`` package (Neff's verifiable shuffles of ElGamal pairs) on Ed25519,
over the batch engine: pair.go, simple.go and sequences.go.  biffle.go needs the general predicate prover of
proof/proof.go and is not mirrored."""
from .pair import PairShuffle, Shuffle, Verifier  # noqa: F401
from .sequences import GetSequenceVerifiable, SequencesShuffle  # noqa: F401
from .simple import SimpleShuffle  # noqa: F401
