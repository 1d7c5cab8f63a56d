"""Host-side mirror of the reference's ``shuffle`` package (Neff's verifiable shuffles of ElGamal pairs) on Ed25519,
over the batch engine: pair.go, simple.go, sequences.go and, over the predicates of kyber_amd/proof/proof.py, biffle.go."""
from .biffle import Biffle, BiffleBatch, BiffleVerifier, BiffleVerifyBatch  # noqa: F401
from .pair import PairShuffle, Shuffle, Verifier  # noqa: F401
from .sequences import GetSequenceVerifiable, SequencesShuffle  # noqa: F401
from .simple import SimpleShuffle  # noqa: F401
