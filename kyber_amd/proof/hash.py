"""Host-side mirror of the reference's hash-based noninteractive Sigma-protocol contexts (proof/hash.go), function for
function, with the challenges drawn on the engine:

  newHashProver / Put / PubRand / PriRand / Proof   hash.go:12-89     -> HashProverContext
  newHashVerifier / Get / PubRand                   hash.go:91-142    -> HashVerifierContext
  HashProve, HashVerify                             hash.go:157-175   -> HashProve, HashVerify
  consumeMsg: Reseed, Write(consumed bytes)         hash.go:46-65, 111-126 over blake.go:55-74 -> root hash by hashlib
  suite.Read of n scalars from the XOF              rand.go:19-46, scalar.go:180-184 -> ONE kyb_ed25519_xof_pick for n picks

The wire layout is what suite.Write produces, read off the call sites (the encoder itself, go.dedis.ch/fixbuf, is not
part of the reference tree): a struct is the concatenation of its fields in order, a slice the concatenation of its
elements, a point its 32 MarshalBinary bytes, a scalar its 32 bytes, with no length prefixes -- which is why the
protocols pre-size every slice (pair.go:105-124, simple.go:76-83).  On read a point that does not decode is an error, a
scalar is copied raw (scalar.go:226-232), a short proof is an error, trailing bytes are ignored and never hashed.

A sequence of picks is sequential in the reference (every rejected draw moves all later ones); here more than a handful
go through ``edwards25519.batch_xof_pick``.  The 128 bytes of a Reseed and single picks stay on the Python XOF.

Points and scalar vectors cross this interface as (n, 32) uint8 arrays; a field of a message is such an array, 32
bytes, or a sequence of them.
"""
from __future__ import annotations

import os

import numpy as np

from ..group import edwards25519 as ed
from ..util import blake2xb

ErrPoint = "invalid Ed25519 curve point"  # point.go:67
ErrShort = "unexpected EOF"  # io.ReadFull on the proof's buffer
DEVICE_PICKS = 8  # more picks than this from one stream go through the engine


class ProofError(ValueError):
    """the reference's error, by its message"""


class Suite:
    """what proof.Suite asks of edwards25519.NewBlakeSHA256Ed25519WithRand(rand): the XOF factory (suite.go:31) and the
    random stream (suite.go:74-79).  rand: a util.blake2xb.XOF for reproducible proofs, None for fresh entropy."""

    def __init__(self, rand=None):
        self._rand = rand if rand is not None else blake2xb.New(os.urandom(64))

    def XOF(self, seed: bytes) -> blake2xb.XOF:
        return blake2xb.New(seed)

    def RandomStream(self):
        return self._rand


def NewBlakeSHA256Ed25519WithRand(rand=None) -> Suite:
    return Suite(rand)


def _reader(stream):
    """n -> n stream bytes, of an XOF mirror, a cipher.Stream mirror or a callable"""
    if hasattr(stream, "Read"):
        return stream.Read
    if hasattr(stream, "XORKeyStream"):
        return lambda n: stream.XORKeyStream(bytes(n))
    return stream


def picks(stream, n: int) -> np.ndarray:
    """n sequential Scalar.Pick(stream) as (n, 32) bytes.  The package's BLAKE2Xb XOF serves more than DEVICE_PICKS of
    them in one engine call and is advanced past the draws consumed; any other stream is read pick by pick."""
    n = int(n)
    if isinstance(stream, blake2xb.XOF) and n > DEVICE_PICKS:
        out, used = ed.batch_xof_pick(stream.Root(), stream.Tell(), n)
        stream.Skip(32 * used)
        return np.asarray(out)
    read = _reader(stream)
    return np.frombuffer(b"".join(blake2xb.pick(read) for _ in range(n)), dtype=np.uint8).reshape(n, 32).copy()


def _wire(field) -> bytes:
    if isinstance(field, np.ndarray):
        return np.ascontiguousarray(field, dtype=np.uint8).tobytes()
    if isinstance(field, (bytes, bytearray, memoryview)):
        return bytes(field)
    if hasattr(field, "MarshalBinary"):
        return field.MarshalBinary()
    return b"".join(_wire(e) for e in field)


class HashProverContext:
    """proof.ProverContext over a hash (hash.go:12-89)"""

    def __init__(self, suite, protocolName):
        self.suite = suite
        self.pubrand = suite.XOF(protocolName.encode() if isinstance(protocolName, str) else bytes(protocolName))
        self.prirand = suite.RandomStream()
        self._msg, self._proof = [], []

    def Put(self, *fields) -> None:
        """the fields of one message, in order"""
        self._msg += [_wire(f) for f in fields]

    def _consumeMsg(self) -> None:
        buf = b"".join(self._msg)
        if buf:
            self.pubrand.Reseed()
            self.pubrand.Write(buf)
            self._proof.append(buf)
            self._msg = []

    def PubRand(self, n: int) -> np.ndarray:
        """n challenges that depend on every bit of the proof so far"""
        self._consumeMsg()
        return picks(self.pubrand, n)

    def PriRand(self, *counts):
        """one (count, 32) array of private scalars per argument, drawn in argument order"""
        return [picks(self.prirand, c) for c in counts]

    def Proof(self) -> bytes:
        self._consumeMsg()
        return b"".join(self._proof)


class HashVerifierContext:
    """proof.VerifierContext over a hash (hash.go:91-142).  Get hands out the bytes at once and defers the decoding of
    the points it read to CheckPoints, which a verifier calls after its last Get: ONE batch_unmarshal for the whole
    transcript, the first undecodable point in transcript order deciding the error, as it does when each Get decodes on
    its own (the challenges depend on the bytes alone)."""

    def __init__(self, suite, protocolName, proof):
        self.suite = suite
        self._buf = bytes(proof)
        self._read = self._stirred = 0
        self.pubrand = suite.XOF(protocolName.encode() if isinstance(protocolName, str) else bytes(protocolName))
        self._pending = []  # point arrays read and not yet decoded, in transcript order

    def Get(self, *spec):
        """spec: (kind, count) per field, kind "P" (points) or "S" (scalars); one (count, 32) array per field"""
        out = []
        for kind, count in spec:
            have = min(count, (len(self._buf) - self._read) // 32)
            a = np.frombuffer(self._buf, dtype=np.uint8, count=32 * have, offset=self._read).reshape(have, 32).copy()
            self._read += 32 * have
            if kind == "P":
                self._pending.append(a)
            if have < count:  # a point before the end of the buffer fails first
                self.CheckPoints()
                raise ProofError(ErrShort)
            out.append(a)
        return out

    def CheckPoints(self) -> None:
        """decode every point read so far; the arrays Get returned then hold MarshalBinary's bytes of the decoded points"""
        pend, self._pending = [a for a in self._pending if a.shape[0]], []
        if not pend:
            return
        canon, st = ed.batch_unmarshal(np.concatenate(pend))
        if np.asarray(st).any():
            raise ProofError(ErrPoint)
        lo = 0
        for a in pend:
            a[:] = np.asarray(canon)[lo:lo + a.shape[0]]
            lo += a.shape[0]

    def PubRand(self, n: int) -> np.ndarray:
        if self._read > self._stirred:
            self.pubrand.Reseed()
            self.pubrand.Write(self._buf[self._stirred:self._read])
            self._stirred = self._read
        return picks(self.pubrand, n)


def HashProve(suite, protocolName, prover) -> bytes:
    """runs a Sigma-protocol prover (a callable taking the context) and returns the noninteractive proof (hash.go:157-163)"""
    ctx = HashProverContext(suite, protocolName)
    prover(ctx)
    return ctx.Proof()


def HashVerify(suite, protocolName, verifier, proof) -> None:
    """returns None if the proof checks out; raises ProofError with the reference's message otherwise (hash.go:168-175)"""
    verifier(HashVerifierContext(suite, protocolName, proof))
