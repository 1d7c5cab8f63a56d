"""Host-side mirror of ``sign/bdn`` (rogue-key-safe BLS aggregation) over the engine's MSM:

  hashPointToR            bdn.go:29-63      128-bit coefficients from BLAKE2Xs over all public keys
  NewMask publicTerms     mask.go:57-61     c_i * P_i + P_i
  AggregateSignatures     bdn.go:126-161    sum over enabled signers of (c_i + 1) * sig_i   -> ONE MSM
  AggregatePublicKeys     bdn.go:166-181    sum over enabled signers of (c_i + 1) * P_i     -> ONE MSM

Scheme on G1: signatures on G1, keys on G2 (NewSchemeOnG1, bdn.go:74-85).  Coefficients are computed over the
whole roster, aggregation only over the participants enabled in the mask.

`hash_point_to_r` and `Scheme` recompute the roster's coefficients on every call, on the host.  The package in full --
`Mask`, `NewMask`, `NewSchemeOnG1` / `NewSchemeOnG2`, the deprecated package functions and the batches -- is below: it
keeps the reference's precomputed coefficients and terms (mask.go:51-61) and gets them from the device.
"""
from __future__ import annotations

from ..util.blake2xs import blake2xs


def hash_point_to_r(publics) -> list[int]:
    """bdn.go:29-63: 16 output bytes per key, read as a little-endian integer (big-endian scalars reverse
    the chunk before SetBytes, which is the same value)."""
    out = blake2xs(b"".join(publics), 16 * len(publics))
    return [int.from_bytes(out[16 * i:16 * i + 16], "little") for i in range(len(publics))]


class Scheme:
    def __init__(self, suite_module):
        self.m = suite_module

    def _scalars(self, coefs, enabled):
        return b"".join(((coefs[i] + 1) % self.m.ORDER).to_bytes(32, "big") for i in enabled)

    def aggregate_public_keys(self, publics, mask_bits) -> bytes:
        coefs = hash_point_to_r(publics)
        enabled = [i for i, b in enumerate(mask_bits) if b]
        # c_i + 1 <= 2^128: the MSM runs 129-bit scalars (half the windows of a 256-bit one)
        out, st = self.m.g2_msm(self._scalars(coefs, enabled), b"".join(publics[i] for i in enabled), self.m.F_SCALAR_BITS(129))
        if st.any():
            raise ValueError("bdn: invalid public key")
        return bytes(out)

    def aggregate_signatures(self, sigs, publics, mask_bits) -> bytes:
        """`sigs` are the signatures of the enabled participants, in roster order (bdn.go:126-161)."""
        coefs = hash_point_to_r(publics)
        enabled = [i for i, b in enumerate(mask_bits) if b]
        if len(sigs) != len(enabled):
            raise ValueError("bdn: length of signatures and public keys must match")
        out, st = self.m.g1_msm(self._scalars(coefs, enabled), b"".join(sigs), self.m.F_SCALAR_BITS(129))
        if st.any():
            raise ValueError("bdn: invalid signature")
        return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# The package in full (bdn.go, mask.go), function for function, over the engine's two fused calls:
#
#   NewMask                 mask.go:34-64     ONE kyb_<suite>_bdn_terms_<g>: coefficients and terms of the whole roster
#   AggregatePublicKeys     bdn.go:166-181    ONE kyb_<suite>_mask_aggregate_<g> over the cached terms (additions only)
#   AggregateSignatures     bdn.go:126-161    ONE MSM of 129-bit scalars from the cached coefficients
#   VerifyBatch             (n cosigned blocks over one roster) ONE mask_aggregate, then the suite's batch_verify
#
# `suite` is a suite module (kyber_amd.pairing.bn256 / bls12381 / bn254); points are the suite's G1Elt / G2Elt mirrors
# or their MarshalBinary bytes; `random` is a callable n -> n bytes (None: os.urandom).
import os as _os

import numpy as _np

from ..pairing._engine import F_SCALAR_BITS as _F_SCALAR_BITS, F_TRUSTED as _F_TRUSTED, pack_fixed as _pack_fixed


def _enc(p) -> bytes:
    return bytes(p.enc) if hasattr(p, "enc") else bytes(p)


class Mask:
    """Mask (mask.go:12-26): the participation bitmask over a roster, with NewMask's precomputed coefficients and terms.
    Only the bitmask is mutable; Clone shares the rest."""

    def __init__(self, engine, group: int, publics, mask, coefs, terms):
        self.engine, self.group = engine, group
        self.publics, self.mask, self.publicCoefs, self.publicTerms = publics, mask, coefs, terms

    # -- mask.go:66-112
    def Mask(self) -> bytes:
        return bytes(self.mask)

    def Len(self) -> int:
        return (len(self.publics) + 7) // 8

    def SetMask(self, mask) -> None:
        """replaces the bitmask by the given buffer -- the buffer itself, as the reference aliases the slice: a bytearray,
        a writable memoryview or a one-dimensional uint8 array is kept and later writes on either side are seen by the
        other.  Only what cannot be written (bytes, a read-only view) is copied: it cannot be shared."""
        if self.Len() != len(mask):
            raise ValueError("mismatching mask lengths")
        if isinstance(mask, bytes) or getattr(mask, "readonly", False) or getattr(getattr(mask, "flags", None), "writeable", True) is False:
            mask = bytearray(mask)
        self.mask = mask

    def GetBit(self, i: int) -> bool:
        if i >= len(self.publics) or i < 0:
            raise IndexError("index out of range")
        return bool(self.mask[i >> 3] & (1 << (i & 7)))

    def SetBit(self, i: int, enable: bool) -> None:
        if i >= len(self.publics) or i < 0:
            raise IndexError("index out of range")
        if enable:
            self.mask[i >> 3] |= 1 << (i & 7)
        else:
            self.mask[i >> 3] &= ~(1 << (i & 7)) & 0xFF

    # -- mask.go:115-157: forEachBitEnabled walks every bit of every byte, stray bits of the last byte included
    def _for_each_bit_enabled(self, f) -> int:
        n = 0
        for i, b in enumerate(self.mask):
            for j in range(8):
                if b & (1 << j):
                    res = f(i, j, n)
                    if res >= 0:
                        return res
                    n += 1
        return -1

    def IndexOfNthEnabled(self, nth: int) -> int:
        return self._for_each_bit_enabled(lambda i, j, n: i * 8 + j if n == nth else -1)

    def NthEnabledAtIndex(self, idx: int) -> int:
        return self._for_each_bit_enabled(lambda i, j, n: n if i * 8 + j == idx else -1)

    # -- mask.go:159-221
    def Publics(self) -> list:
        return list(self.publics)

    def Participants(self) -> list:
        return [p for i, p in enumerate(self.publics) if self.mask[i >> 3] & (1 << (i & 7))]

    def CountEnabled(self) -> int:
        return sum(1 for i in range(len(self.publics)) if self.mask[i >> 3] & (1 << (i & 7)))

    def CountTotal(self) -> int:
        return len(self.publics)

    def Merge(self, mask) -> None:
        if len(self.mask) != len(mask):
            raise ValueError("mismatching mask length")
        for i in range(len(self.mask)):
            self.mask[i] |= mask[i]

    def Clone(self) -> "Mask":
        return Mask(self.engine, self.group, self.publics, bytearray(self.mask), self.publicCoefs, self.publicTerms)

    def _need_terms(self):
        if self.publicTerms is None:  # NewMask(.., myKey) returns before any coefficient exists (mask.go:40-49)
            raise IndexError("bdn: index out of range: this mask was made with a key and holds no coefficients or terms")


def NewMask(group, publics, myKey=None, validated: bool = False) -> Mask:
    """NewMask (mask.go:34-64).  group: the key group (suite.G1() / suite.G2()).  With myKey the mask has that key's
    bit set and, as in the reference, NO coefficients or terms; without it they are precomputed by one engine call.
    The keys go through UnmarshalBinary's checks on the device unless the caller says `validated=True` (every key came
    out of UnmarshalBinary or of the engine): a G1Elt / G2Elt can be built from bytes that were never checked, so the
    type alone vouches for nothing."""
    elt = group.Point()
    engine, g = elt.ENGINE, elt.GROUP
    publics = list(publics)
    m = Mask(engine, g, publics, bytearray((len(publics) + 7) // 8), None, None)
    if myKey is not None:
        mine = _enc(myKey)
        for i, key in enumerate(publics):
            if _enc(key) == mine:
                m.SetBit(i, True)
                return m
        raise ValueError("key not found")
    if not publics:
        m.publicCoefs, m.publicTerms = [], _np.zeros((0, elt.LEN), dtype=_np.uint8)
        return m
    roster, bad = _pack_fixed([_enc(p) for p in publics], elt.LEN)
    flags = _F_TRUSTED(0) if validated else 0
    coefs, terms, st = engine.bdn_terms(g, roster, flags)
    if bad or _np.asarray(st).any():
        raise ValueError("failed to hash public keys: invalid public key")
    m.publicCoefs = [int.from_bytes(bytes(c), "little") for c in _np.asarray(coefs)]
    m.publicTerms = _np.ascontiguousarray(terms)
    return m


class _Scheme:
    """Scheme (bdn.go:65-181): NewSchemeOnG1 keeps signatures on G1 and keys on G2, NewSchemeOnG2 the other way round."""

    def __init__(self, suite, sig_group: int, bls_scheme):
        self.suite, self.engine = suite, suite.ENGINE
        self.sig_group, self.key_group = sig_group, 3 - sig_group
        self.blsScheme = bls_scheme
        self._elt = {1: suite.G1Elt, 2: suite.G2Elt}

    def _bls(self):
        if self.blsScheme is None:
            raise NotImplementedError(f"sign/bls has no scheme with signatures on G{self.sig_group} for {self.engine.name}: "
                                      "the suite hashes to G1 only")
        return self.blsScheme

    def NewKeyPair(self, random=None):
        """bls NewKeyPair (bls.go:60-65): x = Scalar.Pick as util/random's Int draws it (rand.go:19-46: BitLen(order)
        bits big-endian, redrawn while not below the order), X = x * Base of the key group"""
        order = self.engine.ORDER
        bits = order.bit_length()
        rand = random if random is not None else _os.urandom
        while True:
            b = bytearray(rand((bits + 7) // 8))
            if bits & 7:
                b[0] &= ~(0xFF << (bits & 7)) & 0xFF
            v = int.from_bytes(b, "big")
            if v < order:
                break
        x = self.suite.Scalar(v)
        return x, self._elt[self.key_group]().Mul(x, None)

    def Sign(self, x, msg: bytes) -> bytes:
        return self._bls().sign(x.MarshalBinary() if hasattr(x, "MarshalBinary") else bytes(x), bytes(msg))

    def Verify(self, X, msg: bytes, sig: bytes, key_validated: bool = False) -> None:
        """raises ValueError("bls: invalid signature") where the reference returns that error (bls.go:82-96).  The key is
        checked like any received key unless `key_validated=True` (it came out of UnmarshalBinary or of the engine, as
        AggregatePublicKeys' result does)."""
        if not self._bls().verify(_enc(X), bytes(msg), bytes(sig), keys_validated=key_validated):
            raise ValueError("bls: invalid signature")

    def AggregateSignatures(self, sigs, mask: Mask):
        """bdn.go:126-161 as ONE MSM of the 129-bit scalars c_i + 1 over the signatures of the enabled signers.  The
        errors surface in the order of the reference's loop: a signature that does not unmarshal among those the loop
        reaches, then the length error."""
        mask._need_terms()
        elt = self._elt[self.sig_group]
        enabled = [i for i in range(len(mask.publics)) if mask.mask[i >> 3] & (1 << (i & 7))]
        sigs = list(sigs)
        t = min(len(sigs), len(enabled))
        out = elt.NULL
        if t:
            S, bad = _pack_fixed(sigs[:t], elt.LEN)
            scalars = b"".join((mask.publicCoefs[i] + 1).to_bytes(32, "big") for i in enabled[:t])
            res, st = self.engine.msm(self.sig_group, scalars, S, _F_SCALAR_BITS(129))
            st = _np.asarray(st).copy()
            st[bad] = 1
            if st.any():
                first = int(_np.flatnonzero(st)[0])
                if first in bad:
                    raise ValueError(f"{self.engine.name}: wrong size buffer")
                raise ValueError(f"{self.engine.name}: malformed point" if st[first] == 1 else f"{self.engine.name}: point not in subgroup")
            out = bytes(res)
        if len(sigs) != len(enabled):
            raise ValueError("length of signatures and public keys must match")
        return elt(out)

    def AggregatePublicKeys(self, mask: Mask):
        """bdn.go:166-181 as ONE mask_aggregate over the mask's cached terms: additions only.  The terms are the
        engine's own, so they are passed as validated."""
        return self.AggregatePublicKeysBatch(mask, [bytes(mask.mask)])[0]

    def AggregatePublicKeysBatch(self, mask: Mask, masks) -> list:
        """AggregatePublicKeys for n bitmasks over `mask`'s roster as ONE mask_aggregate: a list of key-group points"""
        mask._need_terms()
        elt = self._elt[self.key_group]
        if len(mask.publics) == 0:
            return [elt() for _ in masks]
        out, _, st = self.engine.mask_aggregate(self.key_group, mask.publicTerms, masks, _F_TRUSTED(0))
        if _np.asarray(st).any():
            raise ValueError("bdn: invalid public key term")
        return [elt(bytes(o)) for o in _np.asarray(out)]

    def VerifyBatch(self, mask: Mask, msgs, sigs, masks):
        """n aggregate signatures over ONE roster, each with its own bitmask (a chain of cosigned blocks): ONE
        mask_aggregate for the n aggregate keys, then the suite's batch_verify with keys_validated=True -- the sum of
        validated keys is a valid key by construction.  Returns a bool array; element i is what AggregatePublicKeys
        on masks[i] followed by Verify(msgs[i], sigs[i]) gives."""
        keys = self.AggregatePublicKeysBatch(mask, masks)
        if not (len(keys) == len(msgs) == len(sigs)):
            raise ValueError("one message, signature and mask per element")
        return self._bls().batch_verify([k.enc for k in keys], [bytes(x) for x in msgs], [bytes(s) for s in sigs], keys_validated=True)


def _bls_scheme(suite, sig_group: int):
    from . import bls

    name = suite.ENGINE.prefix
    table = {("bn256", 1): bls.NewSchemeOnG1_bn256, ("bn254", 1): bls.NewSchemeOnG1_bn254,
             ("bls12381", 1): bls.NewSchemeOnG1_bls12381, ("bls12381", 2): bls.NewSchemeOnG2_bls12381}
    make = table.get((name, sig_group))
    return make() if make else None


def NewSchemeOnG1(suite) -> _Scheme:
    """bdn.go:72-86: signatures on G1, public keys on G2"""
    return _Scheme(suite, 1, _bls_scheme(suite, 1))


def NewSchemeOnG2(suite) -> _Scheme:
    """bdn.go:88-102: signatures on G2, public keys on G1 (the orientation of the reference's own benchmark).  On the BN
    suites, which hash to G1 only, the masks and aggregations work and Sign / Verify raise NotImplementedError."""
    return _Scheme(suite, 2, _bls_scheme(suite, 2))


# -- v1 API, deprecated in the reference (bdn.go:183-226): NewSchemeOnG1's methods
def NewKeyPair(suite, random=None):
    return NewSchemeOnG1(suite).NewKeyPair(random)


def Sign(suite, x, msg: bytes) -> bytes:
    return NewSchemeOnG1(suite).Sign(x, msg)


def Verify(suite, X, msg: bytes, sig: bytes, key_validated: bool = False) -> None:
    return NewSchemeOnG1(suite).Verify(X, msg, sig, key_validated)


def AggregateSignatures(suite, sigs, mask: Mask):
    return NewSchemeOnG1(suite).AggregateSignatures(sigs, mask)


def AggregatePublicKeys(suite, mask: Mask):
    return NewSchemeOnG1(suite).AggregatePublicKeys(mask)
