"""CPU ORACLE (test infrastructure, not product code) -- sign/cosi and sign/policy.go, sequentially, in Python integers
over oracle/ed25519.py.  Every function cites the reference code whose behaviour it restates; errors are the
reference's strings.  Points travel as their 32 bytes and are decoded where the reference would hold a kyber.Point;
scalars as integers.

The reference prints no CoSi bytes and there is no Go toolchain next to these tests, so what pins this oracle is the
reference's own EdDSA vectors (cosi_test.go:152-156: a cosignature without its mask is an EdDSA signature under the
aggregate key) and its test scenarios, tests/test_cosi_oracle.py."""
from __future__ import annotations

import functools
import hashlib

from oracle import ed25519 as O

IDENTITY_ENC = O.encode(O.IDENTITY)
ST_OK, ST_BAD_POINT = 0, 1  # include/kyber_hip.h


class CosiError(Exception):
    pass


# ------------------------------------------------------------------------------------------------ sign/policy.go
class CompletePolicy:  # policy.go:23-32
    def Check(self, m) -> bool:
        return m.CountEnabled() == m.CountTotal()


class ThresholdPolicy:  # policy.go:34-50
    def __init__(self, thold: int):
        self.thold = thold

    def Check(self, m) -> bool:
        return m.CountEnabled() >= self.thold


def NewThresholdPolicy(thold: int) -> ThresholdPolicy:
    return ThresholdPolicy(thold)


# ------------------------------------------------------------------------------------------------ points and scalars
@functools.lru_cache(maxsize=None)
def decode(b: bytes):
    """O.decode, remembered: a roster is decoded once, as the reference holds it decoded"""
    return O.decode(b)


def canon(b: bytes):
    """MarshalBinary(UnmarshalBinary(b)), None when b is no point (point.go:54-70)"""
    p = decode(bytes(b))
    return None if p is None else O.encode(p)


@functools.lru_cache(maxsize=None)
def _base_rows():
    """j 16^i B for i < 64, j < 16, extended coordinates: r B in 64 additions"""
    rows, p = [], O._ext(O.B)
    for _ in range(64):
        row = [(0, 1, 1, 0)]
        for _ in range(15):
            row.append(O._ext_add(row[-1], p))
        rows.append(row)
        p = O._ext_add(row[-1], p)
    return rows


def mul_base_int(r: int):
    """r B for 0 <= r < 2^256, the same point as O.mul_int(r, O.B)"""
    acc = (0, 1, 1, 0)
    for i, row in enumerate(_base_rows()):
        d = (r >> (4 * i)) & 15
        if d:
            acc = O._ext_add(acc, row[d])
    return O._aff(acc)


def padd(a, b):
    return O._aff(O._ext_add(O._ext(a), O._ext(b)))


def mask_len(m: int) -> int:  # cosi.go:293-295
    return (m + 7) >> 3


def enabled(mask: bytes, m: int):
    """the indices SetMask's loop over publics enables (cosi.go:300-317): bits at or above m are never looked at"""
    return [j for j in range(m) if mask[j >> 3] & (1 << (j & 7))]


def aggregate(publics, mask: bytes):
    """(AggregatePublic's bytes, CountEnabled) after SetMask(mask) on a fresh mask; (None, count) when a roster key is no
    point -- the engine's rule, the reference holds decoded points"""
    m = len(publics)
    on = enabled(mask, m)
    pts = [decode(bytes(p)) for p in publics]
    if any(p is None for p in pts):
        return None, len(on)
    acc = (0, 1, 1, 0)
    for j in on:
        acc = O._ext_add(acc, O._ext(pts[j]))
    return O.encode(O._aff(acc)), len(on)


def challenge_int(Vb: bytes, Ab: bytes, message: bytes, hash=hashlib.sha512) -> int:
    """cosi.go:86-105 / 214-220: SetBytes of H(V || A || M)"""
    return int.from_bytes(hash(Vb + Ab + message).digest(), "little") % O.L


# ------------------------------------------------------------------------------------------------ the engine's contract
def abi_mask_aggregate(publics, mask: bytes):
    """(out, count, status) of one element of kyb_ed25519_mask_aggregate"""
    a, cnt = aggregate(publics, mask)
    return (a or bytes(32)), cnt, (ST_OK if a else ST_BAD_POINT)


def abi_cosi_verify(publics, message: bytes, sig64: bytes, mask: bytes, hash=hashlib.sha512):
    """(ok, agg, count, status) of one element of kyb_ed25519_cosi_verify"""
    a, cnt = aggregate(publics, mask)
    if a is None:
        return 0, bytes(32), cnt, ST_BAD_POINT
    Vb, r = sig64[:32], int.from_bytes(sig64[32:64], "little") % O.L
    k = challenge_int(Vb, a, message, hash)
    left = padd(O.mul_int(k, O.neg(decode(a))), mul_base_int(r))
    return int(canon(Vb) == O.encode(left)), a, cnt, ST_OK


# ------------------------------------------------------------------------------------------------ cosi.go
class Mask:  # cosi.go:249-377
    def __init__(self, publics, myKey=None):  # NewMask, cosi.go:260-283
        self.publics = [bytes(p) for p in publics]
        self.mask = bytearray(mask_len(len(publics)))
        self.agg = O.IDENTITY
        if myKey is not None:
            for i, key in enumerate(self.publics):
                if canon(key) == canon(bytes(myKey)):
                    self.SetBit(i, True)
                    break
            else:
                raise CosiError("key not found")

    @property
    def AggregatePublic(self) -> bytes:
        return O.encode(self.agg)

    def Mask(self) -> bytes:
        return bytes(self.mask)

    def Len(self) -> int:
        return mask_len(len(self.publics))

    def _flip(self, i: int, on: bool):
        self.mask[i >> 3] ^= 1 << (i & 7)
        p = decode(self.publics[i])
        self.agg = padd(self.agg, p if on else O.neg(p))

    def SetMask(self, mask: bytes):  # cosi.go:300-317
        if self.Len() != len(mask):
            raise CosiError("mismatching mask lengths")
        for i in range(len(self.publics)):
            have, want = bool(self.mask[i >> 3] & (1 << (i & 7))), bool(mask[i >> 3] & (1 << (i & 7)))
            if have != want:
                self._flip(i, want)

    def SetBit(self, i: int, enable: bool):  # cosi.go:321-336
        if i >= len(self.publics):
            raise CosiError("index out of range")
        if bool(self.mask[i >> 3] & (1 << (i & 7))) != bool(enable):
            self._flip(i, bool(enable))

    def IndexEnabled(self, i: int) -> bool:  # cosi.go:339-346
        if i >= len(self.publics):
            raise CosiError("index out of range")
        return bool(self.mask[i >> 3] & (1 << (i & 7)))

    def KeyEnabled(self, public: bytes) -> bool:  # cosi.go:350-357
        for i, key in enumerate(self.publics):
            if canon(key) == canon(bytes(public)):
                return self.IndexEnabled(i)
        raise CosiError("key not found")

    def CountEnabled(self) -> int:  # cosi.go:361-372
        return len(enabled(self.mask, len(self.publics)))

    def CountTotal(self) -> int:
        return len(self.publics)


def AggregateMasks(a: bytes, b: bytes) -> bytes:  # cosi.go:380-389
    if len(a) != len(b):
        raise CosiError("mismatching mask lengths")
    return bytes(x | y for x, y in zip(a, b))


def Commit(v: int):  # cosi.go:57-61 with the random scalar given
    return v % O.L, O.encode(mul_base_int(v % O.L))


def AggregateCommitments(commitments, masks):  # cosi.go:65-84
    if len(commitments) != len(masks):
        raise CosiError("mismatching lengths of commitment and mask slices")
    acc, agg_mask = O.IDENTITY, bytes(len(masks[0]))
    for V, m in zip(commitments, masks):
        acc = padd(acc, decode(bytes(V)))
        agg_mask = AggregateMasks(agg_mask, m)
    return O.encode(acc), agg_mask


def Challenge(commitment, public, message, hash=hashlib.sha512) -> int:  # cosi.go:89-105
    if commitment is None:
        raise CosiError("no commitment provided")
    if message is None:
        raise CosiError("no message provided")
    return challenge_int(canon(commitment), canon(public), message, hash)


def Response(private, random, challenge) -> int:  # cosi.go:109-121
    if private is None:
        raise CosiError("no private key provided")
    if random is None:
        raise CosiError("no random scalar provided")
    if challenge is None:
        raise CosiError("no challenge provided")
    return (random + private * challenge) % O.L


def AggregateResponses(responses) -> int:  # cosi.go:124-133
    if responses is None:
        raise CosiError("no responses provided")
    return sum(responses) % O.L


def Sign(commitment, response, mask) -> bytes:  # cosi.go:138-163
    if commitment is None:
        raise CosiError("no commitment provided")
    if response is None:
        raise CosiError("no response provided")
    if mask is None:
        raise CosiError("no mask provided")
    return canon(commitment) + (response % O.L).to_bytes(32, "little") + mask.Mask()


def Verify(publics, message, sig, policy=None, hash=hashlib.sha512):
    """cosi.go:167-238: None, or the reference's error string"""
    if publics is None:
        return "no public keys provided"
    if message is None:
        return "no message provided"
    if sig is None:
        return "no signature provided"
    if policy is None:
        policy = CompletePolicy()
    if len(sig) < 32:
        return "signature too short"
    if decode(bytes(sig[:32])) is None:
        return "unmarshalling of commitment failed"
    if len(sig) < 64:
        return "signature too short"
    mask = Mask(publics)
    try:
        mask.SetMask(sig[64:])
    except CosiError as e:
        return str(e)
    ok, _, _, _ = abi_cosi_verify(publics, message, sig[:64], sig[64:], hash)
    if not ok:
        return "recreated response is different from signature"
    if not policy.Check(mask):
        return "the policy is not fulfilled"
    return None


def cosign(privates, publics, signers, message: bytes, randoms, hash=hashlib.sha512) -> bytes:
    """testCoSi's protocol run (cosi_test.go:69-137) for the cosigners `signers` (indices into the roster), with the
    random scalars given: V || r || Z"""
    masks = [Mask(publics, publics[i]) for i in signers]
    coms = [Commit(v) for v in randoms]
    aggV, agg_mask = AggregateCommitments([c[1] for c in coms], [m.Mask() for m in masks])
    for m in masks:
        m.SetMask(agg_mask)
    cs = [Challenge(aggV, m.AggregatePublic, message, hash) for m in masks]
    rs = [Response(privates[i], c[0], ch) for i, c, ch in zip(signers, coms, cs)]
    return Sign(aggV, AggregateResponses(rs), masks[0])
