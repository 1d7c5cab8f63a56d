"""Host-side mirror of ``sign/cosi`` (cosi.go) on Ed25519, function for function, with the reference's error strings in
their order, over the engine.  What the engine adds is the batch: a chain of collectively signed blocks is n signatures
over ONE roster, and ``VerifyBatch`` checks them with ONE engine call (edwards25519.batch_cosi_verify ->
kyb_ed25519_cosi_verify: the aggregate keys from tables of subset sums, SHA-512, one ladder and the comb per
signature), where the reference makes up to m Point.Add calls and two Point.Mul per signature (cosi.go:167-238,
300-317).  ``Mask.aggregate_batch`` is the aggregation alone for many masks (kyb_ed25519_mask_aggregate).

The suite's hash: SHA-512, the hash of the package's documentation and tests (cosi.go:31-33, cosi_test.go:23-25), goes
through the fused call.  Any other hashlib constructor takes ``_verify_batch_composed`` -- one batch_mask_aggregate, the
hash on the host, one batch_mul2 and the comparison -- which also is the tests' second opinion and the baseline of
tools/ed_cosi_probe.py.

Errors are ``CosiError`` with the reference's message.  ``Verify`` raises it; ``VerifyBatch`` returns one None or
CosiError per signature.  Points are edwards25519.Point objects (or their 32 canonical bytes), scalars
edwards25519.Scalar objects.  ``Commit`` and ``Response`` handle secrets and use the existing calls; nothing here is
constant-time beyond what those are."""
from __future__ import annotations

import hashlib

import numpy as np

from . import policy as _policy
from ..group import edwards25519 as ed

# Deprecated in the reference (cosi.go:391-437): the policies moved to sign/policy.go
ParticipationMask = _policy.ParticipationMask
Policy = _policy.Policy
CompletePolicy = _policy.CompletePolicy
ThresholdPolicy = _policy.ThresholdPolicy
NewThresholdPolicy = _policy.NewThresholdPolicy

_P = 2**255 - 19


class CosiError(Exception):
    pass


def _enc(p) -> bytes:
    return bytes(p) if isinstance(p, (bytes, bytearray, memoryview)) else ed._pt(p).enc


def _hash_ctor(suite, hash):
    """the suite's hash constructor: `hash` (a hashlib constructor or a name), else suite.Hash, else SHA-512"""
    h = hash if hash is not None else getattr(suite, "Hash", None)
    if h is None:
        return hashlib.sha512
    if isinstance(h, str):
        return lambda: hashlib.new(h)
    return h


def _is_sha512(ctor) -> bool:
    return getattr(ctor(), "name", "") == "sha512"


def _canon_point_bytes(b: bytes) -> bytes:
    """the bytes MarshalBinary writes for a point decoded from b: y reduced below p, the sign cleared where x = 0
    (point.go:54-63 after ge.go:110-150); exact for every b that decodes, and no point's encoding otherwise"""
    v = int.from_bytes(b, "little")
    y = (v & ((1 << 255) - 1)) % _P
    sign = 0 if y in (1, _P - 1) else v >> 255
    return (y | sign << 255).to_bytes(32, "little")


# ------------------------------------------------------------------------------------------------ the mask
class Mask:
    """cosi.go:249-377: a participation bitmask over a roster with its aggregate public key"""

    def __init__(self, suite, publics, myKey=None):
        self.suite = suite
        self.publics = list(publics)
        self.mask = bytearray(self.Len())
        self._agg = ed.Point().Null()
        if myKey is not None:  # cosi.go:266-281
            mine = _enc(myKey)
            for i, key in enumerate(self.publics):
                if _enc(key) == mine:
                    self.SetBit(i, True)
                    break
            else:
                raise CosiError("key not found")

    @property
    def AggregatePublic(self):
        if self._agg is None:  # a mask VerifyBatch made from the engine's count: aggregated when somebody asks
            out, _, st = ed.batch_mask_aggregate(b"".join(_enc(p) for p in self.publics), [bytes(self.mask)])
            if st[0]:
                raise ValueError("invalid Ed25519 curve point")
            self._agg = ed.Point(bytes(out[0]))
        return self._agg

    def Mask(self) -> bytes:  # cosi.go:286-290
        return bytes(self.mask)

    def Len(self) -> int:  # cosi.go:293-295
        return (len(self.publics) + 7) >> 3

    def SetMask(self, mask) -> None:
        """cosi.go:300-317.  The reference adds or subtracts one key per changed bit; the sum of the enabled keys is the
        same point, taken here from ONE engine call."""
        mask = bytes(mask)
        if self.Len() != len(mask):
            raise CosiError("mismatching mask lengths")
        m = len(self.publics)
        keep = bytearray(mask)
        if m & 7:  # the loop over publics never looks at the bits at or above m: they stay as they were (zero)
            keep[-1] &= (1 << (m & 7)) - 1
        self.mask = keep
        self._agg = None if m else ed.Point().Null()
        self.AggregatePublic  # noqa: B018 (aggregate now: an undecodable key is this call's error)

    def SetBit(self, i: int, enable: bool) -> None:  # cosi.go:321-336
        if i >= len(self.publics):
            raise CosiError("index out of range")
        byt, msk = i >> 3, 1 << (i & 7)
        if bool(self.mask[byt] & msk) != bool(enable):
            agg, key = self.AggregatePublic, ed.Point(_enc(self.publics[i]))
            self.mask[byt] ^= msk
            self._agg = ed.Point().Add(agg, key) if enable else ed.Point().Sub(agg, key)

    def IndexEnabled(self, i: int) -> bool:  # cosi.go:339-346
        if i >= len(self.publics):
            raise CosiError("index out of range")
        return bool(self.mask[i >> 3] & (1 << (i & 7)))

    def KeyEnabled(self, public) -> bool:  # cosi.go:350-357
        want = _enc(public)
        for i, key in enumerate(self.publics):
            if _enc(key) == want:
                return self.IndexEnabled(i)
        raise CosiError("key not found")

    def CountEnabled(self) -> int:  # cosi.go:361-372
        m = len(self.publics)
        return sum(1 for i in range(m) if self.mask[i >> 3] & (1 << (i & 7)))

    def CountTotal(self) -> int:  # cosi.go:375-377
        return len(self.publics)

    @staticmethod
    def aggregate_batch(publics, masks):
        """(aggregates (n, 32), counts (n,)): AggregatePublic and CountEnabled of many masks over one roster as ONE
        engine call (edwards25519.batch_mask_aggregate).  masks: byte strings of Len() bytes each, or an (n, stride)
        array or CUDA tensor."""
        roster = b"".join(_enc(p) for p in publics)
        if not roster:
            raise CosiError("no public keys provided")
        try:
            out, cnt, st = ed.batch_mask_aggregate(roster, masks)
        except ValueError as e:
            raise CosiError(str(e)) from None
        if len(st) and bool(st[0]):
            raise ValueError("invalid Ed25519 curve point")
        return out, cnt


def NewMask(suite, publics, myKey=None) -> Mask:  # cosi.go:260-283
    return Mask(suite, publics, myKey)


def AggregateMasks(a, b) -> bytes:  # cosi.go:380-389
    if len(a) != len(b):
        raise CosiError("mismatching mask lengths")
    return bytes(x | y for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the protocol
def Commit(suite, rand=None):
    """cosi.go:57-61: (v, V = v B).  rand: what Scalar.Pick takes; the reference draws from suite.RandomStream()."""
    if rand is None and hasattr(suite, "RandomStream"):
        rand = suite.RandomStream()
    v = suite.Scalar().Pick(rand)
    return v, suite.Point().Mul(v, None)


def AggregateCommitments(suite, commitments, masks):  # cosi.go:65-84
    if len(commitments) != len(masks):
        raise CosiError("mismatching lengths of commitment and mask slices")
    agg, agg_mask = suite.Point().Null(), bytes(len(masks[0]))
    for V, m in zip(commitments, masks):
        agg = suite.Point().Add(agg, V)
        agg_mask = AggregateMasks(agg_mask, m)
    return agg, agg_mask


def Challenge(suite, commitment, public, message, hash=None):
    """cosi.go:89-105: c = SetBytes(H(V || A || M))"""
    if commitment is None:
        raise CosiError("no commitment provided")
    if message is None:
        raise CosiError("no message provided")
    h = _hash_ctor(suite, hash)()
    h.update(_enc(commitment) + _enc(public) + bytes(message))
    return suite.Scalar().SetBytes(h.digest())


def Response(suite, private, random, challenge):  # cosi.go:109-121
    if private is None:
        raise CosiError("no private key provided")
    if random is None:
        raise CosiError("no random scalar provided")
    if challenge is None:
        raise CosiError("no challenge provided")
    ca = suite.Scalar().Mul(private, challenge)
    return ca.Add(random, ca)


def AggregateResponses(suite, responses):  # cosi.go:124-133
    if responses is None:
        raise CosiError("no responses provided")
    r = suite.Scalar().Zero()
    for x in responses:
        r = r.Add(r, x)
    return r


def Sign(suite, commitment, response, mask) -> bytes:
    """cosi.go:138-163: V || r || Z"""
    if commitment is None:
        raise CosiError("no commitment provided")
    if response is None:
        raise CosiError("no response provided")
    if mask is None:
        raise CosiError("no mask provided")
    return _enc(commitment) + response.MarshalBinary() + mask.Mask()


# ------------------------------------------------------------------------------------------------ verification
def _verify_one(suite, publics, message, sig, policy, ctor):
    """cosi.go:167-238, call by call: the path that names the reference's error.  Returns None or the message."""
    if publics is None:
        return "no public keys provided"
    if message is None:
        return "no message provided"
    if sig is None:
        return "no signature provided"
    if policy is None:
        policy = CompletePolicy()
    sig = bytes(sig)
    if len(sig) < 32:
        return "signature too short"
    V = suite.Point()
    try:
        V.UnmarshalBinary(sig[:32])
    except ValueError:
        return "unmarshalling of commitment failed"
    if len(sig) < 64:
        return "signature too short"
    r = suite.Scalar().SetBytes(sig[32:64])
    mask = NewMask(suite, publics, None)
    try:
        mask.SetMask(sig[64:])
    except CosiError as e:
        return str(e)
    A = mask.AggregatePublic
    h = ctor()
    h.update(sig[:32] + A.MarshalBinary() + bytes(message))
    k = suite.Scalar().SetBytes(h.digest())
    kA = suite.Point().Mul(k, suite.Point().Neg(A))
    sB = suite.Point().Mul(r, None)
    if not suite.Point().Add(kA, sB).Equal(V):
        return "recreated response is different from signature"
    if not policy.Check(mask):
        return "the policy is not fulfilled"
    return None


def _verify_batch_composed(roster: bytes, messages, sigs64, masks, ctor=hashlib.sha512):
    """(ok, count, status) of n cosignatures over one roster from the engine's separate calls: ONE batch_mask_aggregate,
    the challenge hashed on the host, ONE batch_mul2 for k (-A) + r B -- the point is negated, as the reference negates
    it: (l - k) A is another point when A has a torsion part -- and the comparison with V's canonical bytes."""
    n = len(sigs64)
    agg, cnt, st = ed.batch_mask_aggregate(roster, masks)
    ok = np.zeros(n, dtype=np.uint8)
    if n == 0 or st.any():
        return ok, cnt, st
    kk, rr, neg = bytearray(), bytearray(), bytearray()
    for i in range(n):
        h = ctor()
        h.update(bytes(sigs64[i][:32]) + bytes(agg[i]) + bytes(messages[i]))
        k = int.from_bytes(h.digest(), "little") % ed.ORDER
        kk += k.to_bytes(32, "little")
        neg += ed.Point().Neg(ed.Point(bytes(agg[i]))).enc
        rr += (int.from_bytes(bytes(sigs64[i][32:64]), "little") % ed.ORDER).to_bytes(32, "little")
    left, st2 = ed.batch_mul2(bytes(kk), bytes(neg), bytes(rr), ed._BASE_ENC * n)
    for i in range(n):
        ok[i] = (not st2[i]) and bytes(left[i]) == _canon_point_bytes(bytes(sigs64[i][:32]))
    return ok, cnt, st


class _Counted(Mask):
    """the mask of a signature VerifyBatch accepted: the bits are the signature's, the count is the engine's, and the
    aggregate key is computed only if the policy asks for it"""

    def __init__(self, suite, publics, mask: bytes, count: int):
        self.suite, self.publics, self.mask, self._agg, self._count = suite, list(publics), bytearray(mask), None, int(count)
        m = len(self.publics)
        if m & 7:
            self.mask[-1] &= (1 << (m & 7)) - 1

    def CountEnabled(self) -> int:
        return self._count


def VerifyBatch(suite, publics, messages, sigs, policy=None, hash=None):
    """[None or CosiError] for n cosignatures over ONE roster: what n calls of cosi.Verify(suite, publics, messages[i],
    sigs[i], policy) return (cosi.go:167-238).  The length errors are decided here; every signature of the right length
    goes through ONE engine call (SHA-512: batch_cosi_verify; another hash: _verify_batch_composed); the policy runs on
    the host over the returned counts, after the equation, as in the reference.  A signature the batch rejects is
    verified again on its own sequential path, so that its message is the reference's."""
    n = len(sigs)
    if len(messages) != n:
        raise ValueError("messages/sigs length mismatch")
    ctor = _hash_ctor(suite, hash)
    if publics is None:
        return [CosiError("no public keys provided") for _ in range(n)]
    policy_ = CompletePolicy() if policy is None else policy
    m = len(publics)
    L = (m + 7) >> 3
    errs = [None] * n
    idx = [i for i in range(n) if messages[i] is not None and sigs[i] is not None and len(sigs[i]) == 64 + L]
    fused = set()
    if idx and m:
        roster = b"".join(_enc(p) for p in publics)
        s64 = [bytes(sigs[i])[:64] for i in idx]
        masks = [bytes(sigs[i])[64:] for i in idx]
        msgs = [bytes(messages[i]) for i in idx]
        if _is_sha512(ctor):
            ok, _, cnt, st = ed.batch_cosi_verify(roster, msgs, s64, masks)
        else:
            ok, cnt, st = _verify_batch_composed(roster, msgs, s64, masks, ctor)
        if st.any():
            raise ValueError("invalid Ed25519 curve point")
        for k, i in enumerate(idx):
            if ok[k]:
                fused.add(i)
                if not policy_.Check(_Counted(suite, publics, masks[k], int(cnt[k]))):
                    errs[i] = CosiError("the policy is not fulfilled")
    for i in range(n):
        if i not in fused:  # a length error, or rejected by the batch: the sequential path names the error
            why = _verify_one(suite, publics, messages[i], sigs[i], policy, ctor)
            errs[i] = None if why is None else CosiError(why)
    return errs


def Verify(suite, publics, message, sig, policy=None, hash=None) -> None:
    """cosi.go:167-238: raises CosiError with the reference's message unless sig is a valid cosignature of message under
    publics and the policy.  VerifyBatch of one."""
    err = VerifyBatch(suite, publics, [message], [sig], policy, hash)[0]
    if err is not None:
        raise err
