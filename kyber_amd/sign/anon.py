"""Host-side mirror of ``sign/anon`` for the Ed25519 group.  The Go package has two halves: sig.go -- Rivest-style ring
signatures and, with a link scope, Liu-Wei-Wong linkable ring signatures -- and enc.go -- encryption for an explicit
anonymity set.

  Encrypt  enc.go:123-148   per ring member a Mul, a MarshalBinary and a BLAKE2Xb stream, then the message stream and MAC
                            -> ONE engine call for a batch (edwards25519.batch_anon_seal: ring products of one scalar over
                               shared window tables, every encoding from the shared inversion, the hashes on the device)
  Decrypt  enc.go:165-192   a Mul to recover the master secret, Mul(x, nil) against X, the whole header regenerated so
                            that every member could have decrypted, the MAC
                            -> ONE engine call for a batch (edwards25519.batch_anon_open)

  Verify   sig.go:192-248   per ring position a Mul(s, nil), up to three Mul, two Add and a hash that needs the encodings
                            -> ONE engine call for a batch (edwards25519.batch_ring_chain: the whole hash chain of a
                               signature in one lane, both points of a step from one inversion, BLAKE2Xb and Pick on the device)
  Sign     sig.go:107-180   -> tag, u G and u linkBase through the existing multiplications under KYB_F_UNIFORM (x and u are
                               secrets), c[mine + 1] from batch_ring_challenge, the other ring - 1 positions as one
                               batch_ring_chain from mine + 1, and s_mine = u - x c_mine on the host

Signature bytes are the reference's: c_0 || s_0 .. s_{ring-1} || [tag], 32 bytes each (suite.Write of uSig / lSig).  The
random scalars come from a caller-supplied stream (the reference draws them from suite.RandomStream()) in the
reference's order: per signature u, then s_i for i = mine + 1 .. mine - 1.  Scalars read from a signature are its wire
bytes, unreduced, as UnmarshalBinary leaves them.
"""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed
from ..util import blake2xb

ErrInvalidSignature = "invalid signature"
# Decrypt's errors (enc.go:56, 71, 87, 98, 176, 189) and UnmarshalBinary's for an X that is no point, by engine status
_DECRYPT_ERRORS = {ed._lib.ST_ANON_SHORT: "ciphertext too short", ed._lib.ST_BAD_POINT: "invalid Ed25519 curve point",
                   ed._lib.ST_ANON_INVALID: "invalid ciphertext", ed._lib.ST_ANON_MAC: "invalid ciphertext: failed MAC check"}
_P = 2**255 - 19


class AnonError(ValueError):
    pass


def _enc(p) -> bytes:
    return p.MarshalBinary() if isinstance(p, (ed.Point, ed.Scalar)) else bytes(p)


def _sets(anonymitySet, n: int):
    """(keys as rows of ring x 32 bytes, ring): one set, or one set per signature, all of the same length"""
    if len(anonymitySet) and isinstance(anonymitySet[0], (list, tuple)):
        if len(anonymitySet) != n or any(len(s) != len(anonymitySet[0]) for s in anonymitySet):
            raise ValueError("one anonymity set, or one per signature, all of the same length")
        ring = len(anonymitySet[0])
        rows = [b"".join(_enc(k) for k in s) for s in anonymitySet]
    else:
        ring = len(anonymitySet)
        rows = [b"".join(_enc(k) for k in anonymitySet)]
    if ring == 0 or any(len(r) != 32 * ring for r in rows):
        raise ValueError("an anonymity set is one or more 32-byte public keys")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 32 * ring), ring


def link_base(linkScope: bytes) -> bytes:
    """suite.Point().Pick(suite.XOF(linkScope)) (sig.go:131-132, 207-208)"""
    return ed.Point().Embed(None, blake2xb.New(bytes(linkScope))).MarshalBinary()


def _canon_tag(t: bytes) -> bytes:
    """MarshalBinary of the point t decodes to: y below p, the sign cleared where x = 0"""
    v = int.from_bytes(t, "little")
    sign, y = v >> 255, (v & ((1 << 255) - 1)) % _P
    if y in (1, _P - 1):
        sign = 0
    return (y | (sign << 255)).to_bytes(32, "little")


def VerifyBatch(messages, anonymitySet, linkScope, sigs, vartime: bool = False):
    """(tags, ok, status): Verify for n signatures as one engine call.  tags[i] is what Verify returns -- b"" for an
    unlinkable signature, the re-encoded tag for a linkable one -- or None where the signature is invalid.  Every
    signature must have its full length, 32 (ring + 1) bytes or 32 (ring + 2) with a tag."""
    n = len(messages)
    keys, ring = _sets(anonymitySet, n)
    slots = ring + (2 if linkScope is not None else 1)
    if len(sigs) != n or any(len(s) < 32 * slots for s in sigs):
        raise AnonError("short signature buffer")
    if n == 0:
        return [], np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)
    rows = np.frombuffer(b"".join(bytes(s)[:32 * slots] for s in sigs), dtype=np.uint8).reshape(n, 32 * slots)
    base = link_base(linkScope) if linkScope is not None else None
    _, _, ok, st = ed.batch_ring_chain(keys, messages, linkScope, base, rows, ring, vartime=vartime)
    tags = [(b"" if linkScope is None else _canon_tag(bytes(rows[i, 32 * (ring + 1):]))) if ok[i] else None for i in range(n)]
    return tags, ok, st


def Verify(message: bytes, anonymitySet, linkScope, signatureBuffer: bytes) -> bytes:
    """sig.go:192-248: the linkage tag (b"" for an unlinkable signature); AnonError for an invalid signature, a short
    buffer or a tag that does not decode."""
    tags, ok, st = VerifyBatch([message], anonymitySet, linkScope, [signatureBuffer])
    if st[0] == ed._lib.ST_BAD_POINT:
        raise AnonError("invalid Ed25519 curve point")
    if not ok[0]:
        raise AnonError(ErrInvalidSignature)
    return tags[0]


def SignBatch(messages, anonymitySet, linkScope, mine, privateKeys, rand):
    """n signatures (sig.go:107-180), signature i by member mine[i] of its set with private key privateKeys[i].  mine: one
    position or one per signature.  rand: a stream with Read(n) (util/blake2xb.XOF); drawn from in the reference's order."""
    n = len(messages)
    keys, ring = _sets(anonymitySet, n)
    mine = [int(mine)] * n if isinstance(mine, (int, np.integer)) else [int(m) for m in mine]
    if len(mine) != n or len(privateKeys) != n or any(not 0 <= m < ring for m in mine):
        raise ValueError("one position inside the ring and one private key per signature")
    if n == 0:
        return []
    linkable = linkScope is not None
    xs = [int.from_bytes(_enc(x), "little") % ed.ORDER for x in privateKeys]
    u = []
    s = np.zeros((n, ring, 32), dtype=np.uint8)
    for i in range(n):
        u.append(blake2xb.pick_int(rand.Read)[0])
        for k in range(1, ring):
            s[i, (mine[i] + k) % ring] = np.frombuffer(blake2xb.pick(rand.Read), dtype=np.uint8)
    ub = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in u), dtype=np.uint8).reshape(n, 32)
    UB = ed.batch_mul_base(ub, uniform=True)
    base = tags = UL = None
    if linkable:
        base = link_base(linkScope)
        xb = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint8).reshape(n, 32)
        tags = ed.commit(xb, base, uniform=True)
        UL = ed.commit(ub, base, uniform=True)
    c_next, st = ed.batch_ring_challenge(messages, linkScope, tags, UB, UL)
    if st.any():
        raise AnonError("Scalar.Pick found no scalar")
    slots = ring + (2 if linkable else 1)
    rows = np.zeros((n, slots, 32), dtype=np.uint8)
    rows[:, 0] = c_next
    rows[:, 1:1 + ring] = s
    if linkable:
        rows[:, 1 + ring] = tags
    if ring > 1:
        start = np.array([(m + 1) % ring for m in mine], dtype=np.uint32)
        c_zero, c_mine, _, st = ed.batch_ring_chain(keys, messages, linkScope, base, rows.reshape(n, 32 * slots), ring,
                                                    start=start, steps=ring - 1)
        if st.any():
            raise AnonError("invalid Ed25519 curve point in the anonymity set" if (st == ed._lib.ST_BAD_POINT).any()
                            else "Scalar.Pick found no scalar")
    else:
        c_zero = c_mine = c_next
    out = []
    for i in range(n):
        cm = int.from_bytes(bytes(c_mine[i]), "little")
        rows[i, 1 + mine[i]] = np.frombuffer(((u[i] - xs[i] * cm) % ed.ORDER).to_bytes(32, "little"), dtype=np.uint8)
        rows[i, 0] = c_zero[i]
        out.append(rows[i].tobytes())
    return out


def Sign(message: bytes, anonymitySet, linkScope, mine: int, privateKey, rand) -> bytes:
    """sig.go:107-180 for one signature"""
    return SignBatch([message], anonymitySet, linkScope, mine, [privateKey], rand)[0]


def _raw(x) -> bytes:
    """a scalar's 32 bytes as Point.Mul reads them: unreduced"""
    return x.v if isinstance(x, ed.Scalar) else bytes(x)


def EncryptBatch(messages, anonymitySet, rand):
    """n ciphertexts (enc.go:123-148), message i for its anonymity set -- one set, or one per message.  The n ephemeral
    keys are drawn from rand as n sequential Encrypts draw them (key.Pair.Gen: the suite's NewKey, 32 stream bytes each);
    everything else is ONE seal."""
    n = len(messages)
    keys, ring = _sets(anonymitySet, n)
    if n == 0:
        return []
    suite = ed.NewSuite()
    x = np.frombuffer(b"".join(suite.NewKey(rand).v for _ in range(n)), dtype=np.uint8).reshape(n, 32)
    out, st = ed.batch_anon_seal(keys, x, [bytes(m) for m in messages], ring)
    if st.any():
        raise AnonError("invalid Ed25519 curve point in the anonymity set")
    return out


def Encrypt(suite, message: bytes, anonymitySet, rand) -> bytes:
    """enc.go:123-148 for one message; rand stands for suite.RandomStream()"""
    return EncryptBatch([message], anonymitySet, rand)[0]


def DecryptBatch(ciphertexts, anonymitySet, mine, privateKeys):
    """Decrypt (enc.go:165-192) for n ciphertexts as ONE open: element i is the plaintext, or the AnonError Decrypt would
    return.  anonymitySet: one set or one per ciphertext; mine: one position or one per ciphertext; privateKeys: one key or
    one per ciphertext.  A position outside the set raises (the reference panics)."""
    n = len(ciphertexts)
    keys, ring = _sets(anonymitySet, n)
    mine = [int(mine)] * n if isinstance(mine, (int, np.integer)) else [int(m) for m in mine]
    if len(mine) != n or any(not 0 <= m < ring for m in mine):
        raise ValueError("private-key index out of range")
    if isinstance(privateKeys, (list, tuple)):
        if len(privateKeys) != n:
            raise ValueError("one private key, or one per ciphertext")
        privs = b"".join(_raw(x) for x in privateKeys)
    else:
        privs = _raw(privateKeys) * n
    if n == 0:
        return []
    msgs, st = ed.batch_anon_open(keys, np.array(mine, dtype=np.uint32), np.frombuffer(privs, dtype=np.uint8).reshape(n, 32),
                                  [bytes(c) for c in ciphertexts], ring)
    return [msgs[i] if not st[i] else AnonError(_DECRYPT_ERRORS[int(st[i])]) for i in range(n)]


def Decrypt(suite, ciphertext: bytes, anonymitySet, mine: int, privateKey) -> bytes:
    """enc.go:165-192 for one ciphertext: the message, or AnonError with the reference's text"""
    out = DecryptBatch([ciphertext], anonymitySet, mine, privateKey)[0]
    if isinstance(out, AnonError):
        raise out
    return out
