"""Host-side mirror of the reference's ``encrypt/ecies`` package (ecies.go) on Ed25519, backed by the engine's fused calls:
``Encrypt`` is R = r B, dh = r pub, HKDF-SHA256 and AES-256-GCM in one kyb_ed25519_ecies_seal, ``Decrypt`` one
kyb_ed25519_ecies_open.  Nothing of the cipher runs in Python.

Conventions kept from the reference:
  * ``hash`` may be None (SHA-256, ecies.go:24-26) or SHA-256 itself (``hashlib.sha256`` or the name); any other hash has
    no kernel and raises ``ValueError``;
  * the ephemeral scalar is ``group.Scalar().Pick(rand)`` (ecies.go:29: ``random.New()``): ``rand`` as ``Scalar.Pick``
    takes it, None for the operating system's randomness;
  * ``Decrypt`` raises ``ValueError`` where the reference returns an error: "invalid ecies cipher" for a ciphertext too
    short to hold R and a tag (ecies.go:85-87; 32 to 47 bytes fail in Open), an R that is no curve point
    (ecies.go:88-90), "cipher: message authentication failed" (ecies.go:111).

``EncryptBatch`` / ``DecryptBatch`` are what the engine adds: n messages in ONE call each, failures per element.
"""
from __future__ import annotations

import hashlib

from .. import _lib
from ..group import edwards25519 as ed

_ERRORS = {
    _lib.ST_ECIES_SHORT: "invalid ecies cipher",
    _lib.ST_BAD_POINT: "invalid Ed25519 curve point",
    _lib.ST_ECIES_AUTH: "cipher: message authentication failed",
}


def _check_hash(hash) -> None:
    if hash is None or hash is hashlib.sha256 or hash == "sha256":
        return
    raise ValueError("ecies: only SHA-256 has a kernel")


def _check_group(group) -> None:
    if not isinstance(group, ed.Curve):
        raise TypeError("ecies: the engine's ECIES is on Ed25519")


def EncryptBatch(group, publics, messages, hash=None, rand=None, r=None):
    """[Encrypt(group, publics[i], messages[i], hash)] in ONE engine call.  publics: one point per message, or ONE point
    for all of them.  r: the ephemeral scalars (a list of Scalar), drawn from rand in message order when None.  Raises
    ValueError if a public key does not decode (a Point that was unmarshalled cannot)."""
    _check_group(group)
    _check_hash(hash)
    n = len(messages)
    if r is None:
        r = [group.Scalar().Pick(rand) for _ in range(n)]
    pubs = [publics] if isinstance(publics, ed.Point) else list(publics)
    if len(r) != n or len(pubs) not in (1, n):
        raise ValueError("ecies: one scalar per message; one public key or one per message")
    if n == 0:
        return []
    ctx, st = ed.batch_ecies_seal(b"".join(ed._sc(s).v for s in r), b"".join(ed._pt(p).MarshalBinary() for p in pubs),
                                  [bytes(m) for m in messages])
    if st.any():
        raise ValueError("invalid Ed25519 curve point")
    return ctx


def Encrypt(group, public, message: bytes, hash=None, rand=None) -> bytes:
    """ecies.go:23-69: R || AES-256-GCM(message) under the key and nonce derived from r * public."""
    return EncryptBatch(group, [public], [message], hash, rand)[0]


def DecryptBatch(group, private, ctxs, hash=None):
    """(messages, status): Decrypt(group, private, ctxs[i], hash) for every i in ONE engine call.  private: one Scalar for
    all ciphertexts (the DKG's case) or one per ciphertext.  messages[i] is None where status[i] != 0
    (_lib.ST_ECIES_SHORT, ST_BAD_POINT, ST_ECIES_AUTH)."""
    _check_group(group)
    _check_hash(hash)
    privs = [private] if isinstance(private, ed.Scalar) else list(private)
    n = len(ctxs)
    if len(privs) not in (1, n):
        raise ValueError("ecies: one private key or one per ciphertext")
    if n == 0:
        return [], ed.HOST.status(0)[:0]
    msgs, st = ed.batch_ecies_open(b"".join(ed._sc(s).v for s in privs), [bytes(c) for c in ctxs])
    return [m if not st[i] else None for i, m in enumerate(msgs)], st


def Decrypt(group, private, ctx: bytes, hash=None) -> bytes:
    """ecies.go:77-112."""
    msgs, st = DecryptBatch(group, private, [ctx], hash)
    if st[0]:
        raise ValueError(_ERRORS.get(int(st[0]), "ecies: decryption failed"))
    return msgs[0]
