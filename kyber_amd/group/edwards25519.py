"""Host-side mirror of the reference's ``group/edwards25519`` suite for the hot
path (kyber.Group / kyber.Point / kyber.Scalar, group.go:23-183), backed by
the HIP engine through the C ABI.  No group arithmetic happens in Python.

Conventions kept from the reference:
  * receiver-mutating methods that return the receiver (``P.Mul(s, A)`` sets P);
  * ``A is None`` means the base point (group.go:128-130);
  * a wrong concrete type raises ``TypeError`` (the reference panics with
    ErrTypeCast, point.go:237-249);
  * ``UnmarshalBinary`` raises ``ValueError`` for an invalid encoding
    (the reference returns an error, point.go:65-70);
  * scalars are 32-byte little-endian; ``UnmarshalBinary`` copies them
    unreduced (scalar.go:226-233), ``SetBytes`` reduces mod l (scalar.go:187).

The batch API (``batch_mul``, ``batch_mul_base``, ``commit``) is what the
engine adds: the reference has no batch entry points.
Batch functions accept either host data (bytes / numpy uint8 arrays) or
device-resident ``torch.uint8`` CUDA tensors; device inputs are processed in
place on the current stream and the result is a CUDA tensor.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

from .. import _lib  # noqa: F401 (sign/anon reads the status codes through this module)
from .._buf import HOST, _is_torch, dst_arg, pack_msgs, space_of
from .._lib import KYB_F_DLEQ_FS, KYB_F_UNIFORM, KYB_F_VARTIME

# group/edwards25519/const.go:15
ORDER = 2**252 + 27742317777372353535851937790883648493
_P = 2**255 - 19
POINT_LEN = 32
SCALAR_LEN = 32
_BASE_ENC = bytes([0x58]) + bytes([0x66]) * 31
_NULL_ENC = bytes([1]) + bytes(31)


# ------------------------------------------------------------------ batch API
def _flags(vartime: bool, uniform: bool) -> int:
    if vartime and uniform:
        raise ValueError("vartime and uniform are exclusive")
    return KYB_F_VARTIME if vartime else (KYB_F_UNIFORM if uniform else 0)


def _rows32(sp, xs):
    """every argument as n x 32 bytes, all of one n"""
    t = [sp.rows(x, 32) for x in xs]
    for x in t:
        if x.shape != t[0].shape:
            raise ValueError("length mismatch")
    return t


def _joined(x):
    return b"".join(x) if isinstance(x, (list, tuple)) else x


def batch_mul_base(scalars, vartime: bool = False, uniform: bool = False):
    """out[i] = scalars[i] * B   (replaces N x Point.Mul(s, nil), ge.go:373).  uniform: KYB_F_UNIFORM -- the table is
    scanned, not indexed (the access pattern of the reference's constant-time path), for secret scalars."""
    flags = _flags(vartime, uniform)
    sp = space_of(scalars)
    s = sp.rows(scalars, 32)
    out = sp.out(s.shape)
    sp.call("kyb_ed25519_mul_base", s.shape[0], sp.ptr(s), sp.ptr(out), flags)
    return out


def batch_mul(scalars, points, vartime: bool = False, uniform: bool = False):
    """(out, status): out[i] = scalars[i] * points[i]; status[i] != 0 where
    points[i] is not a valid encoding (then out[i] is zero bytes).
    Replaces N x (UnmarshalBinary + Point.Mul(s, A) + MarshalBinary)."""
    flags = _flags(vartime, uniform)
    sp = space_of(scalars)
    s, p = sp.rows(scalars, 32), sp.rows(points, 32)
    if s.shape != p.shape:
        raise ValueError("scalars/points length mismatch")
    n = s.shape[0]
    out, st = sp.out(s.shape), sp.status(n)
    sp.call("kyb_ed25519_mul", n, sp.ptr(s), sp.ptr(p), sp.ptr(out), sp.ptr(st), flags)
    return out, st[:n]


def batch_mul2(a, P, b, Q, vartime: bool = False):
    """(out, status): out[i] = a[i] * P[i] + b[i] * Q[i] as one Straus-Shamir chain (kyb_ed25519_mul2): byte-identical to
    batch_add(batch_mul(a, P), batch_mul(b, Q)) under the same flag.  status[i] != 0 and out[i] zero where either point
    does not decode.  The shape of proof/dleq Proof.Verify (dleq.go:160-172)."""
    sp = space_of(a)
    t = _rows32(sp, (a, P, b, Q))
    n = t[0].shape[0]
    out, st = sp.out(t[0].shape), sp.status(n)
    sp.call("kyb_ed25519_mul2", n, *map(sp.ptr, t), sp.ptr(out), sp.ptr(st), KYB_F_VARTIME if vartime else 0)
    return out, st[:n]


def batch_dleq_challenge(xG, xH, vG, vH):
    """(c, status): c[i] = Scalar.Pick(suite.XOF(SHA-256(xG[i] || xH[i] || vG[i] || vH[i]))), the Fiat-Shamir challenge
    of NewDLEQProof (dleq.go:57-79) and VerifyDecShare (pvss.go:250-266), one lane per element (kyb_ed25519_dleq_challenge:
    SHA-256, BLAKE2Xb and Pick's rejection loop on the device).  Every argument is n x 32 bytes."""
    sp = space_of(xG)
    t = _rows32(sp, (xG, xH, vG, vH))
    n = t[0].shape[0]
    c, st = sp.out(t[0].shape), sp.status(n)
    sp.call("kyb_ed25519_dleq_challenge", n, *map(sp.ptr, t), sp.ptr(c), sp.ptr(st))
    return c, st[:n]


def _one_or_n(x, n: int, what: str) -> int:
    """the stride of a base argument: 0 for one element shared by the batch, 32 for one per element"""
    if x.shape[0] == n and n != 1:
        return 32
    if x.shape[0] == 1:
        return 0 if n != 1 else 32
    raise ValueError(f"{what}: one base or one per element")


def batch_dleq_verify(G, H, xG, xH, C, R, VG, VH, expect_c=None, fiat_shamir: bool = False, vartime: bool = False):
    """(ok, status): ok[i] = (Proof{C[i], R[i], VG[i], VH[i]}.Verify(suite, G[i], H[i], xG[i], xH[i]) == nil)
    (dleq.go:160-172) as ONE engine call (kyb_ed25519_dleq_verify).  G and H are n x 32 bytes or ONE 32-byte base shared by
    the batch.  expect_c: one 32-byte scalar every C[i] must equal (pvss.go:154-157); fiat_shamir: every C[i] must equal
    the challenge derived on the device from (xG, xH, VG, VH)[i] (pvss.go:250-270).  status: include/kyber_hip.h."""
    flags = (KYB_F_VARTIME if vartime else 0) | (KYB_F_DLEQ_FS if fiat_shamir else 0)
    sp = space_of(xG)
    t = _rows32(sp, (xG, xH, C, R, VG, VH))
    n = t[0].shape[0]
    g, h = sp.rows(G, 32), sp.rows(H, 32)
    e = sp.rows(expect_c, 32) if expect_c is not None else None
    if e is not None and e.shape[0] != 1:
        raise ValueError("expect_c: one 32-byte scalar")
    ok, st = sp.status(n), sp.status(n)
    sp.call("kyb_ed25519_dleq_verify", n, sp.ptr(g), _one_or_n(g, n, "G"), sp.ptr(h), _one_or_n(h, n, "H"),
            *map(sp.ptr, t), sp.ptr(e), sp.ptr(ok), sp.ptr(st), flags)
    return ok[:n], st[:n]


def batch_xof_pick(root, pos: int, n: int):
    """(scalars, draws_used): the n scalars that n sequential Scalar.Pick calls return from ONE BLAKE2Xb stream read
    from byte position pos (kyb_ed25519_xof_pick): the challenges proof.HashVerify / HashProve read into a
    []kyber.Scalar (hash.go:68-75, 111-142).  root: the stream's 64-byte root hash.  draws_used: the 32-byte draws
    consumed, the n-th accepted one included -- the stream continues at pos + 32 * draws_used.  A Python int for host
    buffers; for a CUDA root a one-element int64 tensor (0, with zeroed scalars, if the window fell short)."""
    sp = space_of(root)
    r = sp.rows(root, 64)
    if r.shape[0] != 1:
        raise ValueError("root: one 64-byte root hash")
    n = int(n)
    out, used = sp.out((n, 32)), sp.out((1, 8))
    sp.call("kyb_ed25519_xof_pick", n, sp.ptr(r), int(pos), sp.ptr(out), sp.ptr(used))
    if sp.is_device:
        import torch

        if n == 0:  # an empty call touches no device
            used.zero_()
        return out, used.view(torch.int64).view(-1)
    return out, int(used.view(np.uint64)[0, 0])


def batch_theta_check(a, A, U, b, B, W, T, vartime: bool = False):
    """(ok, status): ok[i] = (a[i] * (A[i] + U) + Neg(b[i]) * (B[i] + W) == T[i]), the per-element checks of the simple
    k-shuffle (thver over Xhat = X + U, Yhat = Y + W, simple.go:178-183, 225-242) as ONE engine call
    (kyb_ed25519_theta_check).  a, A, b, B, T: n x 32 bytes; U, W: None or one 32-byte point shared by the batch.
    Neg(b) is the scalar -b mod l; a is used unreduced, as batch_mul2 uses it.  status[i] != 0 where A[i], B[i], U or W
    does not decode; a T that is no curve point gives ok = 0 with status 0."""
    sp = space_of(a)
    t = _rows32(sp, (a, A, b, B, T))
    n = t[0].shape[0]
    u, w = (None if x is None else sp.rows(x, 32) for x in (U, W))
    if any(x is not None and x.shape[0] != 1 for x in (u, w)):
        raise ValueError("U, W: None or one 32-byte point")
    ok, st = sp.status(n), sp.status(n)
    sp.call("kyb_ed25519_theta_check", n, sp.ptr(t[0]), sp.ptr(t[1]), sp.ptr(u), sp.ptr(t[2]), sp.ptr(t[3]), sp.ptr(w),
            sp.ptr(t[4]), sp.ptr(ok), sp.ptr(st), KYB_F_VARTIME if vartime else 0)
    return ok[:n], st[:n]


def batch_lincomb(scalars, own, shared, expect=None, want_out: bool = True, vartime: bool = False):
    """(out, ok, status): out[i] = sum_j scalars[i][j] * own[i][j] + sum_j scalars[i][ko + j] * shared[j] as ONE
    Straus-Shamir chain (kyb_ed25519_lincomb): the commitment and the check of a Rep predicate (proof.go:203-237,
    298-322).  scalars: an (n, ko + ks, 32) array or tensor, the own terms first; own: None or (n, ko, 32); shared: a
    sequence of ks entries, each 32 bytes or None -- None is Mul(s, nil), the standard base with batch_mul_base's value
    whatever `vartime` says; every other term has batch_mul's value under `vartime`.  expect: None or n x 32 bytes;
    ok[i] = 1 iff the sum's encoding equals the canonical bytes of expect[i].  out is None with want_out False, ok is None
    without expect.  status[i] != 0, with out[i] zero and ok[i] = 0, where an own point of element i or a shared point
    does not decode.  The engine call runs on the current device."""
    shared = list(shared or ())
    ks = len(shared)
    nil_mask = sum(1 << j for j, p in enumerate(shared) if p is None)
    sp = space_of(scalars)
    if len(scalars.shape) != 3 or scalars.shape[2] != 32 or (own is not None and tuple(own.shape[::2]) != (scalars.shape[0], 32)):
        raise ValueError("scalars: (n, ko + ks, 32); own: None or (n, ko, 32)")
    n, k = scalars.shape[0], scalars.shape[1]
    ko = own.shape[1] if own is not None else 0
    if k != ko + ks or k == 0:
        raise ValueError("one scalar per term")
    s32 = sp.rows(scalars, 32)
    o32 = sp.rows(own, 32) if ko else None
    sh = sp.rows(b"".join(bytes(32) if p is None else bytes(p) for p in shared), 32) if ks else None
    e = sp.rows(expect, 32) if expect is not None else None
    if e is not None and e.shape[0] != n:
        raise ValueError("expect: one point per element")
    if not want_out and e is None:
        raise ValueError("nothing asked for: want_out or expect")
    out = sp.out((n or 1, 32)) if want_out else None
    ok = sp.status(n) if e is not None else None
    st = sp.status(n)
    sp.call("kyb_ed25519_lincomb", n, ko, ks, sp.ptr(s32), sp.ptr(o32), sp.ptr(sh), nil_mask, sp.ptr(e), sp.ptr(out),
            sp.ptr(ok), sp.ptr(st), KYB_F_VARTIME if vartime else 0)
    return (out[:n] if want_out else None), (ok[:n] if e is not None else None), st[:n]


def batch_fs_challenge(names, data):
    """(c, status): c[i] = Scalar.Pick(X) with X = blake2xb.New(names[i]), X.Reseed(), X.Write(data[i]): the challenge
    hashVerifier.PubRand draws after the prover's messages (hash.go:111-142), one lane per proof
    (kyb_ed25519_fs_challenge).  data: n rows of equal length, a multiple of 32 bytes ((n, len) array or tensor); a length
    of 0 means no reseed (hash.go:46-65).  names: ONE name (bytes) shared by the batch, a sequence of n byte strings, or
    -- next to CUDA data -- (blob uint8, n + 1 int64 offsets) already on the device."""
    sp = space_of(data)
    if sp.is_device:
        d = data.contiguous()
        n, dl = d.shape[0], d.shape[1]
    else:
        d = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
        if d.ndim != 2:
            raise ValueError("data: an (n, len) array")
        n, dl = d.shape
    if dl % 32:
        raise ValueError("data: rows of a multiple of 32 bytes")
    blob, off, nl = None, None, 0
    if isinstance(names, (bytes, bytearray)):  # one name for the batch
        nl = len(names)
        if nl:
            blob = sp.rows(bytes(names), 1)
    elif sp.is_device and isinstance(names, tuple) and _is_torch(names[0]):  # packed on the device
        blob, off = _any_msgs(sp, names, n, "names/data length mismatch")
    else:  # a sequence of host byte strings
        if len(names) != n:
            raise ValueError("names/data length mismatch")
        blob, off = _device_msgs(sp, names) if sp.is_device else pack_msgs(names)
    if dl == 0:
        d = None
    c, st = sp.out((n or 1, 32)), sp.status(n)
    sp.call("kyb_ed25519_fs_challenge", n, sp.ptr(blob), sp.ptr(off), nl, sp.ptr(d), dl, sp.ptr(c), sp.ptr(st))
    return c[:n], st[:n]


def _device_msgs(sp, msgs):
    """a sequence of host byte strings as (blob, offsets) on the device"""
    import torch

    blob, off = pack_msgs(msgs)
    return torch.from_numpy(blob.copy()).to(sp.device), torch.from_numpy(off.view(np.int64).copy()).to(sp.device)


def _u32(sp, x, n: int, what: str):
    """n 32-bit indices: uint32 on the host, int32 on the device (the same four bytes)"""
    if sp.is_device:
        import torch

        if not _is_torch(x):
            x = torch.from_numpy(np.asarray(x, dtype=np.uint32).view(np.int32).copy())
        if x.dtype not in (torch.int32, torch.uint32) and x.numel() and (int(x.min()) < 0 or int(x.max()) >= 2**32):
            raise ValueError(f"{what}: indices are 32-bit")
        v = x.to(sp.device).contiguous().to(torch.int32).view(-1)  # (2^31 .. 2^32 - 1 wrap to the same four bytes)
    else:
        v = np.ascontiguousarray(np.asarray(x, dtype=np.uint32)).reshape(-1)
    if tuple(v.shape) != (n,):
        raise ValueError(f"{what}: one index per check")
    return v


def _split(blob, off, n: int, shorter: int):
    """the n elements of a packed host output as byte strings, each `shorter` bytes short of its slot"""
    raw = blob.tobytes()
    return [raw[int(off[i]):max(int(off[i]), int(off[i + 1]) - shorter)] for i in range(n)]


def batch_ecies_seal(r, pubs, msgs):
    """(ctx, status): ctx[i] = ecies.Encrypt(group, pubs[i], msgs[i], sha256) with the ephemeral scalar r[i]
    (ecies.go:23-69) as ONE engine call (kyb_ed25519_ecies_seal): R = r B, then AES-256-GCM under the key and nonce that
    HKDF-SHA256 derives from r pub; 48 bytes longer than the message.  r: n x 32 bytes; pubs: n x 32 bytes or ONE
    recipient.  Host inputs take msgs as a sequence of byte strings and return a list of byte strings; CUDA tensors take
    (blob uint8, n + 1 int64 offsets) and return (blob, offsets) with ciphertext i at offsets[i] + 48 i.
    status[i] != 0, with an all-zero ciphertext, where pubs[i] does not decode."""
    sp = space_of(r)
    rr, p = sp.rows(r, 32), sp.rows(pubs, 32)
    n = rr.shape[0]
    blob, off = _any_msgs(sp, msgs, n, "r/msgs length mismatch")
    stride = _one_or_n(p, n, "pubs") if n else 32
    total = int(off[-1]) if n else 0  # (slots are addressed by the offsets as they are)
    out, st = sp.out(total + 48 * n or 1), sp.status(n)
    sp.call("kyb_ed25519_ecies_seal", n, sp.ptr(rr), sp.ptr(p), stride, sp.ptr(blob), sp.ptr(off), sp.ptr(out), sp.ptr(st))
    if sp.is_device:
        import torch

        return (out, off.to(torch.int64) + 48 * torch.arange(n + 1, device=sp.device)), st[:n]
    return _split(out, [int(off[i]) + 48 * i for i in range(n + 1)], n, 0), st[:n]


def batch_ecies_open(privs, ctx):
    """(msgs, status): msgs[i] = ecies.Decrypt(group, privs[i], ctx[i], sha256) (ecies.go:77-112) as ONE engine call
    (kyb_ed25519_ecies_open).  privs: n x 32 bytes or ONE receiver of every ciphertext.  Host inputs take ctx as a sequence
    of byte strings and return a list of byte strings (empty where status[i] != 0); CUDA tensors take (blob, n + 1 int64
    offsets) and return (blob, offsets): plaintext i lies at offsets[i], 48 bytes shorter than its slot, zero behind it.
    status[i]: _lib.ST_ECIES_SHORT, ST_BAD_POINT (R does not decode), ST_ECIES_AUTH, in the reference's order."""
    sp = space_of(privs)
    x = sp.rows(privs, 32)
    n = len(ctx) if not sp.is_device else ctx[1].numel() - 1
    blob, off = _any_msgs(sp, ctx, n, "ctx length mismatch")
    stride = _one_or_n(x, n, "privs") if n else 32
    total = int(off[-1]) if n else 0
    out, st = sp.out(total or 1), sp.status(n)
    sp.call("kyb_ed25519_ecies_open", n, sp.ptr(x), stride, sp.ptr(blob), sp.ptr(off), sp.ptr(out), sp.ptr(st))
    if sp.is_device:
        return (out, off), st[:n]
    msgs = _split(out, off, n, 48)
    return [m if not st[i] else b"" for i, m in enumerate(msgs)], st[:n]


def batch_deal_check(poly, idx, shares, commits, m: int, t: int):
    """(ok, status): ok[i] = Equal(Mul(shares[i], nil), PubPoly(commits of polynomial poly[i]).Eval(idx[i]).V), the share
    check of share/dkg's ProcessDeals and ProcessJustifications (dkg.go:488-495, 824-832) as ONE engine call
    (kyb_ed25519_deal_check).  commits: m polynomials of t encoded points on the standard base, m t x 32 bytes.
    status has one entry per polynomial: != 0 where one of its commitments does not decode; its checks then give 0."""
    sp = space_of(shares)
    s = sp.rows(shares, 32)
    n, m, t = s.shape[0], int(m), int(t)
    c = sp.rows(commits, 32) if m * t else sp.out((1, 32))
    if m * t and c.shape[0] != m * t:
        raise ValueError("commits: m polynomials of t points")
    pl, ix = _u32(sp, poly, n, "poly"), _u32(sp, idx, n, "idx")
    ok, st = sp.status(n), sp.status(m)
    if sp.is_device and n == 0:  # the engine leaves an empty call's status unwritten: cleared here
        st.zero_()
    sp.call("kyb_ed25519_deal_check", n, sp.ptr(pl), sp.ptr(ix), sp.ptr(s), m, t, sp.ptr(c), sp.ptr(ok), sp.ptr(st))
    return ok[:n], st[:m]


def batch_schnorr_sign(k, privs, msgs):
    """(sigs, status): sigs[i] = schnorr.Sign(privs[i], msgs[i]) under the nonce k[i] (schnorr.go:56-82) as ONE engine call
    (kyb_ed25519_schnorr_sign): R = k B and A = x B on the comb with one shared inversion, h = SHA-512(R || A || msg)
    mod l, S = k + h x mod l.  k: n x 32 bytes; privs: n x 32 bytes or ONE signer.  msgs as in batch_ecies_seal.
    sigs: n x 64 bytes."""
    sp = space_of(k)
    kk, x = sp.rows(k, 32), sp.rows(privs, 32)
    n = kk.shape[0]
    blob, off = _any_msgs(sp, msgs, n, "k/msgs length mismatch")
    stride = _one_or_n(x, n, "privs") if n else 32
    sigs, st = sp.out((n or 1, 64)), sp.status(n)
    sp.call("kyb_ed25519_schnorr_sign", n, sp.ptr(kk), sp.ptr(x), stride, sp.ptr(blob), sp.ptr(off), sp.ptr(sigs), sp.ptr(st))
    return sigs[:n], st[:n]


def batch_eddsa_expand(seeds):
    """(secrets, prefixes, pubs), n x 32 bytes each: Curve.NewKeyAndSeedWithInput(seeds[i]) and Mul(secret, nil)
    (curve.go:51-60, eddsa.go:50-51, 81-86) as ONE engine call (kyb_ed25519_eddsa_expand): SHA-512 of the seed, its first
    half clamped and kept unreduced, its second half the prefix, and secret B on the comb with one shared inversion."""
    sp = space_of(seeds)
    s = sp.rows(seeds, 32)
    n = s.shape[0]
    secrets, prefixes, pubs = (sp.out((n or 1, 32)) for _ in range(3))
    sp.call("kyb_ed25519_eddsa_expand", n, sp.ptr(s), sp.ptr(secrets), sp.ptr(prefixes), sp.ptr(pubs))
    return secrets[:n], prefixes[:n], pubs[:n]


def batch_eddsa_sign(secrets, prefixes, pubs, msgs):
    """(sigs, status): sigs[i] = (*EdDSA).Sign(msgs[i]) under the key (secrets[i], prefixes[i], pubs[i]) (eddsa.go:91-142)
    as ONE engine call (kyb_ed25519_eddsa_sign): r = SHA-512(prefix || msg) mod l and R = r B on the comb, one shared
    inversion, h = SHA-512(R || pub || msg) mod l, S = r + h secret mod l.  A key's three parts as batch_eddsa_expand
    gives them: n x 32 bytes each, or 32 bytes each for ONE key signing every message.  msgs as in batch_ecies_seal.
    sigs: n x 64 bytes."""
    sp = space_of(secrets)
    a, p, A = sp.rows(secrets, 32), sp.rows(prefixes, 32), sp.rows(pubs, 32)
    if p.shape != a.shape or A.shape != a.shape:
        raise ValueError("secrets/prefixes/pubs length mismatch")
    n = len(msgs) if not sp.is_device else msgs[1].numel() - 1
    blob, off = _any_msgs(sp, msgs, n, "msgs length mismatch")
    stride = _one_or_n(a, n, "keys") if n else 32
    sigs, st = sp.out((n or 1, 64)), sp.status(n)
    sp.call("kyb_ed25519_eddsa_sign", n, sp.ptr(a), sp.ptr(p), sp.ptr(A), stride, sp.ptr(blob), sp.ptr(off), sp.ptr(sigs), sp.ptr(st))
    return sigs[:n], st[:n]


def _ctx_rows(sp, ctx, n: int, ctx_len: int):
    """(rows, stride, length): a context of ctx_len bytes for the batch (stride 0) or one per element"""
    if ctx_len not in (32, 128):
        raise ValueError("ctx: 32 bytes (share/vss/pedersen) or 128 (share/vss/rabin)")
    c = sp.rows(ctx, ctx_len)
    if c.shape[0] == 1:
        return c, 0, ctx_len
    if c.shape[0] != n:
        raise ValueError("ctx: one context or one per element")
    return c, ctx_len, ctx_len


def batch_vss_seal(dh, k, dealer_priv, dealer_pub, pubs, ctx, msgs, ctx_len: int = 32):
    """(dhkeys, sigs, ciphers, status): share/vss Dealer.EncryptedDeal (pedersen/vss.go:222-255) for the n verifiers of
    one dealer as ONE engine call (kyb_ed25519_vss_seal): dhkeys[i] = dh[i] B, sigs[i] = schnorr.Sign(dealer_priv,
    dhkeys[i]) under the nonce k[i], ciphers[i] = AES-256-GCM.Seal(key, 0^12, msgs[i], ctx) with the key HKDF-SHA256
    derives from dh[i] pubs[i] and ctx.  ctx: ctx_len bytes (32: pedersen, 128: rabin) for the batch or n x ctx_len.  Host inputs take msgs as a sequence of
    byte strings and return ciphers as a list; CUDA tensors take (blob, n + 1 int64 offsets) and return (blob, offsets)
    with cipher i at offsets[i] + 16 i.  status[i] != 0, with all three outputs zero, where pubs[i] does not decode."""
    sp = space_of(dh)
    d, kk, p = sp.rows(dh, 32), sp.rows(k, 32), sp.rows(pubs, 32)
    n = d.shape[0]
    if kk.shape != d.shape or p.shape != d.shape:
        raise ValueError("dh/k/pubs length mismatch")
    x, a = sp.rows(dealer_priv, 32), sp.rows(dealer_pub, 32)
    if x.shape[0] != 1 or a.shape[0] != 1:
        raise ValueError("one dealer")
    c, cstride, clen = _ctx_rows(sp, ctx, n, ctx_len)
    blob, off = _any_msgs(sp, msgs, n, "dh/msgs length mismatch")
    total = int(off[-1]) if n else 0
    keys, sigs, out, st = sp.out((n or 1, 32)), sp.out((n or 1, 64)), sp.out(total + 16 * n or 1), sp.status(n)
    sp.call("kyb_ed25519_vss_seal", n, sp.ptr(d), sp.ptr(kk), sp.ptr(x), sp.ptr(a), sp.ptr(p), sp.ptr(c), cstride, clen, sp.ptr(blob),
            sp.ptr(off), sp.ptr(keys), sp.ptr(sigs), sp.ptr(out), sp.ptr(st))
    if sp.is_device:
        import torch

        return keys[:n], sigs[:n], (out, off.to(torch.int64) + 16 * torch.arange(n + 1, device=sp.device)), st[:n]
    return keys[:n], sigs[:n], _split(out, [int(off[i]) + 16 * i for i in range(n + 1)], n, 0), st[:n]


def batch_vss_open(privs, dhkeys, ctx, ciphers, ctx_len: int = 32):
    """(msgs, status): the second half of share/vss decryptDeal (pedersen/vss.go:443-457) as ONE engine call
    (kyb_ed25519_vss_open): pre = privs[i] dhkeys[i], the key derivation of batch_vss_seal, Open under the zero nonce
    with ctx as additional data.  privs: n x 32 bytes or ONE receiver.  Host inputs take ciphers as a sequence of byte
    strings and return a list (empty where status[i] != 0); CUDA tensors take and return (blob, offsets): plaintext i at
    offsets[i], 16 bytes shorter than its slot, zero behind it.  status[i]: _lib.ST_ECIES_SHORT, ST_BAD_POINT (the key
    does not decode), ST_ECIES_AUTH, in this precedence."""
    sp = space_of(dhkeys)
    kk = sp.rows(dhkeys, 32)
    n = kk.shape[0]
    x = sp.rows(privs, 32)
    c, cstride, clen = _ctx_rows(sp, ctx, n, ctx_len)
    blob, off = _any_msgs(sp, ciphers, n, "dhkeys/ciphers length mismatch")
    stride = _one_or_n(x, n, "privs") if n else 32
    total = int(off[-1]) if n else 0
    out, st = sp.out(total or 1), sp.status(n)
    sp.call("kyb_ed25519_vss_open", n, sp.ptr(x), stride, sp.ptr(kk), sp.ptr(c), cstride, clen, sp.ptr(blob), sp.ptr(off), sp.ptr(out),
            sp.ptr(st))
    if sp.is_device:
        return (out, off), st[:n]
    msgs = _split(out, off, n, 16)
    return [m if not st[i] else b"" for i, m in enumerate(msgs)], st[:n]


def batch_deal_check2(poly, idx, f_shares, g_shares, commits, H, m: int, t: int):
    """(ok, status): ok[i] = Equal(Add(Mul(f_shares[i], nil), Mul(g_shares[i], H_k)), PubPoly(commits of polynomial
    k = poly[i]).Eval(idx[i]).V), Rabin's VerifyDeal equation (rabin/vss.go:611-651), as ONE engine call
    (kyb_ed25519_deal_check2).  H: one 32-byte point for the batch or m x 32 bytes, one per polynomial.  status has one
    entry per polynomial: != 0 where one of its commitments or its H does not decode; its checks then give 0."""
    sp = space_of(f_shares)
    f, g = sp.rows(f_shares, 32), sp.rows(g_shares, 32)
    if f.shape != g.shape:
        raise ValueError("f/g length mismatch")
    n, m, t = f.shape[0], int(m), int(t)
    c = sp.rows(commits, 32) if m * t else sp.out((1, 32))
    if m * t and c.shape[0] != m * t:
        raise ValueError("commits: m polynomials of t points")
    h = sp.rows(H, 32)
    if h.shape[0] == 1:
        hstride = 0
    elif h.shape[0] == m:
        hstride = 32
    else:
        raise ValueError("H: one point or one per polynomial")
    pl, ix = _u32(sp, poly, n, "poly"), _u32(sp, idx, n, "idx")
    ok, st = sp.status(n), sp.status(m)
    if sp.is_device and n == 0:  # the engine leaves an empty call's status unwritten: cleared here
        st.zero_()
    sp.call("kyb_ed25519_deal_check2", n, sp.ptr(pl), sp.ptr(ix), sp.ptr(f), sp.ptr(g), m, t, sp.ptr(c), sp.ptr(h), hstride,
            sp.ptr(ok), sp.ptr(st))
    return ok[:n], st[:m]


def _dss_commits(sp, long_commits, rand_commits, ns: int):
    """(long rows, random rows, tl, tr): ONE long-term polynomial, ns random ones of one threshold"""
    lc, rc = sp.rows(long_commits, 32), sp.rows(rand_commits, 32)
    tl = lc.shape[0]
    if ns == 0 or rc.shape[0] % ns:
        raise ValueError("rand_commits: ns polynomials of tr points")
    return lc, rc, tl, rc.shape[0] // ns


def batch_dss_check(participants, long_commits, rand_commits, msgs, sess, idx, V, sid, sigs):
    """(ok, status, sess_status): sign/dss ProcessPartialSig (dss.go:141-173) without its sequential state for n partial
    signatures over the ns sessions of ONE long-term key and ONE roster, as ONE engine call (kyb_ed25519_dss_check).
    participants: np x 32 bytes; long_commits: tl x 32; rand_commits: ns tr x 32; msgs: one message per session (as in
    batch_schnorr_sign); sess, idx: n uint32, the session and the signer of partial i; V, sid: n x 32; sigs: n x 64.
    status[i], in the reference's order: _lib.ST_DSS_INDEX, the signature's status as batch_verify reports it or
    ST_DSS_SIG, ST_DSS_SESSION, ST_BAD_POINT (the session's commitments), ST_DSS_PARTIAL; ok[i] = 1 only with 0.
    sess_status[b] != 0 where a commitment of session b does not decode."""
    sp = space_of(V)
    v, s, g = sp.rows(V, 32), sp.rows(sid, 32), sp.rows(sigs, 64)
    n = v.shape[0]
    if s.shape[0] != n or g.shape[0] != n:
        raise ValueError("V/sid/sigs length mismatch")
    ns = len(msgs) if not sp.is_device else msgs[1].numel() - 1
    if n == 0:
        return sp.status(0)[:0], sp.status(0)[:0], sp.status(0)[:0]
    pk = sp.rows(participants, 32)
    lc, rc, tl, tr = _dss_commits(sp, long_commits, rand_commits, ns)
    blob, off = _any_msgs(sp, msgs, ns, "rand_commits/msgs length mismatch")
    se, ix = _u32(sp, sess, n, "sess"), _u32(sp, idx, n, "idx")
    ok, st, sst = sp.status(n), sp.status(n), sp.status(ns)
    sp.call("kyb_ed25519_dss_check", n, pk.shape[0], sp.ptr(pk), tl, sp.ptr(lc), ns, tr, sp.ptr(rc), sp.ptr(blob), sp.ptr(off),
            sp.ptr(se), sp.ptr(ix), sp.ptr(v), sp.ptr(s), sp.ptr(g), sp.ptr(ok), sp.ptr(st), sp.ptr(sst))
    return ok[:n], st[:n], sst[:ns]


def batch_dss_partial(priv, index: int, alpha, beta, k, long_commits, rand_commits, msgs):
    """(V, sid, sigs): sign/dss PartialSig (dss.go:113-134) for the ns sessions of one signer as ONE engine call
    (kyb_ed25519_dss_partial).  priv: the long-term secret; index: its place in the roster; alpha: the share of the
    long-term key; beta, k: ns x 32, the shares of the random keys and the Schnorr nonces.  V[b] = h_b alpha + beta_b,
    sid[b] the session id, sigs[b] = schnorr.Sign(priv, SHA-256(SHA-256(V[b] || u32le(index)) || sid[b])) under k[b]."""
    sp = space_of(beta)
    b, kk = sp.rows(beta, 32), sp.rows(k, 32)
    ns = b.shape[0]
    if kk.shape[0] != ns:
        raise ValueError("beta/k length mismatch")
    if ns == 0:
        return sp.out((0, 32)), sp.out((0, 32)), sp.out((0, 64))
    x, a = sp.rows(priv, 32), sp.rows(alpha, 32)
    if x.shape[0] != 1 or a.shape[0] != 1:
        raise ValueError("one signer")
    lc, rc, tl, tr = _dss_commits(sp, long_commits, rand_commits, ns)
    blob, off = _any_msgs(sp, msgs, ns, "beta/msgs length mismatch")
    V, sid, sigs = sp.out((ns, 32)), sp.out((ns, 32)), sp.out((ns, 64))
    sp.call("kyb_ed25519_dss_partial", ns, sp.ptr(x), int(index), sp.ptr(a), sp.ptr(b), sp.ptr(kk), tl, sp.ptr(lc), tr, sp.ptr(rc),
            sp.ptr(blob), sp.ptr(off), sp.ptr(V), sp.ptr(sid), sp.ptr(sigs))
    return V, sid, sigs


def _scope_arg(sp, scope):
    """(buffer, length) of a link scope: None stays None (unlinkable); an empty scope keeps a non-NULL pointer"""
    if scope is None:
        return None, 0
    if _is_torch(scope):
        return sp.rows(scope if scope.numel() else scope.new_zeros(1), 1), scope.numel()
    b = bytes(scope)
    return sp.rows(b or b"\0", 1), len(b)


def _any_msgs(sp, msgs, n: int, mismatch: str):
    """(blob, offsets) of n messages of any lengths: a sequence of byte strings on the host, (blob uint8, n + 1 64-bit
    offsets) already packed on the device"""
    if not sp.is_device:
        if len(msgs) != n:
            raise ValueError(mismatch)
        return pack_msgs(msgs)
    import torch

    blob, off = msgs
    blob, off = blob.contiguous(), off.contiguous()
    if off.dtype not in (torch.int64, torch.uint64) or off.numel() != n + 1:
        raise ValueError("msgs: (blob, n + 1 64-bit offsets)")
    if blob.numel() == 0:
        blob = torch.zeros(1, dtype=torch.uint8, device=sp.device)
    return blob, off


def _ring_start(sp, start, n: int):
    """one start position per signature: uint32 on the host, int32 on the device (the same four bytes)"""
    if start is None:
        return None
    if sp.is_device:
        import torch

        s = start.contiguous().to(torch.int32).view(-1)
    else:
        s = np.ascontiguousarray(np.asarray(start, dtype=np.uint32))
    if tuple(s.shape) != (n,):
        raise ValueError("start: one position per signature")
    return s


def _ring_stride(k, n: int, ring: int) -> int:
    """0 for one ring shared by the batch (one row, whatever n), 32 * ring for one ring per signature"""
    if k.shape[0] == 1:
        return 0
    if k.shape[0] == n:
        return 32 * ring
    raise ValueError("keys: one ring or one per signature")


def batch_ring_chain(keys, msgs, scope, link_base, sigs, ring: int, start=None, steps=None, vartime: bool = False):
    """(c_zero, c_out, ok, status): the ring loop of sign/anon for n signatures as ONE engine call
    (kyb_ed25519_ring_chain) -- Verify's loop (sig.go:231-238) with start None and steps None (= ring), the open ring of
    Sign (sig.go:159-166) with start = mine + 1 and steps = ring - 1.  keys: ring x 32 bytes shared by the batch or
    n x ring x 32 bytes; scope: None (unlinkable) or the link scope with link_base = Point.Pick(XOF(scope));
    sigs: n rows of c_0 || s_0 .. s_{ring-1} || [tag].  Host inputs take msgs as a sequence of byte strings; CUDA
    tensors take msgs as (blob uint8, offsets int64 of n + 1 entries) and run on the current stream."""
    ring = int(ring)
    steps = ring if steps is None else int(steps)
    slots = ring + (2 if scope is not None else 1)
    if ring <= 0:
        raise ValueError("empty ring")
    if (scope is None) != (link_base is None):
        raise ValueError("a link scope and its base go together")
    sp = space_of(sigs)
    sg = sp.rows(_joined(sigs), 32 * slots)
    n = sg.shape[0]
    k = sp.rows(_joined(keys), 32 * ring)
    blob, off = _any_msgs(sp, msgs, n, "msgs/sigs length mismatch")
    sc, sl = _scope_arg(sp, scope)
    lb = sp.rows(link_base, 32) if link_base is not None else None
    if lb is not None and sp.is_device and lb.shape[0] != 1:  # (the host entry point reads the first 32 bytes)
        raise ValueError("link_base: one 32-byte point")
    stt = _ring_start(sp, start, n)
    cz, co, ok, st = sp.out((n or 1, 32)), sp.out((n or 1, 32)), sp.status(n), sp.status(n)
    sp.call("kyb_ed25519_ring_chain", n, ring, sp.ptr(k), _ring_stride(k, n, ring), sp.ptr(blob), sp.ptr(off), sp.ptr(sc), sl,
            sp.ptr(lb), sp.ptr(sg), 32 * slots, sp.ptr(stt), steps, sp.ptr(cz), sp.ptr(co), sp.ptr(ok), sp.ptr(st),
            KYB_F_VARTIME if vartime else 0)
    return cz[:n], co[:n], ok[:n], st[:n]


def batch_ring_challenge(msgs, scope, tags, PG, PH):
    """(c, status): c[i] = signH1(signH1pre(msgs[i], scope, tags[i]), PG[i], PH[i]) (sign/anon, sig.go:23-43), one lane per
    element (kyb_ed25519_ring_challenge: BLAKE2Xb keyed with the first 64 message bytes and Pick's rejection loop on the
    device).  scope, tags and PH are None for unlinkable signatures.  msgs as in batch_ring_chain."""
    if (scope is None) != (tags is None) or (scope is None) != (PH is None):
        raise ValueError("scope, tags and PH go together")
    sp = space_of(PG)
    pg = sp.rows(PG, 32)
    n = pg.shape[0]
    tg = sp.rows(tags, 32) if tags is not None else None
    ph = sp.rows(PH, 32) if PH is not None else None
    if any(x is not None and x.shape != pg.shape for x in (tg, ph)):
        raise ValueError("length mismatch")
    blob, off = _any_msgs(sp, msgs, n, "length mismatch")
    sc, sl = _scope_arg(sp, scope)
    c, st = sp.out((n or 1, 32)), sp.status(n)
    sp.call("kyb_ed25519_ring_challenge", n, sp.ptr(blob), sp.ptr(off), sp.ptr(sc), sl, sp.ptr(tg), sp.ptr(pg), sp.ptr(ph),
            sp.ptr(c), sp.ptr(st))
    return c[:n], st[:n]


def batch_anon_seal(keys, x, msgs, ring: int):
    """(ctx, status): ctx[i] = anon.Encrypt(suite, msgs[i], set) under the ephemeral private key x[i] (enc.go:123-148) as
    ONE engine call (kyb_ed25519_anon_seal): X = x B, one slot per ring member -- xb = x mod l under BLAKE2Xb keyed with
    the bytes of x Y -- then the message under BLAKE2Xb(xb) and its 16-byte MAC; 48 + 32 ring bytes longer than the
    message.  keys: ring x 32 bytes shared by the batch or n x ring x 32 bytes; x: n x 32 bytes, used unreduced.  Host
    inputs take msgs as a sequence of byte strings and return a list of byte strings; CUDA tensors take (blob uint8,
    n + 1 int64 offsets) and return (blob, offsets).  status[i] != 0, with an all-zero ciphertext, where a ring member
    does not decode."""
    ring = int(ring)
    if not 0 < ring <= _lib.ANON_MAX_RING:
        raise ValueError("an anonymity set of 1 .. %d keys" % _lib.ANON_MAX_RING)
    sp = space_of(x)
    xx = sp.rows(x, 32)
    n = xx.shape[0]
    k = sp.rows(_joined(keys), 32 * ring)
    blob, off = _any_msgs(sp, msgs, n, "x/msgs length mismatch")
    over = 48 + 32 * ring
    total = int(off[-1]) if n else 0  # (slots are addressed by the offsets as they are)
    out, st = sp.out(total + over * n or 1), sp.status(n)
    sp.call("kyb_ed25519_anon_seal", n, ring, sp.ptr(k), _ring_stride(k, n, ring), sp.ptr(xx), sp.ptr(blob), sp.ptr(off), sp.ptr(out),
            sp.ptr(st))
    if sp.is_device:
        import torch

        return (out, off.to(torch.int64) + over * torch.arange(n + 1, device=sp.device)), st[:n]
    return _split(out, [int(off[i]) + over * i for i in range(n + 1)], n, 0), st[:n]


def batch_anon_open(keys, mine, privs, ctx, ring: int):
    """(msgs, status): msgs[i] = anon.Decrypt(suite, ctx[i], set, mine[i], privs[i]) (enc.go:165-192) as ONE engine call
    (kyb_ed25519_anon_open): xb from slot mine[i], x B against X, EVERY member's slot recomputed and compared, the MAC,
    then the plaintext.  keys as in batch_anon_seal; mine: n positions; privs: n x 32 bytes or ONE receiver.  Host inputs
    take ctx as a sequence of byte strings and return a list of byte strings (empty where status[i] != 0); CUDA tensors
    take (blob, n + 1 int64 offsets) and return (blob, offsets): plaintext i lies at offsets[i], zero behind it.
    status[i]: _lib.ST_ANON_SHORT, ST_BAD_POINT, ST_ANON_INVALID, ST_ANON_MAC, in the reference's order."""
    ring = int(ring)
    if not 0 < ring <= _lib.ANON_MAX_RING:
        raise ValueError("an anonymity set of 1 .. %d keys" % _lib.ANON_MAX_RING)
    sp = space_of(privs)
    p = sp.rows(privs, 32)
    n = len(ctx) if not sp.is_device else ctx[1].numel() - 1
    k = sp.rows(_joined(keys), 32 * ring)
    m = _u32(sp, mine, n, "mine")
    blob, off = _any_msgs(sp, ctx, n, "ctx length mismatch")
    stride = _one_or_n(p, n, "privs") if n else 32
    total = int(off[-1]) if n else 0
    out, st = sp.out(total or 1), sp.status(n)
    sp.call("kyb_ed25519_anon_open", n, ring, sp.ptr(k), _ring_stride(k, n, ring), sp.ptr(m), sp.ptr(p), stride, sp.ptr(blob), sp.ptr(off),
            sp.ptr(out), sp.ptr(st))
    if sp.is_device:
        return (out, off), st[:n]
    msgs = _split(out, off, n, 48 + 32 * ring)
    return [b if not st[i] else b"" for i, b in enumerate(msgs)], st[:n]


def _cosi_masks(sp, masks, n, m: int):
    """(buffer, n, stride) of n participation masks over m keys: a sequence of byte strings of (m + 7) >> 3 bytes each,
    or an (n, stride) uint8 array or tensor with stride >= (m + 7) >> 3 whose rows start with the mask"""
    L = (m + 7) >> 3
    if isinstance(masks, (list, tuple)):
        if any(len(x) != L for x in masks):
            raise ValueError("mismatching mask lengths")
        masks = np.frombuffer(b"".join(bytes(x) for x in masks), dtype=np.uint8).reshape(len(masks), L)
    if len(masks.shape) != 2 or masks.shape[1] < L:
        raise ValueError("masks: (n, stride) bytes, stride >= (m + 7) >> 3")
    if n is not None and masks.shape[0] != n:
        raise ValueError("one mask per element")
    stride = int(masks.shape[1])
    return sp.rows(masks, stride), int(masks.shape[0]), stride


def _cosi_roster(sp, roster):
    r = sp.rows(_joined(roster), 32)
    if r.shape[0] < 1:
        raise ValueError("empty roster")
    return r, int(r.shape[0])


def _u32_out(sp, n: int):
    """n 32-bit counts: uint32 on the host, int32 on the device (the same four bytes)"""
    if sp.is_device:
        import torch

        return torch.empty(n or 1, dtype=torch.int32, device=sp.device)
    return np.zeros(n or 1, dtype=np.uint32)


def cosi_group_width(n: int, m: int) -> int:
    """the subset-table width, 4 or 8, that a call of n elements over m keys uses (kyb_ed25519_cosi_group_width)"""
    return int(_lib.load().kyb_ed25519_cosi_group_width(int(n), int(m)))


def batch_mask_aggregate(roster, masks):
    """(out, count, status): out[i] = the sum of the roster keys that masks[i] enables, count[i] = their number: cosi
    Mask.SetMask / AggregatePublic / CountEnabled (cosi.go:300-317, 361-372) for n masks over ONE roster as ONE engine
    call (kyb_ed25519_mask_aggregate).  roster: m x 32 bytes; masks: see _cosi_masks (bit j & 7 of byte j >> 3 enables
    key j; bits at or above m are ignored).  status[i] != 0, with out[i] zero, for every i when a roster key does not
    decode.  The memory space is the masks'; the call runs on the current device."""
    sp = space_of(masks)
    r, m = _cosi_roster(sp, roster)
    mk, n, stride = _cosi_masks(sp, masks, None, m)
    out, cnt, st = sp.out((n or 1, 32)), _u32_out(sp, n), sp.status(n)
    sp.call("kyb_ed25519_mask_aggregate", n, m, sp.ptr(r), sp.ptr(mk), stride, sp.ptr(out), sp.ptr(cnt), sp.ptr(st), 0)
    return out[:n], cnt[:n], st[:n]


def batch_cosi_verify(roster, msgs, sigs, masks, want_agg: bool = False):
    """(ok, agg, count, status): ok[i] = 1 iff cosi.Verify's equation holds for (sigs[i] = V || r, masks[i]) on msgs[i]
    under the roster (cosi.go:214-232), the whole batch as ONE engine call (kyb_ed25519_cosi_verify): the aggregate key
    from the subset tables, k = SHA-512(V || A || msg) mod l, one ladder on -A with the comb for r B, and the
    comparison with V on canonical bytes.  r is reduced, not rejected; nothing is checked for small order.  agg is None
    unless want_agg; count[i] is what the policy looks at.  sigs: n x 64 bytes; msgs as in batch_ring_chain: a sequence
    of byte strings next to host buffers, (blob uint8, n + 1 int64 offsets) next to CUDA tensors."""
    sp = space_of(sigs)
    s = sp.rows(_joined(sigs), 64)
    n = int(s.shape[0])
    r, m = _cosi_roster(sp, roster)
    mk, _, stride = _cosi_masks(sp, masks, n, m)
    blob, off = _any_msgs(sp, msgs, n, "msgs/sigs length mismatch")
    agg = sp.out((n or 1, 32)) if want_agg else None
    ok, cnt, st = sp.status(n), _u32_out(sp, n), sp.status(n)
    sp.call("kyb_ed25519_cosi_verify", n, m, sp.ptr(r), sp.ptr(blob), sp.ptr(off), sp.ptr(s), sp.ptr(mk), stride, sp.ptr(agg),
            sp.ptr(cnt), sp.ptr(ok), sp.ptr(st), 0)
    return ok[:n], (agg[:n] if want_agg else None), cnt[:n], st[:n]


def batch_verify(pubs, msgs, sigs, want_status: bool = True):
    """(ok, status): ok[i] = 1 iff sign/eddsa VerifyWithChecks(pubs[i], msgs[i], sigs[i]) == nil (eddsa.go:143-229), the
    whole batch in one engine call (kyb_ed25519_verify).  pubs: n x 32 bytes, sigs: n x 64 bytes, msgs: a sequence of
    n byte strings of any lengths.  status: include/kyber_hip.h (None when want_status is False).  Host buffers."""
    sp = HOST
    p, s = sp.rows(_joined(pubs), 32), sp.rows(_joined(sigs), 64)
    n = s.shape[0]
    if p.shape[0] != n or len(msgs) != n:
        raise ValueError("pubs/msgs/sigs length mismatch")
    m, off = pack_msgs(msgs)
    ok = sp.status(n)
    st = sp.status(n) if want_status else None
    sp.call("kyb_ed25519_verify", n, sp.ptr(p), sp.ptr(m), sp.ptr(off), sp.ptr(s), sp.ptr(ok), sp.ptr(st), 0)
    return ok[:n], (st[:n] if want_status else None)


def commit(scalars, base=None, vartime: bool = False, uniform: bool = False):
    """commits[i] = coeffs[i] * b  -- share.PriPoly.Commit (share/poly.go:143-149).
    ``base`` None means the standard base point (poly.go:144 passes nil through).  uniform: the coefficients of a
    PriPoly are secrets -- KYB_F_UNIFORM keeps them out of the memory addresses.  With a base: host buffers."""
    if base is None:
        return batch_mul_base(scalars, vartime, uniform)
    flags = _flags(vartime, uniform)
    sp = HOST
    s, b = sp.rows(scalars, 32), sp.rows(base, 32)
    n = s.shape[0]
    out, st = sp.out(s.shape), sp.status(n)
    sp.call("kyb_ed25519_mul_same_base", n, sp.ptr(s), sp.ptr(b), sp.ptr(out), sp.ptr(st), flags)
    if n and st[0]:
        raise ValueError("invalid Ed25519 curve point")
    return out


def msm(scalars, points, scalar_bits: int = 256):
    """(out, status): out = sum_i scalars[i] * points[i] as one 32-byte point -- what PubPoly.Eval /
    RecoverCommit (share/poly.go:340-348, 449-476) compute with N x (Mul + Add).  Scalars are 256-bit
    little-endian integers, never reduced mod l; one whose top radix-16 digit the reference's recoding drops (>= ~2^255)
    counts as the integer the reference's Mul multiplies by, as in batch_mul.  If any status is non-zero the output is
    all-zero bytes.  scalar_bits < 256 (host buffers): every scalar is below 2^scalar_bits, higher bits are ignored
    (KYB_F_SCALAR_BITS: proportionally fewer windows)."""
    sp = space_of(scalars)
    s, p = sp.rows(scalars, 32), sp.rows(points, 32)
    if s.shape != p.shape:
        raise ValueError("scalars/points length mismatch")
    n = s.shape[0]
    out, st = sp.out(32), sp.status(n)
    if scalar_bits != 256 and not sp.is_device:
        sp.call("kyb_ed25519_msm_flags", n, sp.ptr(s), sp.ptr(p), sp.ptr(out), sp.ptr(st), scalar_bits << 16)
    else:
        sp.call("kyb_ed25519_msm", n, sp.ptr(s), sp.ptr(p), sp.ptr(out), sp.ptr(st))
    return out, st[:n]


def poly_eval(commits, indices):
    """(out, status): out[i] = sum_j commits[j] * (indices[i] + 1)^j -- share.PubPoly.Eval (share/poly.go:340-348) for
    many indices in one launch (host buffers).  status has one entry per commitment."""
    sp = HOST
    c = sp.rows(commits, 32)
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
    n, t = idx.shape[0], c.shape[0]
    out, st = sp.out((n, 32)), sp.status(t)
    sp.call("kyb_ed25519_poly_eval", n, sp.ptr(idx), t, sp.ptr(c), sp.ptr(out), sp.ptr(st))
    return out, st[:t]


def scalar_poly_eval(coeffs, indices):
    """out[i] = sum_j coeffs[j] * (indices[i] + 1)^j mod l, 32-byte little-endian scalars -- share.PriPoly.Eval
    (share/poly.go:85-93) for many indices in one launch: PriPoly.Shares (poly.go:96-102).  Host buffers."""
    sp = HOST
    c = sp.rows(coeffs, 32)
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
    n, t = idx.shape[0], c.shape[0]
    out = sp.out((n, 32))
    sp.call("kyb_ed25519_scalar_poly_eval", n, sp.ptr(idx), t, sp.ptr(c), sp.ptr(out))
    return out


def batch_unmarshal(points):
    """(out, status): N x (*point).UnmarshalBinary (point.go:65-70 -> ge.go:110-150): status[i] != 0 where the reference
    returns an error; out[i] = MarshalBinary of the accepted point (canonical y, point.go:54-58)."""
    sp = space_of(points)
    p = sp.rows(points, 32)
    n = p.shape[0]
    out, st = sp.out(p.shape), sp.status(n)
    sp.call("kyb_ed25519_unmarshal", n, sp.ptr(p), sp.ptr(out), sp.ptr(st))
    return out, st[:n]


def batch_add(a, b):
    """(out, status): out[i] = a[i] + b[i]  (N x Point.Add, point.go:216-223)."""
    sp = space_of(a)
    x, y = sp.rows(a, 32), sp.rows(b, 32)
    if x.shape != y.shape:
        raise ValueError("length mismatch")
    n = x.shape[0]
    out, st = sp.out(x.shape), sp.status(n)
    sp.call("kyb_ed25519_add", n, sp.ptr(x), sp.ptr(y), sp.ptr(out), sp.ptr(st))
    return out, st[:n]


def batch_hash(msgs, dst: bytes):
    """out[i] = Hash(msgs[i], dst): (*point).Hash (point.go:325-334, RFC 9380 edwards25519_XMD:SHA-512_ELL2_RO_)
    for n equal-length messages (list of bytes, (n, len) uint8 array or CUDA tensor)."""
    sp = space_of(msgs)
    m, n, ln = sp.msgs(msgs, "batch_hash")
    out = sp.out((n, 32))
    sp.call("kyb_ed25519_hash", n, sp.ptr(m), ln, dst_arg(dst), len(dst), sp.ptr(out))
    return out


# ------------------------------------------------------- kyber.Scalar mirror
class Scalar:
    """kyber.Scalar for Ed25519 (group/edwards25519/scalar.go:32-34): 32 bytes LE."""

    __slots__ = ("v",)

    def __init__(self, v: bytes = bytes(32)):
        self.v = bytes(v)

    # -- encoding
    def MarshalBinary(self) -> bytes:
        return (int.from_bytes(self.v, "little") % ORDER).to_bytes(32, "little")

    def UnmarshalBinary(self, buf: bytes) -> "Scalar":
        if len(buf) != 32:
            raise ValueError("wrong size buffer")
        self.v = bytes(buf)  # unreduced, scalar.go:226-233
        return self

    def MarshalSize(self) -> int:
        return 32

    def SetBytes(self, b: bytes) -> "Scalar":
        self.v = (int.from_bytes(b, "little") % ORDER).to_bytes(32, "little")
        return self

    def SetInt64(self, v: int) -> "Scalar":
        self.v = (v % ORDER).to_bytes(32, "little")
        return self

    def Zero(self) -> "Scalar":
        self.v = bytes(32)
        return self

    def One(self) -> "Scalar":
        return self.SetInt64(1)

    def Set(self, a: "Scalar") -> "Scalar":
        self.v = _sc(a).v
        return self

    def Clone(self) -> "Scalar":
        return Scalar(self.v)

    def Equal(self, a: "Scalar") -> bool:
        return self._int() % ORDER == _sc(a)._int() % ORDER

    def _int(self) -> int:
        return int.from_bytes(self.v, "little")

    def _set(self, x: int) -> "Scalar":
        self.v = (x % ORDER).to_bytes(32, "little")
        return self

    # -- arithmetic mod l (host plumbing, like group/mod.Int)
    def Add(self, a, b):
        return self._set(_sc(a)._int() + _sc(b)._int())

    def Sub(self, a, b):
        return self._set(_sc(a)._int() - _sc(b)._int())

    def Neg(self, a):
        return self._set(-_sc(a)._int())

    def Mul(self, a, b):
        return self._set(_sc(a)._int() * _sc(b)._int())

    def Inv(self, a):
        return self._set(pow(_sc(a)._int() % ORDER, ORDER - 2, ORDER))

    def Div(self, a, b):
        return self._set(_sc(a)._int() * pow(_sc(b)._int() % ORDER, ORDER - 2, ORDER))

    def Pick(self, rand=None) -> "Scalar":
        """rand: a callable returning n bytes (64 are reduced mod l), or a kyber.XOF mirror (util/blake2xb.XOF) -- then
        this is the reference's Pick: 32 stream bytes big-endian, 253 bits, redrawn until below l (scalar.go:180-184)."""
        if hasattr(rand, "XORKeyStream"):
            from ..util import blake2xb

            self.v = blake2xb.pick(rand.Read)
            return self
        raw = rand(64) if rand is not None else os.urandom(64)
        return self._set(int.from_bytes(raw, "little"))

    def String(self) -> str:
        return self.MarshalBinary().hex()

    __repr__ = String


def _sc(s) -> Scalar:
    if not isinstance(s, Scalar):
        raise TypeError("ErrTypeCast: not an edwards25519 scalar")
    return s


# -------------------------------------------------------- kyber.Point mirror
class Point:
    """kyber.Point for Ed25519 holding the canonical 32-byte encoding; every
    operation that needs curve arithmetic is one (batch-of-one) engine call."""

    __slots__ = ("enc", "var_time")

    def __init__(self, enc: bytes = _NULL_ENC):
        self.enc = bytes(enc)
        self.var_time = False

    def AllowVarTime(self, on: bool) -> None:  # point_vartime.go:9
        self.var_time = bool(on)

    def MarshalBinary(self) -> bytes:
        return self.enc

    def MarshalSize(self) -> int:
        return 32

    def UnmarshalBinary(self, b: bytes) -> "Point":
        if len(b) != 32:
            raise ValueError("invalid Ed25519 curve point")
        one = (1).to_bytes(32, "little")
        out, st = batch_mul(one, b)
        if st[0]:
            raise ValueError("invalid Ed25519 curve point")
        # the reference keeps the decoded point; its re-encoding is canonical
        self.enc = bytes(out[0])
        return self

    def Null(self) -> "Point":
        self.enc = _NULL_ENC
        return self

    def Base(self) -> "Point":
        self.enc = _BASE_ENC
        return self

    def Set(self, p: "Point") -> "Point":
        self.enc = _pt(p).enc
        return self

    def Clone(self) -> "Point":
        return Point(self.enc)

    def Equal(self, p: "Point") -> bool:
        return self.enc == _pt(p).enc

    def Add(self, a: "Point", b: "Point") -> "Point":
        """a + b through the engine's batch addition (the complete unified addition, ge.go:183)."""
        out, st = batch_add(_pt(a).enc, _pt(b).enc)
        if st.any():
            raise ValueError("invalid Ed25519 curve point")
        self.enc = bytes(out[0])
        return self

    def Neg(self, a: "Point") -> "Point":
        """-(x, y) = (-x, y): flip the sign bit of the encoding unless x = 0 (ge.go Neg: X and T negated)."""
        e = _pt(a).enc
        y = int.from_bytes(e, "little") & ((1 << 255) - 1)
        self.enc = e if y in (1, _P - 1) else e[:31] + bytes([e[31] ^ 0x80])
        return self

    def Sub(self, a: "Point", b: "Point") -> "Point":
        return self.Add(a, Point().Neg(b))

    def Pick(self, rand=None) -> "Point":
        """A random element of the prime-order subgroup, k * B.  (The reference's Pick embeds random
        data, point.go:177-233; its outputs are random too and only reproducible with Go's XOF stream.)"""
        return self.Mul(Scalar().Pick(rand), None)

    def EmbedLen(self) -> int:
        """point.go:125-130: 8 bits kept for pseudo-randomness, 8 for the length of the embedded data"""
        return (255 - 8 - 8) // 8

    def Embed(self, data, rand) -> "Point":
        """point.go:132-178.  rand: a kyber.XOF mirror (util/blake2xb.XOF).  Each try draws 32 stream bytes
        (XORKeyStream over zeros), writes the length byte and the data when there is data, and decodes; without data the
        point is multiplied by the cofactor and kept unless it is the identity, with data it is kept only if it already
        lies in the prime-order subgroup.  Decoding and both multiplications are the engine's."""
        dl = min(self.EmbedLen(), len(data)) if data is not None else 0
        while True:
            b = bytearray(rand.XORKeyStream(bytes(32)))
            if data is not None:
                b[0] = dl
                b[1:1 + dl] = bytes(data[:dl])
            out, st = batch_unmarshal(bytes(b))
            if st[0]:
                continue
            enc = bytes(out[0])
            if data is None:
                q, st = batch_mul((8).to_bytes(32, "little"), enc)  # cofactorScalar
                if bytes(q[0]) == _NULL_ENC:
                    continue
                self.enc = bytes(q[0])
                return self
            q, st = batch_mul(ORDER.to_bytes(32, "little"), enc)  # primeOrderScalar, unreduced
            if bytes(q[0]) == _NULL_ENC:
                self.enc = enc
                return self

    def Data(self) -> bytes:
        """point.go:185-193: the data Embed put into the encoding"""
        dl = self.enc[0]
        if dl > self.EmbedLen():
            raise ValueError("invalid embedded data length")
        return self.enc[1:1 + dl]

    def Hash(self, m: bytes, dst: str | bytes) -> "Point":
        """kyber.HashablePoint (hash.go:13; point.go:325-334)."""
        d = dst.encode() if isinstance(dst, str) else bytes(dst)
        self.enc = bytes(batch_hash([bytes(m)], d)[0])
        return self

    def Mul(self, s: Scalar, A: "Point | None") -> "Point":
        a = _sc(s).v
        if A is None:
            self.enc = bytes(batch_mul_base(a)[0])
        else:
            out, st = batch_mul(a, _pt(A).enc, vartime=self.var_time)
            if st[0]:
                raise ValueError("invalid Ed25519 curve point")
            self.enc = bytes(out[0])
        return self

    def String(self) -> str:
        return self.enc.hex()

    __repr__ = String


def _pt(p) -> Point:
    if not isinstance(p, Point):
        raise TypeError("ErrTypeCast: not an edwards25519 point")
    return p


class Curve:
    """kyber.Group (group.go:175-183) for Ed25519."""

    def String(self) -> str:
        return "Ed25519"

    def ScalarLen(self) -> int:
        return SCALAR_LEN

    def Scalar(self) -> Scalar:
        return Scalar()

    def PointLen(self) -> int:
        return POINT_LEN

    def Point(self) -> Point:
        return Point()

    def NewKeyAndSeedWithInput(self, buffer: bytes):
        """curve.go:51-60: clamped, unreduced secret."""
        digest = bytearray(hashlib.sha512(buffer).digest())
        digest[0] &= 0xF8
        digest[31] &= 0x7F
        digest[31] |= 0x40
        return Scalar(bytes(digest[:32])), buffer, bytes(digest[32:])

    def NewKeyAndSeed(self, stream):
        """curve.go:62-69: 32 bytes of the stream (random.Bytes) are the input"""
        return self.NewKeyAndSeedWithInput(stream.XORKeyStream(bytes(32)))

    def NewKey(self, stream) -> Scalar:
        """curve.go:71-76, the key.Generator interface: the clamped secret, stored unreduced"""
        return self.NewKeyAndSeed(stream)[0]


def NewSuite() -> Curve:
    return Curve()
