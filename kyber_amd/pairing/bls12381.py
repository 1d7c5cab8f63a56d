"""Host-side mirror of the reference's ``pairing/bls12381`` suites for the hot path
(pairing.Suite, pairing/pairing.go:8-20; kilic adapter kilic/{g1,g2,gt,suite}.go), backed by the
HIP engine through the C ABI.  No curve or field arithmetic happens in Python.

Wire formats are the adapters' MarshalBinary encodings: scalars 32-byte big-endian (mod.Int),
G1 48-byte / G2 96-byte ZCash compressed, GT 576 bytes.

Batch functions accept host data (bytes / numpy uint8) or device-resident ``torch.uint8`` CUDA
tensors; device inputs are processed on the current stream and results stay on the device.
"""
import secrets

import numpy as np

from .._buf import _is_torch, dst_arg, space_of
from ._engine import F_SCALAR_BITS, F_TRUSTED, F_TRUSTED_ALL, F_UNCOMPRESSED, F_UNCOMPRESSED_OUT, Engine, pack_fixed  # noqa: F401 (re-exported flags)

ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # kilic/scalar.go:11-12
G1_LEN, G2_LEN, GT_LEN, SCALAR_LEN = 48, 96, 576, 32
G1_BASE = bytes.fromhex(
    "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G2_BASE = bytes.fromhex(
    "93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
G1_NULL = bytes([0xC0]) + bytes(47)
G2_NULL = bytes([0xC0]) + bytes(95)



def _neg(group: int, enc: bytes) -> bytes:
    """-P on the ZCash compressed encoding: flip the y-sign flag (no point of the r-torsion has y = 0)."""
    if enc[0] & 0x40:  # infinity
        return enc
    return bytes([enc[0] ^ 0x20]) + enc[1:]


ENGINE = Engine("bls12381", "bls12-381", ORDER, G1_LEN, G2_LEN, GT_LEN, G1_BASE, G2_BASE, G1_NULL, G2_NULL, _neg)
g1_batch_mul, g2_batch_mul = ENGINE.g1_batch_mul, ENGINE.g2_batch_mul
g1_commit, g2_commit = ENGINE.g1_commit, ENGINE.g2_commit
batch_pair, batch_validate_pairing = ENGINE.batch_pair, ENGINE.batch_validate_pairing
_mul = ENGINE.mul
g1_msm, g2_msm = ENGINE.g1_msm, ENGINE.g2_msm
gt_batch_mul = ENGINE.gt_batch_mul
g1_batch_add = lambda a, b: ENGINE.add(1, a, b)
g2_batch_add = lambda a, b: ENGINE.add(2, a, b)
g1_batch_unmarshal = lambda pts, flags=0: ENGINE.batch_unmarshal(1, pts, flags)
g2_batch_unmarshal = lambda pts, flags=0: ENGINE.batch_unmarshal(2, pts, flags)
Scalar, G1Elt, G2Elt, GTElt, Suite = ENGINE.make_types()


def NewSuite() -> Suite:
    return Suite()

DOMAIN_G1 = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"  # kilic/g1.go:17
DOMAIN_G2 = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"  # kilic/g2.go:18


def _batch_hash(group: int, msgs, dst: bytes):
    sp = space_of(msgs)
    m, n, ln = sp.msgs(msgs, "batch hash")
    out, st = sp.out((n, G1_LEN if group == 1 else G2_LEN)), sp.status(n)
    sp.call(f"kyb_bls12381_hash_g{group}", n, sp.ptr(m), ln, dst_arg(dst), len(dst), sp.ptr(out), sp.ptr(st))
    return out, st[:n]


def batch_hash_g1(msgs, dst: bytes = DOMAIN_G1):
    """(out, status): G1Elt.Hash for n equal-length messages (kilic/g1.go:161-170, RFC 9380 hash_to_curve)."""
    return _batch_hash(1, msgs, dst)


def batch_hash_g2(msgs, dst: bytes = DOMAIN_G2):
    return _batch_hash(2, msgs, dst)


def batch_verify_g1(pubkeys, msgs, sigs, dst: bytes = DOMAIN_G1, flags: int = 0):
    return _batch_verify(1, pubkeys, msgs, sigs, dst, flags)


def batch_verify_g2(pubkeys, msgs, sigs, dst: bytes = DOMAIN_G2, flags: int = 0):
    """As batch_verify_g1 for the scheme with signatures on G2 and keys on G1 (NewSchemeOnG2, bls.go:48-58)."""
    return _batch_verify(2, pubkeys, msgs, sigs, dst, flags)


def _fixed(sp, x, width: int):
    """(rows, bad lanes) of per-element keys / signatures.  A list on the host is packed element by element, so that an
    (attacker-supplied) element of the wrong length fails alone: its lane is zero bytes and comes back in `bad`."""
    if isinstance(x, (list, tuple)) and not sp.is_device:
        return pack_fixed(x, width)
    return sp.rows(x, width), []


def _fail_lanes(ok, st, bad, keep_status: bool = True):
    """the lanes pack_fixed blanked are invalid: status BAD_POINT unless (keep_status) the native call already said more"""
    for i in bad:
        ok[i] = 0
        if st[i] == 0 or not keep_status:
            st[i] = 1  # KYB_ST_BAD_POINT


def batch_verify_g1_same_key(pubkey, msgs, sigs, dst: bytes = DOMAIN_G1, flags: int = 0):
    """(ok, status): N x bls.Verify under ONE public key (sign/bls/bls.go:82-96 in a loop with the same X: a drand
    chain, sign/tbls/tbls.go:100-107) -- both Miller loops from line tables (kyb_bls12381_verify_g1_same_key).
    pubkey: 96 bytes (192 with F_UNCOMPRESSED) or a CUDA tensor of that size when msgs / sigs are CUDA tensors."""
    wk, wsig = (192, 96) if flags & F_UNCOMPRESSED else (96, 48)
    sp = space_of(msgs)
    m, n, ln = sp.msgs(msgs, "batch_verify_same_key")
    s, bad_s = _fixed(sp, sigs, wsig)
    klen = pubkey.numel() if _is_torch(pubkey) else len(bytes(pubkey))
    if s.shape[0] != n or (sp.is_device and klen != wk):
        raise ValueError("batch_verify_same_key: " + (f"key of {klen} bytes, " if sp.is_device else "")
                         + f"{n} messages, {s.shape[0]} signatures")
    ok, st = sp.status(n), sp.status(n)
    if klen != wk:  # (host) a key of the wrong length fails every element, as UnmarshalBinary would fail the one key
        st[:] = 1
        return ok[:n], st[:n]
    k = sp.rows(pubkey, wk)
    sp.call("kyb_bls12381_verify_g1_same_key", n, sp.ptr(k), sp.ptr(m), ln, dst_arg(dst), len(dst), sp.ptr(s), sp.ptr(ok),
            sp.ptr(st), flags)
    _fail_lanes(ok, st, bad_s)  # precedence as the header documents it: the key's verdict first, then the signature's
    return ok[:n], st[:n]


def _rows(x, width: int, what: str):
    """(n, width) uint8 array of a list of equal-length byte strings or an array; width None: any equal width"""
    if isinstance(x, (list, tuple)):
        w = width if width is not None else (len(x[0]) if x else 0)
        if any(len(bytes(e)) != w for e in x):
            raise ValueError(f"{what}: every element must be {w} bytes")
        a = np.frombuffer(b"".join(bytes(e) for e in x), dtype=np.uint8).reshape(len(x), w)
    else:
        a = np.asarray(x, dtype=np.uint8)
        if a.ndim != 2 or (width is not None and a.shape[1] != width):
            raise ValueError(f"{what}: expected an (n, {width if width is not None else 'L'}) uint8 array, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _sigmas(n: int, ln: int) -> np.ndarray:
    return np.frombuffer(secrets.token_bytes(n * ln), dtype=np.uint8).reshape(n, ln).copy()


def _ibe_plain_host(sp, name, msz, master, ident, msgs, sigmas):
    """(msgs, sigmas, master, ident, ident length) of host buffers, each refused with a message of its own"""
    m = _rows(msgs, None, name + " msgs")
    n, ln = m.shape
    if ln > 32:
        raise ValueError(f"{name}: plaintext of {ln} bytes is too long for SHA-256 (at most 32)")
    s = _rows(sigmas, ln, name + " sigmas") if sigmas is not None else _sigmas(n, ln)
    if s.shape[0] != n:
        raise ValueError(f"{name}: {n} messages, {s.shape[0]} sigmas")
    mb, ib = bytes(master), bytes(ident)
    if len(mb) != msz:
        raise ValueError(f"{name}: master key of {len(mb)} bytes (want {msz})")
    return m, s, sp.rows(mb, msz), sp.rows(ib or b"\0", 1), len(ib)


def _ibe_plain_cuda(sp, name, msz, master, ident, msgs, sigmas):
    """the same of device tensors; a master key, an identity or fresh sigmas that are host bytes are uploaded"""
    m, n, ln = sp.msgs(msgs)
    s = (sigmas if sigmas is not None else sp.rows(_sigmas(n, ln), ln or 1).view(n, ln)).contiguous()
    mk = sp.rows(master, 1)
    id_len = ident.numel() if _is_torch(ident) else len(bytes(ident))
    idt = sp.rows(ident if _is_torch(ident) else bytes(ident) or b"\0", 1)
    if mk.numel() != msz or tuple(s.shape) != (n, ln) or ln > 32:
        raise ValueError(f"{name}: master of {mk.numel()} bytes (want {msz}), sigmas {tuple(s.shape)}, msgs {(n, ln)} (L <= 32)")
    return m, s, mk, idt, id_len


def _ibe_encrypt(on_g2: bool, master, ident: bytes, msgs, sigmas, dst: bytes, flags: int):
    name = "kyb_bls12381_ibe_encrypt_" + ("g2" if on_g2 else "g1")
    msz = (192 if on_g2 else 96) if flags & F_UNCOMPRESSED else (96 if on_g2 else 48)
    usz = (192 if on_g2 else 96) if flags & F_UNCOMPRESSED_OUT else (96 if on_g2 else 48)
    if len(dst) > 255:
        raise ValueError(f"{name}: DST of {len(dst)} bytes (at most 255, as expand_message_xmd takes it)")
    sp = space_of(msgs)
    m, s, mk, idt, id_len = (_ibe_plain_cuda if sp.is_device else _ibe_plain_host)(sp, name, msz, master, ident, msgs, sigmas)
    n, ln = m.shape
    u, v, w, st = sp.out((n, usz)), sp.out((n, ln)), sp.out((n, ln)), sp.status(n)
    sp.call(name, n, sp.ptr(mk), sp.ptr(idt), id_len, dst_arg(dst), len(dst), sp.ptr(s), sp.ptr(m), ln, sp.ptr(u), sp.ptr(v),
            sp.ptr(w), sp.ptr(st), flags)
    return u, v, w, st[:n]


def _ibe_cipher_host(sp, name, ksz, usz, privates, us, vs, ws):
    """(keys, key stride, U, V, W) of host buffers, each refused with a message of its own"""
    u = _rows(us, usz, name + " U")
    n = u.shape[0]
    w = _rows(ws, None, name + " W") if n else np.zeros((0, 0), dtype=np.uint8)
    ln = w.shape[1]
    v = _rows(vs, ln, name + " V") if n else w
    if ln > 32 or v.shape[0] != n or w.shape[0] != n:
        raise ValueError(f"{name}: {n} U, {v.shape[0]} V, {w.shape[0]} W of {ln} bytes (at most 32)")
    if isinstance(privates, (bytes, bytearray)) or (isinstance(privates, np.ndarray) and privates.ndim == 1):
        k, stride = np.frombuffer(bytes(privates), dtype=np.uint8), 0
        if k.size != ksz:
            raise ValueError(f"{name}: private key of {k.size} bytes (want {ksz})")
    else:
        k, stride = _rows(privates, ksz, name + " private keys"), ksz
        if k.shape[0] != n:
            raise ValueError(f"{name}: {k.shape[0]} private keys for {n} ciphertexts")
    return np.ascontiguousarray(k), stride, u, v, w


def _ibe_cipher_cuda(sp, name, ksz, usz, privates, us, vs, ws):
    """the same of device tensors; a private key that is host bytes is uploaded"""
    u = sp.rows(us, usz)
    n = u.shape[0]
    v, w = (x.contiguous().view(n, -1 if n else x.shape[-1]) for x in (vs, ws))  # (no width to infer from 0 rows)
    ln = w.shape[1]
    k = sp.rows(privates, 1)
    stride = 0 if k.numel() == ksz else ksz
    if v.shape[1] != ln or ln > 32 or (stride and k.numel() != n * ksz):
        raise ValueError(f"{name}: V / W of {v.shape[1]} / {ln} bytes (equal, at most 32), keys of {k.numel()} bytes for {n} ciphertexts")
    return k, stride, u, v, w


def _ibe_decrypt(on_g2: bool, privates, us, vs, ws, flags: int):
    name = "kyb_bls12381_ibe_decrypt_" + ("g2" if on_g2 else "g1")
    ksz = (96 if on_g2 else 192) if flags & F_UNCOMPRESSED else (48 if on_g2 else 96)
    usz = (192 if on_g2 else 96) if flags & F_UNCOMPRESSED else (96 if on_g2 else 48)
    sp = space_of(us)
    k, stride, u, v, w = (_ibe_cipher_cuda if sp.is_device else _ibe_cipher_host)(sp, name, ksz, usz, privates, us, vs, ws)
    n, ln = w.shape
    out, st = sp.out((n, ln)), sp.status(n)
    sp.call(name, n, sp.ptr(k), stride, sp.ptr(u), sp.ptr(v), sp.ptr(w), ln, sp.ptr(out), sp.ptr(st), flags)
    return out, st[:n]


def batch_ibe_encrypt_g1(master, ident: bytes, msgs, sigmas=None, dst: bytes = DOMAIN_G2, flags: int = 0):
    """(U, V, W, status): EncryptCCAonG1 (encrypt/ibe/ibe.go:51-98) of n equal-length messages (at most 32 bytes) to ONE
    identity under ONE master key on G1; the identity hashes to G2 under `dst`.  sigmas: the per-message randomness
    (n x L bytes), drawn with `secrets` when None.  kyb_bls12381_ibe_encrypt_g1 (_dev for CUDA tensors)."""
    return _ibe_encrypt(False, master, ident, msgs, sigmas, dst, flags)


def batch_ibe_encrypt_g2(master, ident: bytes, msgs, sigmas=None, dst: bytes = DOMAIN_G1, flags: int = 0):
    """EncryptCCAonG2 (ibe.go:137-185): master key and U on G2, the identity hashed to G1 (drand quicknet / tlock)."""
    return _ibe_encrypt(True, master, ident, msgs, sigmas, dst, flags)


def batch_ibe_decrypt_g1(privates, U, V, W, flags: int = 0):
    """(msgs, status): DecryptCCAonG1 (ibe.go:100-135) of n ciphertexts with equal-length V and W.  privates: ONE G2 key
    (bytes: every ciphertext of a tlock round under its beacon) or one per ciphertext.  status 3 = rP != U
    (ST_IBE_CHECK), 1 / 2 = a key or U that does not unmarshal; the message is zero bytes there."""
    return _ibe_decrypt(False, privates, U, V, W, flags)


def batch_ibe_decrypt_g2(privates, U, V, W, flags: int = 0):
    """DecryptCCAonG2 (ibe.go:187-232): private keys on G1, U on G2."""
    return _ibe_decrypt(True, privates, U, V, W, flags)


def batch_verify_g1_same_msg(pubkeys, msg, sigs, dst: bytes = DOMAIN_G1, flags: int = 0):
    """(ok, status): ok[i] = bls.Verify(pubkeys[i], msg, sigs[i]) for ONE message -- the verification loop of
    tbls.Recover (sign/tbls/tbls.go:118-131: every partial signature signs the same msg under its own public share):
    H(msg) is hashed once per call (kyb_bls12381_verify_g1_same_msg), the rest is batch_verify_g1.
    msg: bytes, or a 1-D CUDA uint8 tensor when pubkeys / sigs are CUDA tensors."""
    wk, wsig = (192, 96) if flags & F_UNCOMPRESSED else (96, 48)
    sp = space_of(pubkeys)
    p, bad_p = _fixed(sp, pubkeys, wk)
    s, bad_s = _fixed(sp, sigs, wsig)
    n = p.shape[0]
    if s.shape[0] != n:
        raise ValueError(f"batch_verify_same_msg: {n} public keys, {s.shape[0]} signatures")
    ln = int(msg.numel()) if _is_torch(msg) else len(bytes(msg))
    if ln:
        m = sp.rows(msg, 1)
    else:  # an empty message: a dummy byte on the device, NULL on the host
        m = sp.out(1).zero_() if sp.is_device else None
    ok, st = sp.status(n), sp.status(n)
    sp.call("kyb_bls12381_verify_g1_same_msg", n, sp.ptr(p), sp.ptr(m), ln, dst_arg(dst), len(dst), sp.ptr(s), sp.ptr(ok),
            sp.ptr(st), flags)
    _fail_lanes(ok, st, bad_p + bad_s)  # a wrong-length key / signature fails alone
    return ok[:n], st[:n]


def _batch_verify(sig_group: int, pubkeys, msgs, sigs, dst: bytes, flags: int):
    """(ok, status): N x bls.Verify (sign/bls/bls.go:82-96; signatures on G1, keys on G2) fused in ONE kernel:
    hash_to_curve, both unmarshal checks, two Miller loops sharing their squarings and one final exponentiation
    per lane.  msgs: (n, msg_len) uint8 array / CUDA tensor or list of equal-length bytes.  flags: F_TRUSTED(0) for
    public keys validated before (the usual case: keys are unmarshalled once), F_TRUSTED(1) for the signatures,
    F_UNCOMPRESSED for uncompressed-affine keys and signatures."""
    wk, wsig = (96, 48) if sig_group == 1 else (48, 96)
    if flags & F_UNCOMPRESSED:
        wk, wsig = 2 * wk, 2 * wsig
    sp = space_of(msgs)
    m, n, ln = sp.msgs(msgs, "batch_verify")
    p, bad_p = _fixed(sp, pubkeys, wk)
    s, bad_s = _fixed(sp, sigs, wsig)
    if p.shape[0] != n or s.shape[0] != n:
        raise ValueError(f"batch_verify: {n} messages, {p.shape[0]} public keys, {s.shape[0]} signatures")
    ok, st = sp.status(n), sp.status(n)
    sp.call(f"kyb_bls12381_verify_g{sig_group}", n, sp.ptr(p), sp.ptr(m), ln, dst_arg(dst), len(dst), sp.ptr(s), sp.ptr(ok),
            sp.ptr(st), flags)
    _fail_lanes(ok, st, bad_p + bad_s, keep_status=False)
    return ok[:n], st[:n]
