"""The labelled cases of the share/vss engine calls, shared by the host-harness tests and the GPU tests: deterministic
inputs and, computed once per process, what tests/_vss_oracle.py says about them.  Batches are cut from the END of a pool
(so every batch size sees the planted rejects in its last places) or from its front."""
import functools
import hashlib

import numpy as np

from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _oracle_c as OC
from tests import _vss_oracle as VO

L = O.L
# a deal's marshalled length at threshold t: SessionID 34, SecShare 38, T 2, t commitments of 34 bytes each
# (tests/test_vss_protobuf.py holds the encoder to these)
DEAL_LEN = {2: 142, 17: 652}
# plaintext lengths: the block edges of CTR and GHASH, and a real deal's at t = 2 and t = 17
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, DEAL_LEN[2], DEAL_LEN[17])
# message lengths of a signature: the same, and the edges of SHA-512's second and third block behind R || A
SIGN_LENGTHS = LENGTHS + (46, 111, 112, 175, 176, 177)
SIZES = (1, 63, 64, 65, 127, 128, 129)
POOL = 140


def scalars(tag: bytes, n: int, top: int = 0x0F) -> np.ndarray:
    """n x 32 bytes below 2^252 (top = 0x0F), below 2^255 (0x7F) or any (0xFF)"""
    s = np.frombuffer(hashlib.shake_256(tag).digest(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    s[:, 31] &= top
    return s


def msgs(tag: bytes, n: int, lengths=LENGTHS):
    return [hashlib.shake_256(tag + b" %d" % i).digest(lengths[i % len(lengths)]) for i in range(n)]


# ------------------------------------------------------------------------------------------------------ schnorr.Sign
@functools.lru_cache(maxsize=None)
def sign_pool():
    """(k, x, msgs, want): POOL signatures, a signer each.  Nonces and keys below 2^255, mostly unreduced (>= l); the last
    three rows take k = l - 1, x = 2^256 - 1 and k = 7 * 2^253 + 5: every 32 bytes are a scalar here."""
    k, x = scalars(b"vss sign k", POOL, 0x7F), scalars(b"vss sign x", POOL, 0x7F)
    k[-3] = np.frombuffer((L - 1).to_bytes(32, "little"), dtype=np.uint8)
    x[-2] = 0xFF
    k[-1] = np.frombuffer((7 * 2**253 + 5).to_bytes(32, "little"), dtype=np.uint8)
    m = msgs(b"vss sign msg", POOL, SIGN_LENGTHS)
    want = [VO.schnorr_sign(bytes(k[i]), bytes(x[i]), m[i]) for i in range(POOL)]
    return k, x, m, want


# ------------------------------------------------------------------------------------------------ EncryptedDeal / open
SPECIAL = {POOL - 1: DC.UNDECODABLE, POOL - 30: DC.IDENTITY, POOL - 61: DC.ORDER8, POOL - 64: DC.UNDECODABLE, POOL - 90: DC.NONCANONICAL,
           POOL - 129: DC.UNDECODABLE, 2: DC.UNDECODABLE}


def seal_expected(dh, k, priv, pub, vpubs, ctx, m):
    """VO.seal for a batch, its point multiplications by the oracle's C restatement; None where the key does not decode"""
    keys = OC.ed_mul_base(dh, threads=4)
    pre, st = OC.ed_mul(dh, vpubs, threads=4)
    out = []
    for i in range(len(m)):
        if st[i]:
            out.append(None)
            continue
        c = bytes(ctx[i]) if len(ctx) > 1 else bytes(ctx[0])
        sig = VO.schnorr_sign(bytes(k[i]), priv, bytes(keys[i]), pub)
        out.append((bytes(keys[i]), sig, VO.gcm_seal_aad(VO.aead_key(bytes(pre[i]), c), VO.ZERO_NONCE, m[i], c)))
    return out


@functools.lru_cache(maxsize=None)
def seal_pool(per_element_ctx: bool):
    """(dh, k, priv, pub, vpriv, vpubs, ctx, msgs, want): POOL verifiers of one dealer; keys that are the identity, of
    order 8, written non-canonically or no point at all are planted so that a batch of any size cut from the end has
    an undecodable key in its last place, and the larger ones in the middle and in first place."""
    dh, k = scalars(b"vss seal dh", POOL), scalars(b"vss seal k", POOL)
    vpriv = scalars(b"vss seal x", POOL)
    vpubs = OC.ed_mul_base(vpriv, threads=4)
    for i, p in SPECIAL.items():
        vpubs[i] = np.frombuffer(p, dtype=np.uint8)
    priv = bytes(scalars(b"vss dealer", 1)[0])
    pub = O.mul_base(priv)
    ctx = scalars(b"vss ctx", POOL if per_element_ctx else 1, 0xFF)
    m = msgs(b"vss seal msg", POOL)
    want = seal_expected(dh, k, priv, pub, vpubs, ctx, m)
    assert want[0] == VO.seal(bytes(dh[0]), bytes(k[0]), priv, pub, bytes(vpubs[0]), bytes(ctx[0]), m[0])
    assert [i for i, w in enumerate(want) if w is None] == sorted(i for i, p in SPECIAL.items() if p == DC.UNDECODABLE)
    return dh, k, priv, pub, vpriv, vpubs, ctx, m, want


def open_cases(priv: bytes, context: bytes, want_ok):
    """(dhkey, cipher, label) rows for one receiver under one context, made from sealed elements (dhkey, sig, cipher):
    untouched; a flipped tag bit; a flipped cipher bit; 15 bytes; a key that does not decode; a key that is another
    point.  A flipped context bit is the caller's (it changes the context, not the row)."""
    rows = []
    for j, (key, _, cipher) in enumerate(want_ok):
        rows.append((key, cipher, "good"))
        b = bytearray(cipher)
        b[-1 - (j % 16)] ^= 1 << (j % 8)
        rows.append((key, bytes(b), "tag bit"))
        if len(cipher) > 16:
            b = bytearray(cipher)
            b[(7 * j) % (len(cipher) - 16)] ^= 0x80 >> (j % 8)
            rows.append((key, bytes(b), "cipher bit"))
        rows.append((key, cipher[:15], "short"))
        rows.append((DC.UNDECODABLE, cipher, "undecodable key"))
        rows.append((O.mul_base(bytes([j + 1]) + bytes(31)), cipher, "another key"))
    return rows


# ------------------------------------------------------------------------------------------------- Rabin's share check
def _pedersen_commits(fc, gc, H: bytes):
    """C_j = f_j B + g_j H (rabin/vss.go:160-180: F + G with G = g.Commit(H))"""
    h = O.decode(H)
    return [O.encode(O.add(O.mul_int(a, O.B), O.mul_int(b, h))) for a, b in zip(fc, gc)]


def le(x: int) -> bytes:
    return (x % 2**256).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def check2_table(per_poly_h: bool):
    """(poly, idx, f, g, m, t, commits, H, want_ok, want_status, labels): ONE call's arguments at threshold t = 4 over
    m = 12 polynomials, with every labelled share row at several indices; polynomial 9 is named by no check.
    per_poly_h False: one subgroup point H serves all, and a commitment that does not decode is planted in the first slot
    of the first polynomial, a middle slot of polynomial 6 and the last slot of the last polynomial.
    per_poly_h True: H differs per polynomial -- it does not decode for the first, polynomial 6 and the last; it is the
    identity, a point with an order-8 component, the identity written non-canonically, a subgroup point for others --
    and polynomial 4 has a commitment that does not decode."""
    m, t = 12, 4
    hs = O.mul_base(le(DC.scalar(b"vss H")))
    torsion = O.encode(O.add(O.decode(hs), O.decode(DC.ORDER8)))
    Hs = [DC.UNDECODABLE, DC.IDENTITY, torsion, DC.NONCANONICAL, hs, hs, DC.UNDECODABLE, torsion, hs, hs, hs, DC.UNDECODABLE] if per_poly_h else [hs]
    bad_slots = {4: 2} if per_poly_h else {0: 0, 6: 1, m - 1: t - 1}
    commits, fcs, gcs = [], [], []
    for k in range(m):
        fc = [DC.scalar(b"vss f %d %d" % (k, j)) for j in range(t)]
        gc = [DC.scalar(b"vss g %d %d" % (k, j)) for j in range(t)]
        H = Hs[k] if per_poly_h else hs
        c = _pedersen_commits(fc, gc, H if O.decode(H) is not None else hs)
        if k in bad_slots:
            c[bad_slots[k]] = DC.UNDECODABLE
        commits += c
        fcs.append(fc)
        gcs.append(gc)
    rows = []
    for k in [k for k in range(m) if k != 9]:
        for idx in (0, 1, 255, 2**31, 2**32 - 1):
            fi, gi = DC.eval_scalar(fcs[k], idx), DC.eval_scalar(gcs[k], idx)
            rows += [(k, idx, le(fi), le(gi), "right"), (k, idx, le(fi + 1), le(gi), "forged f"), (k, idx, le(fi), le(gi + 1), "forged g"),
                     (k, idx, le(fi + L), le(gi + L), "both + l"), (k, idx, le(fi), bytes([0xFF]) * 32, "g = 2^256 - 1"),
                     (k, idx, le(fi), le(gi + 2**255), "g + 2^255")]
    poly = np.array([r[0] for r in rows], dtype=np.uint32)
    idx = np.array([r[1] for r in rows], dtype=np.uint32)
    f, g = b"".join(r[2] for r in rows), b"".join(r[3] for r in rows)
    want_ok, bad = [], set()
    for k, i, fs, gs, _ in rows:
        v = VO.deal_check2(fs, gs, commits[k * t:(k + 1) * t], Hs[k] if per_poly_h else hs, i)
        if v is None:
            bad.add(k)
        want_ok.append(v or 0)
    status = [1 if k in bad else 0 for k in range(m)]
    return poly, idx, f, g, m, t, b"".join(commits), b"".join(Hs), want_ok, status, [r[4] for r in rows]


def check2_threshold(t: int, per_poly_h: bool = False):
    """one polynomial at threshold t with the right shares, a forged f and a forged g at three indices"""
    hs = O.mul_base(le(DC.scalar(b"vss H t")))
    fc = [DC.scalar(b"vss tf %d %d" % (t, j)) for j in range(t)]
    gc = [DC.scalar(b"vss tg %d %d" % (t, j)) for j in range(t)]
    commits = _pedersen_commits(fc, gc, hs)
    rows = []
    for idx in (0, 6, 2**32 - 1):
        fi, gi = DC.eval_scalar(fc, idx), DC.eval_scalar(gc, idx)
        rows += [(idx, le(fi), le(gi)), (idx, le(fi + 1), le(gi)), (idx, le(fi), le(gi + 1))]
    want = [VO.deal_check2(fs, gs, commits, hs, i) for i, fs, gs in rows]
    return rows, b"".join(commits), hs, want
