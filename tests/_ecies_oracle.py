"""encrypt/ecies (ecies.go) restated in pure Python for the tests: AES-256-GCM from FIPS 197 / SP 800-38D on Python
integers, HKDF-SHA256 (RFC 5869) on hmac / hashlib, the points on oracle/ed25519.py.  The checker of
kyb_ed25519_ecies_seal / _open and of kyber_amd/encrypt/ecies.py, never the thing shipped, written from the reference's
text and the standards without looking at the device code.  tests/golden/aes256gcm.json (OpenSSL's outputs) pins the
AES-GCM here; RFC 5869 test case 3 pins the HKDF.

The reference prints no ECIES bytes and no Go toolchain is at hand, so no transcript of the Go program is pinned."""
import hashlib
import hmac

from oracle import ed25519 as O

ST_OK, ST_BAD_POINT, ST_ECIES_SHORT, ST_ECIES_AUTH = 0, 1, 9, 10


def _sbox():
    s = [0] * 256
    p = q = 1
    while True:
        p = (p ^ (p << 1) ^ (0x1B if p & 0x80 else 0)) & 0xFF
        q ^= q << 1
        q ^= q << 2
        q ^= q << 4
        q &= 0xFF
        if q & 0x80:
            q ^= 0x09
        rot = lambda v, k: ((v << k) | (v >> (8 - k))) & 0xFF
        s[p] = q ^ rot(q, 1) ^ rot(q, 2) ^ rot(q, 3) ^ rot(q, 4) ^ 0x63
        if p == 1:
            break
    s[0] = 0x63
    return s


SBOX = _sbox()


def _xtime(a):
    return ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF


def expand_key(key: bytes):
    """FIPS 197 section 5.2 for Nk = 8: 60 words as 4-byte strings"""
    assert len(key) == 32
    w = [key[4 * i:4 * i + 4] for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = w[i - 1]
        if i % 8 == 0:
            t = bytes(SBOX[b] for b in t[1:] + t[:1])
            t = bytes([t[0] ^ rcon]) + t[1:]
            rcon = _xtime(rcon)
        elif i % 8 == 4:
            t = bytes(SBOX[b] for b in t)
        w.append(bytes(a ^ b for a, b in zip(w[i - 8], t)))
    return w


def encrypt_block(w, block: bytes) -> bytes:
    """FIPS 197 section 5.1, the state as 16 bytes column by column"""
    s = [b ^ k for b, k in zip(block, b"".join(w[0:4]))]
    for r in range(1, 15):
        s = [SBOX[b] for b in s]
        s = [s[(4 * c + 5 * j) % 16] for c in range(4) for j in range(4)]  # ShiftRows: row j from column c + j
        if r < 14:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_xtime(a[j]) ^ _xtime(a[(j + 1) % 4]) ^ a[(j + 1) % 4] ^ a[(j + 2) % 4] ^ a[(j + 3) % 4] for j in range(4)]
            s = m
        s = [b ^ k for b, k in zip(s, b"".join(w[4 * r:4 * r + 4]))]
    return bytes(s)


def _gf_mul(x: int, y: int) -> int:
    """SP 800-38D section 6.3, blocks as big-endian integers"""
    z, v = 0, y
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ (0xE1 << 120 if v & 1 else 0)
    return z


def _ghash(h: int, data: bytes) -> int:
    y = 0
    for i in range(0, len(data), 16):
        y = _gf_mul(y ^ int.from_bytes(data[i:i + 16].ljust(16, b"\0"), "big"), h)
    return y


def _ctr(w, nonce: bytes, data: bytes) -> bytes:
    out = bytearray()
    for i in range(0, len(data), 16):
        ks = encrypt_block(w, nonce + (2 + i // 16).to_bytes(4, "big"))
        out += bytes(a ^ b for a, b in zip(data[i:i + 16], ks))
    return bytes(out)


def _tag(w, nonce: bytes, ct: bytes) -> bytes:
    h = int.from_bytes(encrypt_block(w, bytes(16)), "big")
    y = _ghash(h, ct)
    y = _gf_mul(y ^ (len(ct) * 8), h)  # the length block: no additional data, then the ciphertext's bits
    mask = int.from_bytes(encrypt_block(w, nonce + b"\0\0\0\1"), "big")
    return (y ^ mask).to_bytes(16, "big")


def gcm_seal(key: bytes, nonce: bytes, msg: bytes) -> bytes:
    assert len(nonce) == 12
    w = expand_key(key)
    ct = _ctr(w, nonce, msg)
    return ct + _tag(w, nonce, ct)


def gcm_open(key: bytes, nonce: bytes, sealed: bytes):
    """the plaintext, or None (cipher: message authentication failed)"""
    if len(sealed) < 16:
        return None
    w = expand_key(key)
    ct, tag = sealed[:-16], sealed[-16:]
    if not hmac.compare_digest(_tag(w, nonce, ct), tag):
        return None
    return _ctr(w, nonce, ct)


def hkdf_sha256(secret: bytes, n: int) -> bytes:
    """RFC 5869 with no salt (HashLen zero bytes) and no info"""
    prk = hmac.new(bytes(32), secret, hashlib.sha256).digest()
    out, t, i = b"", b"", 1
    while len(out) < n:
        t = hmac.new(prk, t + bytes([i]), hashlib.sha256).digest()
        out += t
        i += 1
    return out[:n]


def derive(dh: bytes):
    """ecies.go:115-127: key (32 bytes) and nonce (12)"""
    okm = hkdf_sha256(dh, 44)
    return okm[:32], okm[32:]


def encrypt(r: bytes, pub: bytes, msg: bytes):
    """ecies.go:23-69 with the ephemeral scalar given: R || Seal, or None when pub does not decode"""
    dh = O.mul(r, pub)
    if dh is None:
        return None
    key, nonce = derive(dh)
    return O.mul_base(r) + gcm_seal(key, nonce, msg)


def decrypt(priv: bytes, ctx: bytes):
    """ecies.go:77-112: (plaintext, 0) or (None, status)"""
    if len(ctx) < 48:
        return None, ST_ECIES_SHORT
    dh = O.mul(priv, ctx[:32])
    if dh is None:
        return None, ST_BAD_POINT
    key, nonce = derive(dh)
    msg = gcm_open(key, nonce, ctx[32:])
    return (msg, ST_OK) if msg is not None else (None, ST_ECIES_AUTH)


# The plaintext lengths of every ECIES test: the block edges of CTR and GHASH and the HKDF / tag paths
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 255, 256, 257, 1000)
