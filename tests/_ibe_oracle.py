"""encrypt/ibe (ibe.go:51-281) end to end on the Python oracle (test infrastructure): EncryptCCAonG1/G2 and
DecryptCCAonG1/G2 with the suite hash SHA-256 and kilic's GT bytes, on top of oracle/bls12381.py and the IBE helpers of
tests/test_oracle_bls12381.py.  Sigma is an argument, as in the engine's C ABI."""
import hashlib

from oracle import bls12381 as O
from tests.test_oracle_bls12381 import _ibe_decrypt, _ibe_h3

TAGS = {"H2": "IBE-H2", "H3": "IBE-H3", "H4": "IBE-H4"}
DOMAIN_G1 = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"
DOMAIN_G2 = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"


def _xor(a: bytes, b: bytes) -> bytes:
    return bytes(x ^ y for x, y in zip(a, b))


def h3(sigma: bytes, msg: bytes) -> int:
    return _ibe_h3(sigma, msg, TAGS)


def h2(gt_bytes: bytes, length: int) -> bytes:
    return hashlib.sha256(b"IBE-H2" + gt_bytes).digest()[:length]


def h4(sigma: bytes, length: int) -> bytes:
    return hashlib.sha256(b"IBE-H4" + sigma).digest()[:length]


def gid(on_g2: bool, master: bytes, ident: bytes, dst: bytes = None):
    """Gid = e(master, H(ID)) on G1 (ID hashed to G2), e(H(ID), master) on G2 (ID hashed to G1), as an Fp12 element"""
    if on_g2:
        return O.pair(O.hash_to_g1(ident, dst or DOMAIN_G1), O.g2_decompress(master))
    return O.pair(O.g1_decompress(master), O.hash_to_g2(ident, dst or DOMAIN_G2))


def encrypt(on_g2: bool, master: bytes, ident: bytes, msg: bytes, sigma: bytes, dst: bytes = None, g=None):
    """(U, V, W) of EncryptCCAonG1 / EncryptCCAonG2 (ibe.go:51-98, 137-185); g: a precomputed Gid"""
    assert len(msg) <= 32 and len(sigma) == len(msg)
    g = gid(on_g2, master, ident, dst) if g is None else g
    r = h3(sigma, msg)
    U = O.g2_compress(O.g2_mul(r, O.G2_GEN)) if on_g2 else O.g1_compress(O.g1_mul(r, O.G1_GEN))
    V = _xor(sigma, h2(O.gt_to_bytes(O.f12_pow(g, r)), len(msg)))
    W = _xor(msg, h4(sigma, len(msg)))
    return U, V, W


def decrypt(on_g2: bool, private: bytes, U: bytes, V: bytes, W: bytes):
    """DecryptCCAonG1 / DecryptCCAonG2 (ibe.go:100-135, 187-232): the message, or ValueError where the reference errs"""
    if len(W) > 32 or len(V) != len(W):
        raise ValueError("ciphertext too long / XorSigma of invalid length")
    gt = O.pair_bytes(private, U) if on_g2 else O.pair_bytes(U, private)
    sigma, msg = _ibe_decrypt(gt, V, W, TAGS)
    r = h3(sigma, msg)
    rP = O.g2_compress(O.g2_mul(r, O.G2_GEN)) if on_g2 else O.g1_compress(O.g1_mul(r, O.G1_GEN))
    if rP != U:
        raise ValueError("invalid proof: rP check failed")
    return msg


def keys(on_g2: bool, s: int, ident: bytes, dst: bytes = None):
    """(master, private) for master secret s: master = s Base, private = s H(ID) (a drand beacon signature)"""
    if on_g2:
        return O.g2_compress(O.g2_mul(s, O.G2_GEN)), O.g1_compress(O.g1_mul(s, O.hash_to_g1(ident, dst or DOMAIN_G1)))
    return O.g1_compress(O.g1_mul(s, O.G1_GEN)), O.g2_compress(O.g2_mul(s, O.hash_to_g2(ident, dst or DOMAIN_G2)))
