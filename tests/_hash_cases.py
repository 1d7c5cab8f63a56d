"""Case tables for the hash-to-curve length tests (tests/test_gpu_hash_lengths.py, the host-harness twin in
tests/test_host_harness_bls12381.py); tests/test_hash_cases.py checks the coverage they claim, without a GPU.

expand_message_xmd (RFC 9380 section 5.3.1) runs two kinds of hash.  b_0 absorbs Z_pad || msg || l_i_b_str(2) || 0 ||
DST || len(DST), so it finishes at position (zpad + msg_len + dst_len + 4) mod block; every b_i absorbs a digest, a
counter, DST and len(DST), so it finishes at (digest + dst_len + 2) mod block -- only the DST length moves it.  A
Merkle-Damgard finish is one block up to position threshold - 1 and spills into an extra block from `threshold` on
(SHA-256: 56 of 64, SHA-512: 112 of 128); Keccak's pad10*1 folds into ONE byte at position block - 1 (135 of 136).  The
positions a table has to reach are therefore

    required = {min(block - 10, threshold - 2) .. block - 1, 0, 1}

which is {54 .. 63, 0, 1} for SHA-256, {110 .. 127, 0, 1} for SHA-512 and {126 .. 135, 0, 1} for Keccak-256: two
positions before the switch, every position after it up to the end of the block, and the first two of the next block.
"""
import hashlib
from collections import namedtuple

Xmd = namedtuple("Xmd", "block zpad digest threshold")
SHA256 = Xmd(block=64, zpad=64, digest=32, threshold=56)        # BLS12-381 (bls12381_h2c.cuh), sha256.cuh
KECCAK256 = Xmd(block=136, zpad=136, digest=32, threshold=135)  # bn254 (bn_suite.inc), keccak256.cuh
SHA512 = Xmd(block=128, zpad=128, digest=64, threshold=112)     # Ed25519 (ed25519_h2c.cuh), sha512.cuh

DST_LENS = (0, 1, 21, 22, 43, 50, 85, 86, 254, 255)
DST_LENS_NONEMPTY = DST_LENS[1:]  # Ed25519 refuses an empty DST, as (*point).Hash does


def required_positions(block: int, threshold: int | None = None) -> frozenset:
    threshold = block - 8 if threshold is None else threshold
    return frozenset(range(min(block - 10, threshold - 2), block)) | {0, 1}


def b0_position(msg_len: int, dst_len: int, block: int, zpad: int) -> int:
    return (zpad + msg_len + 2 + 1 + dst_len + 1) % block


def bi_position(dst_len: int, block: int, digest: int = 32) -> int:
    return (digest + 1 + dst_len + 1) % block


# message-length classes: empty, one byte, small (2 .. block - 1), one block (block .. 2 block - 1), a few blocks
# (from 3 block + 8: 200 bytes for SHA-256), several blocks (from 1000 bytes)
def length_class(msg_len: int, block: int) -> str:
    if msg_len < 2:
        return ("empty", "one byte")[msg_len]
    if msg_len < block:
        return "small"
    if msg_len < 2 * block:
        return "one block"
    return "several blocks" if msg_len >= 1000 else "a few blocks"


def _fit(lo: int, pos: int, dst_len: int, block: int, zpad: int) -> int:
    """the message length in [lo, lo + block) whose b_0 finishes at `pos` under a DST of dst_len bytes"""
    return lo + (pos - b0_position(lo, dst_len, block, zpad)) % block


def cases(hash_block: int, zpad: int, dst_lens=DST_LENS, digest: int = 32, threshold: int | None = None) -> list:
    """(msg_len, dst_len) pairs, in a fixed order, such that
      * every DST length of dst_lens is used with messages of 0, 1 and 32 bytes;
      * every b_i finish position of required_positions() is reached (by the DST length that gives it), with a message whose
        b_0 finishes at the same position;
      * every b_0 finish position of required_positions() is reached with a message of every length class."""
    block = hash_block
    req = sorted(required_positions(block, threshold), key=lambda p: (p - 2) % block)  # ..., block - 1, 0, 1
    lows = {"small": 2, "one block": block, "a few blocks": 3 * block + 8, "several blocks": 1000}
    out, seen = [], set()

    def add(m, d):
        assert 0 <= d <= 255 and (d in dst_lens or d > 0)
        if (m, d) not in seen:
            seen.add((m, d))
            out.append((m, d))

    def legal(d):  # a DST length congruent to d that the suite takes
        return d + block if d == 0 and 0 not in dst_lens else d

    for d in dst_lens:
        for m in (0, 1, 32):
            add(m, d)
    names = list(lows)
    for k, p in enumerate(req):
        d = legal((p - digest - 2) % block)
        m = _fit(lows[names[k % len(names)]], p, d, block, zpad)
        if names[k % len(names)] == "small" and m >= block:
            m = _fit(block, p, d, block, zpad)
        add(m, d)
    k = 0
    for p in req:
        for m in (0, 1):
            add(m, legal((p - b0_position(m, 0, block, zpad)) % block))
        for name, lo in lows.items():
            while True:
                d = dst_lens[k % len(dst_lens)]
                k += 1
                m = _fit(lo, p, d, block, zpad)
                if name != "small" or m < block:
                    break
            add(m, d)
    return out


def reached(table, xmd: Xmd):
    """({b_0 position: set of length classes}, {b_i positions}) of a table"""
    b0, bi = {}, set()
    for m, d in table:
        b0.setdefault(b0_position(m, d, xmd.block, xmd.zpad), set()).add(length_class(m, xmd.block))
        bi.add(bi_position(d, xmd.block, xmd.digest))
    return b0, bi


SHA256_CASES = cases(SHA256.block, SHA256.zpad, DST_LENS, SHA256.digest, SHA256.threshold)
KECCAK256_CASES = cases(KECCAK256.block, KECCAK256.zpad, DST_LENS, KECCAK256.digest, KECCAK256.threshold)
SHA512_CASES = cases(SHA512.block, SHA512.zpad, DST_LENS_NONEMPTY, SHA512.digest, SHA512.threshold)


def oneshot_lengths(block: int, threshold: int | None = None) -> list:
    """message lengths for a one-shot hash (bn256 pointG1.Hash: SHA-256 of the message, finish at len mod block): every
    required position below one block (0 and 1 among them), within the second block and past 1000 bytes"""
    req = sorted(required_positions(block, threshold))
    big = -(-1000 // block) * block
    return sorted({lo + p for p in req for lo in (0, block, big)})


# bn256 HashG1 is HKDF-SHA-256 (RFC 5869) with the message as the secret and the DST as the salt: the inner hash of the
# extract step absorbs a 64-byte key block and the message (finish at msg_len mod 64), and a salt longer than a block is
# hashed down first (finish at dst_len mod 64).  The SHA-256 table runs through it as it stands; these pairs add the
# positions it leaves out.
SVDW_EXTRA = [(m, (0, 1, 64, 65, 255)[k % 5]) for k, m in enumerate(oneshot_lengths(64))] + \
             [(32 + k, 64 + p if p > 1 else 128 + p) for k, p in enumerate(sorted(required_positions(64)))]
SVDW_CASES = SHA256_CASES + [c for c in SVDW_EXTRA if c not in set(SHA256_CASES)]


def boundary_pairs(table, xmd: Xmd) -> list:
    """six pairs that sit on the boundaries: b_0 at threshold - 1, threshold and 0, b_i at threshold - 1 and threshold
    (two pairs for the latter: a short and the longest message)"""
    t = xmd.threshold
    pick = [next(c for c in table if b0_position(*c, xmd.block, xmd.zpad) == p and c[0] >= 2) for p in (t - 1, t, 0)]
    at = lambda p: [c for c in table if bi_position(c[1], xmd.block, xmd.digest) == p and c not in pick]
    pick += [at(t - 1)[0], at(t)[0], max(at(t), key=lambda c: c[0])]
    assert len(set(pick)) == 6
    return pick


def cover(table, xmd: Xmd) -> list:
    """a small sub-table that still reaches every required position of both hashes and holds an empty message, an empty DST
    (where the suite takes one) and a 255-byte DST: the entries the fused verifications run"""
    req = required_positions(xmd.block, xmd.threshold)
    need = {("b0", p) for p in req} | {("bi", p) for p in req}
    gives = lambda c: {("b0", b0_position(*c, xmd.block, xmd.zpad)), ("bi", bi_position(c[1], xmd.block, xmd.digest))} & need
    pick = []
    while need:
        best = max(table, key=lambda c: len(gives(c)))  # (first of the best: the table's order is fixed)
        assert gives(best)
        pick.append(best)
        need -= gives(best)
    want = [lambda c: c[0] == 0, lambda c: c[1] == 255, lambda c: c[0] >= 1000]
    if any(c[1] == 0 for c in table):
        want.append(lambda c: c[1] == 0 and c[0] > 1)
    for w in want:
        if not any(w(c) for c in pick):
            pick.append(next(c for c in table if w(c)))
    return pick


def messages(label: bytes, n: int, msg_len: int):
    """(n, msg_len) uint8 array from SHAKE-256(label): every byte position of every message carries its own value"""
    import numpy as np

    raw = hashlib.shake_256(label + b"/%d/%d" % (n, msg_len)).digest(n * msg_len)
    return np.frombuffer(raw, dtype=np.uint8).reshape(n, msg_len).copy()


def dst_bytes(dst_len: int) -> bytes:
    return hashlib.shake_256(b"hash-lengths/dst/%d" % dst_len).digest(dst_len)


# ---------------------------------------------------------------- the oracles, by name (picklable: the GPU tests spread
# them over worker processes that never open the GPU)
def oracle_hash(job):
    """job = (kind, msg, dst) -> the reference's bytes for Hash(msg) under dst"""
    kind, msg, dst = job
    if kind in ("bls_g1", "bls_g2"):
        from oracle import bls12381 as O

        return O.g1_compress(O.hash_to_g1(msg, dst)) if kind == "bls_g1" else O.g2_compress(O.hash_to_g2(msg, dst))
    if kind == "bn254":
        from oracle import bn254 as O

        return O.g1_marshal(O.hash_to_g1(msg, dst))
    if kind in ("bn256_svdw", "bn256"):
        from oracle import bn256 as O

        return O.g1_marshal(O.hash_g1_svdw(msg, dst) if kind == "bn256_svdw" else O.hash_to_g1(msg))
    if kind == "ed25519":
        from oracle import ed25519 as O

        return O.hash_to_curve(msg, dst)
    raise ValueError(kind)


def oracle_sign(job):
    """job = (group, x, msg, dst) -> x * hash_to_curve(msg, dst) on BLS12-381 G1 / G2, compressed: a BLS signature made
    without the engine"""
    from oracle import bls12381 as O

    group, x, msg, dst = job
    if group == 1:
        return O.g1_compress(O.g1_mul(x, O.hash_to_g1(msg, dst)))
    return O.g2_compress(O.g2_mul(x, O.hash_to_g2(msg, dst)))
