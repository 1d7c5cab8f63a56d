"""BLAKE2Xb extendable-output function (host plumbing): ``blake2xb.New(seed)`` of the reference
(xof/blake2xb/blake.go:19-41), the XOF of the Ed25519 suite (group/edwards25519/suite.go:31) and so the stream behind
every Fiat-Shamir challenge of proof/dleq and share/pvss (``Scalar.Pick(suite.XOF(cb))``).  hashlib's blake2b refuses
the depth = 0 parameter block BLAKE2X needs for its output nodes, hence this parameterised BLAKE2b, the 64-bit sibling
of util/blake2xs.py.  The device restatement for 32-byte seeds is kyber_amd/csrc/blake2xb.cuh.

Pinned by two outputs the reference prints: examples/dh_test.go:19-48 (unkeyed, two picks of three draws each) and
proof/proof_test.go:89-117 (keyed with "example"); tests/test_blake2xb.py checks both.
"""
from __future__ import annotations

import hashlib
import struct

IV = [0x6A09E667F3BCC908, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1,
      0x510E527FADE682D1, 0x9B05688C2B3E6C1F, 0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179]
SIGMA = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
         [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4], [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
         [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13], [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
         [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11], [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
         [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5], [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0]]
M64 = (1 << 64) - 1
SIZE, BLOCK = 64, 128
UNKNOWN = 0xFFFFFFFF  # blake2b.OutputLengthUnknown
ORDER = 2**252 + 27742317777372353535851937790883648493


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def compress(h, block, t, last):
    """one BLAKE2b compression: h (8 words), a 128-byte block, t bytes hashed so far, last block flag"""
    m = struct.unpack("<16Q", block)
    v = list(h) + IV[:]
    v[12] ^= t & M64
    v[13] ^= (t >> 64) & M64
    if last:
        v[14] ^= M64

    def G(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & M64
        v[d] = _rotr(v[d] ^ v[a], 32)
        v[c] = (v[c] + v[d]) & M64
        v[b] = _rotr(v[b] ^ v[c], 24)
        v[a] = (v[a] + v[b] + y) & M64
        v[d] = _rotr(v[d] ^ v[a], 16)
        v[c] = (v[c] + v[d]) & M64
        v[b] = _rotr(v[b] ^ v[c], 63)

    for r in range(12):
        s = SIGMA[r % 10]
        G(0, 4, 8, 12, m[s[0]], m[s[1]])
        G(1, 5, 9, 13, m[s[2]], m[s[3]])
        G(2, 6, 10, 14, m[s[4]], m[s[5]])
        G(3, 7, 11, 15, m[s[6]], m[s[7]])
        G(0, 5, 10, 15, m[s[8]], m[s[9]])
        G(1, 6, 11, 12, m[s[10]], m[s[11]])
        G(2, 7, 8, 13, m[s[12]], m[s[13]])
        G(3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]


def param_block(digest_len, key_len, fanout, depth, leaf_len, node_off, xof_len, node_depth, inner_len) -> bytes:
    """the 64-byte BLAKE2b parameter block with BLAKE2X's xof length in the upper half of the node offset"""
    return struct.pack("<BBBBIIIBB", digest_len, key_len, fanout, depth, leaf_len, node_off, xof_len, node_depth, inner_len) + bytes(46)


def blake2b_param(data: bytes, param: bytes, key: bytes = b"") -> bytes:
    """BLAKE2b of key block || data under a full parameter block; the digest length is param[0]"""
    h = [IV[i] ^ w for i, w in enumerate(struct.unpack("<8Q", param))]
    if key:
        data = key.ljust(BLOCK, b"\0") + data
    blocks = [data[i:i + BLOCK] for i in range(0, len(data), BLOCK)] or [b""]
    t = 0
    for i, b in enumerate(blocks):
        t += len(b)
        h = compress(h, b.ljust(BLOCK, b"\0"), t, i == len(blocks) - 1)
    return struct.pack("<8Q", *h)[:param[0]]


def root_hash(key: bytes, msg: bytes) -> bytes:
    """the root node of blake2b.NewXOF(OutputLengthUnknown, key) after Write(msg).  Its parameter block is one hashlib
    accepts (fanout 1, depth 1; the xof length is the upper half of the 64-bit node offset), so a transcript of any size
    is hashed at hashlib's speed; the output nodes (depth 0) are not."""
    return hashlib.blake2b(msg, key=key, digest_size=SIZE, fanout=1, depth=1, node_offset=UNKNOWN << 32).digest()


def output_node(root: bytes, i: int) -> bytes:
    """output block i: BLAKE2b(root) as a leaf of length 64 at node offset i, fanout 0, depth 0"""
    return blake2b_param(root, param_block(SIZE, 0, 0, 0, SIZE, i, UNKNOWN, 0, SIZE))


class XOF:
    """kyber.XOF over BLAKE2Xb: New(seed) keys with the first 64 seed bytes and writes the rest
    (blake.go:19-41).  Calling the object with a length reads that many bytes, so an XOF is a stream for
    ``Scalar.Pick``."""

    def __init__(self, seed: bytes = b""):
        seed = bytes(seed or b"")
        self._key, self._msg = seed[:SIZE], seed[SIZE:]
        self._root = None  # set by the first Read: no Write after it
        self._pos = 0

    def Write(self, src: bytes) -> int:
        if self._root is not None:
            raise ValueError("blake2xb: write to XOF after read")
        self._msg += bytes(src)
        return len(src)

    def Read(self, n: int) -> bytes:
        if self._root is None:
            self._root = root_hash(self._key, self._msg)
        out = bytearray()
        while len(out) < n:
            node, off = divmod(self._pos, SIZE)
            part = output_node(self._root, node)[off:off + n - len(out)]
            out += part
            self._pos += len(part)
        return bytes(out)

    __call__ = Read

    def Root(self) -> bytes:
        """the 64-byte root hash every output node compresses; fixes it as the first Read does (no Write after it)"""
        if self._root is None:
            self._root = root_hash(self._key, self._msg)
        return self._root

    def Tell(self) -> int:
        """the byte position of the next Read"""
        return self._pos

    def Skip(self, n: int) -> None:
        """advance the stream by n bytes, as a Read of n bytes does"""
        self.Root()
        self._pos += int(n)

    def XORKeyStream(self, src: bytes) -> bytes:  # blake.go:82-104
        return bytes(a ^ b for a, b in zip(src, self.Read(len(src))))

    def Clone(self) -> "XOF":  # blake.go:43-45
        c = XOF()
        c._key, c._msg, c._root, c._pos = self._key, self._msg, self._root, self._pos
        return c

    def Reseed(self) -> None:  # blake.go:55-74: a new XOF keyed with 128 bytes of this one's output
        self.__init__(self.Read(128))


def New(seed: bytes = b"") -> XOF:
    return XOF(seed)


def pick_int(stream) -> tuple:
    """(scalar, draws) of Scalar.Pick(stream) (scalar.go:180-184 -> util/random/rand.go:19-46): 32 stream bytes read
    big-endian, the top byte masked to 253 bits, redrawn until below l.  stream(n) returns n bytes."""
    draws = 0
    while True:
        b = bytearray(stream(32))
        draws += 1
        b[0] &= 0x1F
        v = int.from_bytes(b, "big")
        if v < ORDER:
            return v, draws


def pick(stream) -> bytes:
    """the 32 little-endian bytes of Scalar.Pick(stream)"""
    return pick_int(stream)[0].to_bytes(32, "little")
