// Per-lane hashing of the Boneh-Franklin CCA scheme of encrypt/ibe (ibe.go:51-281) with the suite hash SHA-256 on
// BLS12-381: H2 over the 576 GT bytes (gtToHash, ibe.go:297-313), H4 (ibe.go:283-295) and h3's rejection sampling
// (ibe.go:234-281).  One ciphertext per lane; all lanes of a launch share one message length L (0..32), so the loops
// below are uniform but for h3's trip count.
//
// 32-byte values (sigma, msg, digests) live in eight big-endian words, bytes beyond L zero: every byte is picked out of
// registers by compile-time index or by an unrolled select, never by a run-time index into a private array (which
// would put the array in scratch memory).  Compiles for the host too (tests/ibe_harness.cpp checks it against hashlib).
#pragma once
#include "sha256.cuh"

namespace kyb {
namespace ibe {

constexpr int MSG_MAX = 32;           // s.Hash().Size(): longer plaintexts are an error in the reference
constexpr int ST_IBE_CHECK = 3;       // include/kyber_hip.h KYB_ST_IBE_CHECK
constexpr int ST_IBE_H3 = 4;          // include/kyber_hip.h KYB_ST_IBE_H3
constexpr int GT_BYTES = 576;

// the order r of BLS12-381's groups, big-endian words (kilic/scalar.go:11-12)
KYB_HD uint32_t order_word(int k) {
    constexpr uint32_t R[8] = {0x73EDA753, 0x299D7D48, 0x3339D808, 0x09A1D805, 0x53BDA402, 0xFFFE5BFE, 0xFFFFFFFF, 0x00000001};
    return R[k];
}

// byte idx (0..31) of eight big-endian words; idx may be a run-time value (eight selects)
KYB_HD uint32_t byte_of(const uint32_t (&w)[8], int idx) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v = (k == (idx >> 2)) ? w[k] : v;
    return (v >> (24 - 8 * (idx & 3))) & 0xffu;
}

// 32 bytes (at most `len` of them read, the rest zero) -> big-endian words
KYB_HD void load_words(uint32_t (&w)[8], const uint8_t* p, int len) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) v |= (4 * k + j < len ? (uint32_t)p[4 * k + j] : 0u) << (24 - 8 * j);
        w[k] = v;
    }
}
KYB_HD void store_words(uint8_t* p, const uint32_t (&w)[8], int len) {
#pragma unroll
    for (int k = 0; k < 32; k++)
        if (k < len) p[k] = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
}

// SHA-256 of a message of `len` <= 119 bytes whose byte p is byte(p): at most two blocks, built in registers
template <class ByteFn>
KYB_HD void sha256_short(uint32_t (&h)[8], int len, ByteFn byte) {
    h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a;
    h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
    const int nblk = len + 9 <= 64 ? 1 : 2;
#pragma unroll
    for (int b = 0; b < 2; b++) {
        if (b >= nblk) break;
        uint32_t blk[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int p = 64 * b + 4 * k + j;
                const uint32_t c = p < len ? byte(p) : (p == len ? 0x80u : 0u);
                v |= c << (24 - 8 * j);
            }
            blk[k] = v;
        }
        if (b == nblk - 1) {
            blk[14] = 0;
            blk[15] = (uint32_t)len * 8u;
        }
        sha256_block_inl(h, blk);
    }
}

// "IBE-" and the tag's last two characters ("H2", "H3", "H4"), big-endian
constexpr uint32_t TAG_HEAD = 0x4942452Du;
KYB_HD uint32_t tag_byte(int p, uint32_t tag2) { return p < 4 ? (TAG_HEAD >> (24 - 8 * p)) & 0xffu : (tag2 >> (8 * (5 - p))) & 0xffu; }

// big-endian word m (bytes 4m .. 4m + 3) of a 4-byte aligned buffer
KYB_HD uint32_t ld_be32(const uint8_t* p, int m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap32(reinterpret_cast<const uint32_t*>(p)[m]);
#else
    const uint8_t* q = p + 4 * m;
    return ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
#endif
}

// H2: SHA-256("IBE-H2" || gt), gt = the 576 bytes of GTElt.MarshalBinary (4-byte aligned).  The 582-byte message and
// its padding are ten blocks; message word j >= 2 is the tail of gt word j - 2 and the head of gt word j - 1.
KYB_HD void h2(uint32_t (&h)[8], const uint8_t* gt) {
    h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a;
    h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
    constexpr int GW = GT_BYTES / 4;  // 144 words of gt
    uint32_t prev = 0;                // gt word j - 2
#pragma unroll 1
    for (int b = 0; b < 10; b++) {
        uint32_t blk[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int j = 16 * b + k;
            uint32_t v;
            if (j == 0) v = TAG_HEAD;
            else if (j == 1) {
                prev = ld_be32(gt, 0);
                v = 0x48320000u | (prev >> 16);
            } else if (j < GW + 1) {
                const uint32_t cur = ld_be32(gt, j - 1);
                v = (prev << 16) | (cur >> 16);
                prev = cur;
            } else if (j == GW + 1) v = (prev << 16) | 0x8000u;  // the last two bytes of gt, then the padding's 0x80
            else if (j == 159) v = (uint32_t)(6 + GT_BYTES) * 8u;
            else v = 0;
            blk[k] = v;
        }
        sha256_block_inl(h, blk);
    }
}

// H4: SHA-256("IBE-H4" || sigma), sigma of len bytes
KYB_HD void h4(uint32_t (&h)[8], const uint32_t (&sigma)[8], int len) {
    sha256_short(h, 6 + len, [&](int p) -> uint32_t { return p < 6 ? tag_byte(p, 0x4834u) : byte_of(sigma, p - 6); });
}

// h3 (ibe.go:234-281): buf = SHA-256("IBE-H3" || sigma || msg); for i = 1 .. 65534, SHA-256(LE16(i) || buf) with the
// first byte shifted right by one bit (32-byte big-endian scalars, 255-bit order) is r when it is below the order.
// Returns 0 and r (big-endian words), or ST_IBE_H3 when all tries are rejected (the reference's "rejection sampling
// failure"; r is zero then).
KYB_HD int h3(uint32_t (&r)[8], const uint32_t (&sigma)[8], const uint32_t (&msg)[8], int len) {
    uint32_t buf[8];
    sha256_short(buf, 6 + 2 * len, [&](int p) -> uint32_t {
        return p < 6 ? tag_byte(p, 0x4833u) : (p < 6 + len ? byte_of(sigma, p - 6) : byte_of(msg, p - 6 - len));
    });
    // the 34-byte message LE16(i) || buf in one block: buf shifted by two bytes, the padding's 0x80 at byte 34
    uint32_t tail[9];
    tail[0] = buf[0] >> 16;
#pragma unroll
    for (int k = 1; k < 8; k++) tail[k] = (buf[k - 1] << 16) | (buf[k] >> 16);
    tail[8] = (buf[7] << 16) | 0x8000u;
#pragma unroll 1
    for (uint32_t i = 1; i < 65535u; i++) {
        uint32_t blk[16];
        blk[0] = ((i & 0xffu) << 24) | ((i >> 8) << 16) | tail[0];
#pragma unroll
        for (int k = 1; k < 9; k++) blk[k] = tail[k];
#pragma unroll
        for (int k = 9; k < 15; k++) blk[k] = 0;
        blk[15] = 34 * 8;
        uint32_t d[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        sha256_block_inl(d, blk);
        d[0] = (d[0] & 0x00ffffffu) | ((d[0] >> 25) << 24);  // hashed[0] >>= 1
        // d < r, big-endian word by word
        int lt = 0;
        bool decided = false;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t o = order_word(k);
            if (!decided && d[k] != o) {
                lt = d[k] < o;
                decided = true;
            }
        }
        if (lt) {
#pragma unroll
            for (int k = 0; k < 8; k++) r[k] = d[k];
            return 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = 0;
    return ST_IBE_H3;
}

// xor of the first len bytes of a digest into a (zero-padded) value
KYB_HD void xor_words(uint32_t (&out)[8], const uint32_t (&a)[8], const uint32_t (&d)[8], int len) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int keep = len - 4 * k;  // bytes of word k inside the message
        const uint32_t mask = keep >= 4 ? 0xffffffffu : (keep <= 0 ? 0u : ~(0xffffffffu >> (8 * keep)));
        out[k] = (a[k] ^ d[k]) & mask;
    }
}

}  // namespace ibe
}  // namespace kyb
