// BLAKE2b compression and the BLAKE2Xb stream behind Scalar.Pick, one stream per lane.
//
// Replaces, in the reference:
//   xof/blake2xb New(seed) + Read        blake.go:19-41, 47-49   -> the root node and the output nodes below
//   util/random Bits / Int               rand.go:19-46           -> the draw: 32 bytes big-endian, 253 bits, redrawn if >= l
//   edwards25519 scalar.Pick             scalar.go:180-184       -> ed_scalar_pick
// for the one shape proof/dleq and share/pvss use: Pick(suite.XOF(cb)) with cb a 32-byte SHA-256 digest.  A seed of at
// most 64 bytes is the BLAKE2b KEY (blake.go:20-27), the message is empty, so the root node is one compression of the
// zero-padded key block; output node i is one compression of the 64-byte root hash under a leaf parameter block.
// State and message words stay in registers: every round and sigma index is a compile-time constant
// (sha512_compress_regs keeps its schedule the same way).  Compiles with g++ too (tests/dleq_harness.cpp).
#pragma once
#include "hd.h"

#include <stdint.h>

namespace kyb {

#define KYB_BLAKE2B_IV                                                                                           \
    {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, \
     0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull}

KYB_HD uint64_t blake2b_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// h <- F(h, m, t, last): RFC 7693 section 3.2 with 12 rounds; t = bytes hashed so far, this block included (< 2^64)
KYB_HD void blake2b_compress_regs(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t, bool last) {
    constexpr uint64_t IV[8] = KYB_BLAKE2B_IV;
    constexpr uint8_t S[12][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = h[i];
        v[8 + i] = IV[i];
    }
    v[12] ^= t;
    if (last) v[14] = ~v[14];
#define KYB_B2B_G(a, b, c, d, x, y)        \
    v[a] += v[b] + (x);                    \
    v[d] = blake2b_rotr(v[d] ^ v[a], 32);  \
    v[c] += v[d];                          \
    v[b] = blake2b_rotr(v[b] ^ v[c], 24);  \
    v[a] += v[b] + (y);                    \
    v[d] = blake2b_rotr(v[d] ^ v[a], 16);  \
    v[c] += v[d];                          \
    v[b] = blake2b_rotr(v[b] ^ v[c], 63);
#pragma unroll
    for (int r = 0; r < 12; r++) {
        KYB_B2B_G(0, 4, 8, 12, m[S[r][0]], m[S[r][1]])
        KYB_B2B_G(1, 5, 9, 13, m[S[r][2]], m[S[r][3]])
        KYB_B2B_G(2, 6, 10, 14, m[S[r][4]], m[S[r][5]])
        KYB_B2B_G(3, 7, 11, 15, m[S[r][6]], m[S[r][7]])
        KYB_B2B_G(0, 5, 10, 15, m[S[r][8]], m[S[r][9]])
        KYB_B2B_G(1, 6, 11, 12, m[S[r][10]], m[S[r][11]])
        KYB_B2B_G(2, 7, 8, 13, m[S[r][12]], m[S[r][13]])
        KYB_B2B_G(3, 4, 9, 14, m[S[r][14]], m[S[r][15]])
    }
#undef KYB_B2B_G
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

// The chaining value a node starts from: IV ^ its 64-byte parameter block.
// Root of blake2b.NewXOF(OutputLengthUnknown, key) with a 32-byte key: digest 64, key length 32, fanout 1, depth 1,
// xof length 0xFFFFFFFF in the upper half of the node offset.
KYB_HD void blake2xb_root_iv(uint64_t (&h)[8]) {
    constexpr uint64_t IV[8] = KYB_BLAKE2B_IV;
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= 0x01012040ull;
    h[1] ^= 0xffffffff00000000ull;
}
// Output node i: digest 64, key length 0, fanout 0, depth 0, leaf length 64, node offset i, xof length 0xFFFFFFFF,
// node depth 0, inner length 64.
KYB_HD void blake2xb_node_iv(uint64_t (&h)[8], uint32_t i) {
    constexpr uint64_t IV[8] = KYB_BLAKE2B_IV;
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = IV[k];
    h[0] ^= 0x40ull | (64ull << 32);
    h[1] ^= 0xffffffff00000000ull | i;
    h[2] ^= 0x4000ull;
}

constexpr int ED_PICK_MAX_NODES = 64;  // 128 draws: a lane that exhausts them has met a 2^-128 event

// 32 stream bytes, held as four little-endian 64-bit words o[0..3] in stream order, read as the reference reads a draw
// (rand.go:19-31: big-endian, the first byte masked to 253 bits) into eight little-endian scalar words; true iff < l.
KYB_HD bool ed_pick_draw(uint32_t (&c)[8], uint64_t o0, uint64_t o1, uint64_t o2, uint64_t o3) {
    const uint64_t w[4] = {__builtin_bswap64(o3), __builtin_bswap64(o2), __builtin_bswap64(o1), __builtin_bswap64(o0)};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c[2 * i] = (uint32_t)w[i];
        c[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    c[7] &= 0x1fffffffu;
    // l = 2^252 + 0x14def9dea2f79cd65812631a5cf5d3ed (const.go:15)
    constexpr uint32_t L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0, 0, 0, 0x10000000u};
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t d = (uint64_t)c[i] - L[i] - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    return borrow != 0;
}

// c = scalar.Pick(blake2xb.New(cb)) for a 32-byte seed cb (eight little-endian words of the seed's bytes).  Returns the
// number of draws taken, or 0 when ED_PICK_MAX_NODES output nodes held no scalar below l (c is then zero).
// One compression site serves the root and every output node: the first trip hashes the key block, each later one the
// root hash under the next node's parameter block.  About half of all draws are rejected, so the trips differ per lane:
// the loop's condition is the lane's own, and a wave leaves it when its last lane has accepted.
KYB_HD int ed_scalar_pick(uint32_t (&c)[8], const uint32_t cb[8]) {
    uint64_t h[8], m[16];
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = (uint64_t)cb[2 * i] | ((uint64_t)cb[2 * i + 1] << 32);
#pragma unroll
    for (int i = 4; i < 16; i++) m[i] = 0;
    blake2xb_root_iv(h);
    uint64_t t = 128;  // the key block counts in full
    int draws = 0;
    bool done = false;
#pragma unroll 1
    for (int node = -1; node < ED_PICK_MAX_NODES && !done; node++) {
        blake2b_compress_regs(h, m, t, true);
        if (node < 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) m[i] = h[i];  // the root hash is every node's message
            t = 64;
        } else {
            done = ed_pick_draw(c, h[0], h[1], h[2], h[3]);
            draws = 2 * node + 1;
            if (!done) {
                done = ed_pick_draw(c, h[4], h[5], h[6], h[7]);
                draws = 2 * node + 2;
            }
        }
        blake2xb_node_iv(h, (uint32_t)(node + 1));
    }
    if (!done) {
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = 0;
        return 0;
    }
    return draws;
}

}  // namespace kyb
