// BLAKE2s compression and the BLAKE2Xs stream behind sign/bdn's coefficients.
//
// Replaces, in the reference:
//   blake2s.NewXOF(OutputLengthUnknown, nil) + Write + Read   bdn.go:29-47   -> blake2xs_root, blake2xs_node
// for the one shape hashPointToR uses: no key, every roster key's MarshalBinary bytes written in order, 16 bytes read per
// key.  The root node (digest 32, fanout 1, depth 1, XOF length 0xFFFF) hashes the message block by block and is
// sequential: ceil(len / 64) compressions in ONE lane.  Output node i (digest 32, fanout 0, depth 0, leaf length 32, node
// offset i, XOF length 0xFFFF, inner length 32) is one compression of the 32-byte root hash and independent of every
// other node: one lane per node, 32 stream bytes each, which is two coefficients.
// State and message words stay in registers: every round and sigma index is a compile-time constant, as in
// blake2xb.cuh.  Compiles with g++ too (tests/bdn_harness.cpp).
#pragma once
#include "hd.h"

#include <stdint.h>

namespace kyb {

#define KYB_BLAKE2S_IV {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u}

KYB_HD uint32_t blake2s_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// h <- F(h, m, t, last): RFC 7693 section 3.2 with 10 rounds; t = bytes hashed so far, this block included
KYB_HD void blake2s_compress_regs(uint32_t (&h)[8], const uint32_t (&m)[16], uint64_t t, bool last) {
    constexpr uint32_t IV[8] = KYB_BLAKE2S_IV;
    constexpr uint8_t S[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = h[i];
        v[8 + i] = IV[i];
    }
    v[12] ^= (uint32_t)t;
    v[13] ^= (uint32_t)(t >> 32);
    if (last) v[14] = ~v[14];
#define KYB_B2S_G(a, b, c, d, x, y)       \
    v[a] += v[b] + (x);                   \
    v[d] = blake2s_rotr(v[d] ^ v[a], 16); \
    v[c] += v[d];                         \
    v[b] = blake2s_rotr(v[b] ^ v[c], 12); \
    v[a] += v[b] + (y);                   \
    v[d] = blake2s_rotr(v[d] ^ v[a], 8);  \
    v[c] += v[d];                         \
    v[b] = blake2s_rotr(v[b] ^ v[c], 7);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        KYB_B2S_G(0, 4, 8, 12, m[S[r][0]], m[S[r][1]])
        KYB_B2S_G(1, 5, 9, 13, m[S[r][2]], m[S[r][3]])
        KYB_B2S_G(2, 6, 10, 14, m[S[r][4]], m[S[r][5]])
        KYB_B2S_G(3, 7, 11, 15, m[S[r][6]], m[S[r][7]])
        KYB_B2S_G(0, 5, 10, 15, m[S[r][8]], m[S[r][9]])
        KYB_B2S_G(1, 6, 11, 12, m[S[r][10]], m[S[r][11]])
        KYB_B2S_G(2, 7, 8, 13, m[S[r][12]], m[S[r][13]])
        KYB_B2S_G(3, 4, 9, 14, m[S[r][14]], m[S[r][15]])
    }
#undef KYB_B2S_G
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

// h0 = the root hash of `len` message bytes, read byte by byte (no alignment assumed, nothing read past data + len).
// The empty message is one compression of a zero block with t = 0.
KYB_HD void blake2xs_root(uint32_t (&h0)[8], const uint8_t* __restrict__ data, size_t len) {
    constexpr uint32_t IV[8] = KYB_BLAKE2S_IV;
#pragma unroll
    for (int i = 0; i < 8; i++) h0[i] = IV[i];
    h0[0] ^= 0x01010020u;  // digest 32, no key, fanout 1, depth 1
    h0[3] ^= 0x0000ffffu;  // XOF length 0xFFFF (leaf length, node offset, node depth, inner length: 0)
    const size_t blocks = len ? (len + 63) / 64 : 1;
#pragma unroll 1
    for (size_t b = 0; b < blocks; b++) {
        const size_t off = 64 * b, left = len - off, take = left < 64 ? left : 64;
        uint32_t m[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((size_t)(4 * i + k) < take) w |= (uint32_t)data[off + 4 * i + k] << (8 * k);
            m[i] = w;
        }
        blake2s_compress_regs(h0, m, (uint64_t)(off + take), b == blocks - 1);
    }
}

// o = stream bytes 32 i .. 32 i + 31 as eight little-endian words: output node i over the root hash
KYB_HD void blake2xs_node(uint32_t (&o)[8], const uint32_t (&h0)[8], uint32_t i) {
    constexpr uint32_t IV[8] = KYB_BLAKE2S_IV;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = IV[k];
    o[0] ^= 0x00000020u;  // digest 32, no key, fanout 0, depth 0
    o[1] ^= 32u;          // leaf length
    o[2] ^= i;            // node offset
    o[3] ^= 0x2000ffffu;  // XOF length 0xFFFF, node depth 0, inner length 32
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        m[k] = h0[k];
        m[8 + k] = 0;
    }
    blake2s_compress_regs(o, m, 32, true);
}

}  // namespace kyb
