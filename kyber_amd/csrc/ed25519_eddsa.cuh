// sign/eddsa signing on Ed25519 (eddsa.go): the lane programs of ed25519_eddsa.hip.
//
// Replaces, in the reference:
//   Curve.NewKeyAndSeedWithInput, Mul(secret, nil)   curve.go:51-60, eddsa.go:50-51, 81-86 -> ed_eddsa_expand_lane
//   Sign's nonce: r = SHA-512(prefix || msg) mod l   eddsa.go:92-101                        -> ed_eddsa_nonce
//   Sign's point: R = r B                            eddsa.go:102                            -> ed_eddsa_nonce_lane
//   Sign's challenge and response                    eddsa.go:104-141                        -> ed_eddsa_sign_element
// Everything but the two hashes' heads stands elsewhere and is used as it stands: the schedule in registers and the
// reduction of a digest (sha512_compress_regs, sc_reduce512, ed_hram: ed25519_verify.cuh), the response and a
// signature's last pass (ed_schnorr_response, ed_schnorr_sign_element: ed25519_vss.cuh -- EdDSA's S = r + h a is
// Schnorr's with the nonce r and the key a), the comb (recode16, ed_comb_mul_base).  New here: a SHA-512 whose head is
// 32 bytes -- the prefix -- with the message streamed from global memory behind it, and the one-block hash of a seed.
// A nonce lane hashes FIRST and multiplies after, as ed_verify_lane does: the hash's working set (24 64-bit words) and
// the point's never meet in the registers.
// Compiles with g++ too (tests/eddsa_harness.cpp runs these programs on the CPU against the oracle).
#pragma once
#include "ed25519_vss.cuh"

namespace kyb {

// ed_hram_msg_word for a message with 32 hashed bytes in front of it instead of 64: the stream's words are the same but
// for the length, and the word at lenpos holds nothing else (the 0x80 and the high half of the 128-bit length lie
// before it), so the 32 bytes' 256 bits come off as a number.
KYB_DEV uint64_t ed_eddsa_msg_word(const uint8_t* __restrict__ msg, size_t len, size_t pos, size_t lenpos) {
    uint64_t v = ed_hram_msg_word(msg, len, pos, lenpos);
    if (pos == lenpos) v -= 32 * 8;
    return v;
}

// The 64 bytes of a SHA-512 state as sixteen little-endian words (the digest's bytes are h[0..7] big-endian)
KYB_DEV void ed_eddsa_digest_words(uint32_t (&x)[16], const uint64_t (&h)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t le = __builtin_bswap64(h[i]);
        x[2 * i] = (uint32_t)le;
        x[2 * i + 1] = (uint32_t)(le >> 32);
    }
}

// r = SHA-512(prefix || msg) mod l as eight little-endian words (eddsa.go:92-101).  The first block is the prefix and
// the message's first 96 bytes; the others are the message's alone, from byte 96 on.
KYB_DEV void ed_eddsa_nonce(uint32_t (&rw)[8], const uint32_t pw[8], const uint8_t* __restrict__ msg, size_t len, const sf::Mod& m) {
    uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    const size_t padded = (32 + len + 17 + 127) / 128 * 128;  // bytes hashed, padding and length included
    const size_t lenpos = padded - 32 - 8;
    uint64_t w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = ed_be64(pw[2 * i], pw[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 12; i++) w[4 + i] = ed_eddsa_msg_word(msg, len, 8 * i, lenpos);
    sha512_compress_regs(h, w);
#pragma unroll 1
    for (size_t pos = 96; pos + 32 < padded; pos += 128) {
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = ed_eddsa_msg_word(msg, len, pos + 8 * i, lenpos);
        sha512_compress_regs(h, w);
    }
    uint32_t x[16];
    ed_eddsa_digest_words(x, h);
    sc_reduce512(rw, x, m);
}

// One signature's first pass: r, then R = r B on the comb (r < l: no digit is dropped)
KYB_DEV void ed_eddsa_nonce_lane(ge_p3& R, uint32_t (&rw)[8], const uint32_t pw[8], const uint8_t* __restrict__ msg, size_t len,
                                 const int32_t* __restrict__ wide, const sf::Mod& m) {
    ed_eddsa_nonce(rw, pw, msg, len, m);
    int8_t e[65];
    recode16(e, rw, false);
    ed_comb_mul_base(R, e, wide);
}

// One signature's last pass: sig = R || (r + h a mod l) with h = SHA-512(R || A || msg) mod l.  rb: R's bytes from the
// encoder; aw: the public key's bytes as the caller gave them, hashed as they stand (eddsa.go:110-118); sw: the secret,
// any 32 bytes (the clamped digest is not reduced).
KYB_DEV void ed_eddsa_sign_element(uint32_t (&sig)[16], const uint32_t rb[8], const uint32_t aw[8], const uint32_t rw[8],
                                   const uint32_t sw[8], const uint8_t* __restrict__ msg, size_t len, const sf::Mod& m) {
    ed_schnorr_sign_element(sig, rb, aw, rw, sw, msg, len, m);
}

// SHA-512 of a 32-byte seed, ONE block; secret = digest[0:32] clamped and NOT reduced, prefix = digest[32:64]
// (curve.go:51-60), both as little-endian words
KYB_DEV void ed_eddsa_expand_seed(uint32_t (&secret)[8], uint32_t (&prefix)[8], const uint32_t seed[8]) {
    uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    uint64_t w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = ed_be64(seed[2 * i], seed[2 * i + 1]);
    w[4] = 0x8000000000000000ull;
#pragma unroll
    for (int i = 5; i < 15; i++) w[i] = 0;
    w[15] = 32 * 8;
    sha512_compress_regs(h, w);
    uint32_t x[16];
    ed_eddsa_digest_words(x, h);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        secret[i] = x[i];
        prefix[i] = x[8 + i];
    }
    secret[0] &= 0xfffffff8u;                              // digest[0] &= 0xf8
    secret[7] = (secret[7] & 0x7fffffffu) | 0x40000000u;  // digest[31] &= 0x7f, |= 0x40
}

// One key: the seed's hash, then A = secret B on the comb -- kyb_ed25519_mul_base's value at flags 0 (secret < 2^255)
KYB_DEV void ed_eddsa_expand_lane(ge_p3& A, uint32_t (&secret)[8], uint32_t (&prefix)[8], const uint32_t seed[8],
                                  const int32_t* __restrict__ wide) {
    ed_eddsa_expand_seed(secret, prefix, seed);
    int8_t e[65];
    recode16(e, secret, false);
    ed_comb_mul_base(A, e, wide);
}

}  // namespace kyb
