// AES-256-GCM (FIPS 197, NIST SP 800-38D) with a 12-byte nonce and no additional data, one message per lane: what Go's
// cipher.NewGCM(aes.NewCipher(key)).Seal / Open compute for encrypt/ecies (ecies.go:56-64, 100-111).  Curve-independent.
//
// A lane streams its message block by block: CTR keystream, GHASH over the ciphertext, nothing of the message kept.
// Only the forward cipher is needed (CTR and the tag both encrypt).  The S-box is a 256-byte table the caller owns --
// LDS in the kernel, a plain array on the host -- and the 60 round-key words live behind a put / get pair like the
// encoder's prefix products (EncPreLds): in LDS as [word][lane] columns, where a wave's read of one round-key word is 64
// consecutive words, or in a lane-private array on the host.  State, counter and the GHASH accumulator are registers.
// GHASH multiplies bit by bit (128 shift-and-conditional-xor steps per block, no table): a 32-byte share is three blocks
// next to a scalar multiplication of a few hundred thousand instructions, and long messages only have to be correct.
// Compiles with g++ too (tests/dkg_harness.cpp runs it against the fixtures of tests/golden/aes256gcm.json).
#pragma once
#include "hd.h"

namespace kyb {

struct AesSbox {
    uint8_t v[256];
};
// The S-box from its definition: the multiplicative inverse in GF(2^8) mod x^8 + x^4 + x^3 + x + 1 (p runs through the
// powers of the generator 3, q through the powers of its inverse) followed by the affine map.
constexpr AesSbox aes_make_sbox() {
    AesSbox s{};
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ (uint8_t)(p << 1) ^ ((p & 0x80) ? 0x1b : 0));
        q = (uint8_t)(q ^ (uint8_t)(q << 1));
        q = (uint8_t)(q ^ (uint8_t)(q << 2));
        q = (uint8_t)(q ^ (uint8_t)(q << 4));
        q = (uint8_t)(q ^ ((q & 0x80) ? 0x09 : 0));
        const uint8_t x = (uint8_t)(q ^ (uint8_t)((q << 1) | (q >> 7)) ^ (uint8_t)((q << 2) | (q >> 6)) ^
                                    (uint8_t)((q << 3) | (q >> 5)) ^ (uint8_t)((q << 4) | (q >> 4)));
        s.v[p] = (uint8_t)(x ^ 0x63);
    } while (p != 1);
    s.v[0] = 0x63;
    return s;
}
// sbox[first], sbox[first + stride], ... copied into the caller's table (a block of `stride` lanes fills its LDS copy)
KYB_HD void aes_fill_sbox(uint8_t* sbox, int first, int stride) {
    constexpr AesSbox S = aes_make_sbox();
    for (int i = first; i < 256; i += stride) sbox[i] = S.v[i];
}

// Round keys in a lane-private array (the host build, and the reference layout the LDS one is tested against)
struct AesKeysLocal {
    uint32_t w[60];
    KYB_HD void put(int i, uint32_t v) { w[i] = v; }
    KYB_HD uint32_t get(int i) const { return w[i]; }
};
// Round keys in LDS, [word][lane]: col = the block's array + threadIdx.x
template <int LANES>
struct AesKeysLds {
    uint32_t* col;
    static constexpr int WORDS = 60 * LANES;
    KYB_HD void put(int i, uint32_t v) { col[i * LANES] = v; }
    KYB_HD uint32_t get(int i) const { return col[i * LANES]; }
};
// The AEAD kernels of the Ed25519 units: a block of ED_AEAD_BLOCK lanes keeps the S-box and its lanes' round keys in LDS
constexpr unsigned ED_AEAD_BLOCK = 64;
constexpr size_t ED_AEAD_LDS_BYTES = 256 + sizeof(uint32_t) * AesKeysLds<ED_AEAD_BLOCK>::WORDS;
static_assert(ED_AEAD_LDS_BYTES == 15616, "S-box + 64 lanes x 60 round-key words: ten blocks on a CU's 160 KiB");

KYB_HD uint32_t aes_subword(uint32_t x, const uint8_t* sbox) {
    return ((uint32_t)sbox[x >> 24] << 24) | ((uint32_t)sbox[(x >> 16) & 255] << 16) | ((uint32_t)sbox[(x >> 8) & 255] << 8) |
           (uint32_t)sbox[x & 255];
}

// KeyExpansion for Nk = 8 (FIPS 197 section 5.2): key = eight big-endian words, 60 round-key words out
template <class RK>
KYB_HD void aes256_expand(RK& rk, const uint32_t key[8], const uint8_t* sbox) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        k[i] = key[i];
        rk.put(i, k[i]);
    }
    uint32_t rcon = 1;
#pragma unroll 1
    for (int r = 0; r < 7; r++) {
        k[0] ^= aes_subword((k[7] << 8) | (k[7] >> 24), sbox) ^ (rcon << 24);
        k[1] ^= k[0];
        k[2] ^= k[1];
        k[3] ^= k[2];
#pragma unroll
        for (int i = 0; i < 4; i++) rk.put(8 + 8 * r + i, k[i]);
        if (r == 6) break;  // 60 words: the last group is half a key
        k[4] ^= aes_subword(k[3], sbox);
        k[5] ^= k[4];
        k[6] ^= k[5];
        k[7] ^= k[6];
#pragma unroll
        for (int i = 0; i < 4; i++) rk.put(12 + 8 * r + i, k[4 + i]);
        rcon <<= 1;
    }
}

KYB_HD uint32_t aes_xtime4(uint32_t x) {  // four bytes times x in GF(2^8), side by side
    return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1bu);
}

// out = Cipher(in) (FIPS 197 section 5.1), 14 rounds; a block is four big-endian words, word c = column c
template <class RK>
KYB_HD void aes256_encrypt(uint32_t (&out)[4], const uint32_t (&in)[4], const RK& rk, const uint8_t* sbox) {
    uint32_t s[4], t[4];
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = in[c] ^ rk.get(c);
#pragma unroll 1
    for (int r = 1; r <= 14; r++) {
#pragma unroll
        for (int c = 0; c < 4; c++)  // SubBytes + ShiftRows: row j of column c comes from column c + j
            t[c] = ((uint32_t)sbox[s[c] >> 24] << 24) | ((uint32_t)sbox[(s[(c + 1) & 3] >> 16) & 255] << 16) |
                   ((uint32_t)sbox[(s[(c + 2) & 3] >> 8) & 255] << 8) | (uint32_t)sbox[s[(c + 3) & 3] & 255];
        if (r < 14) {
#pragma unroll
            for (int c = 0; c < 4; c++) {  // MixColumns: 2 a_j + 3 a_(j+1) + a_(j+2) + a_(j+3) in every row j
                const uint32_t a = t[c], a1 = (a << 8) | (a >> 24), a2 = (a << 16) | (a >> 16), a3 = (a << 24) | (a >> 8);
                t[c] = aes_xtime4(a ^ a1) ^ a1 ^ a2 ^ a3;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) s[c] = t[c] ^ rk.get(4 * r + c);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = s[c];
}

// GHASH (SP 800-38D section 6.4): y = (y ^ x) * h in GF(2^128), blocks as two big-endian 64-bit halves
struct Ghash {
    uint64_t hh, hl, yh, yl;
    KYB_HD void init(const uint32_t (&h)[4]) {
        hh = ((uint64_t)h[0] << 32) | h[1];
        hl = ((uint64_t)h[2] << 32) | h[3];
        yh = yl = 0;
    }
    KYB_HD void update(const uint32_t (&x)[4]) {
        uint64_t xh = yh ^ (((uint64_t)x[0] << 32) | x[1]), xl = yl ^ (((uint64_t)x[2] << 32) | x[3]);
        uint64_t zh = 0, zl = 0, vh = hh, vl = hl;
#pragma unroll 1
        for (int i = 0; i < 128; i++) {
            const uint64_t take = 0 - (xh >> 63);  // bit i of x, most significant first
            zh ^= vh & take;
            zl ^= vl & take;
            xh = (xh << 1) | (xl >> 63);
            xl <<= 1;
            const uint64_t fold = 0 - (vl & 1);
            vl = (vl >> 1) | (vh << 63);
            vh = (vh >> 1) ^ (fold & 0xe100000000000000ull);
        }
        yh = zh;
        yl = zl;
    }
};

// bytes p[0 .. cnt) as a zero-padded block, cnt <= 16: nothing is read at or past p + cnt
KYB_HD void gcm_load_block(uint32_t (&w)[4], const uint8_t* p, size_t cnt) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) v = (v << 8) | ((size_t)(4 * c + k) < cnt ? (uint32_t)p[4 * c + k] : 0u);
        w[c] = v;
    }
}
KYB_HD void gcm_store_block(uint8_t* p, const uint32_t (&w)[4], size_t cnt) {
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int k = 0; k < 4; k++)
            if ((size_t)(4 * c + k) < cnt) p[4 * c + k] = (uint8_t)(w[c] >> (24 - 8 * k));
}

// One message under one (key schedule, 12-byte nonce): the hash key H = E(0), the tag mask E(nonce || 1), data blocks
// from counter 2 on (SP 800-38D section 7.1 with a 96-bit IV).
template <class RK>
struct Gcm {
    const RK& rk;
    const uint8_t* sbox;
    uint32_t ctr[4];
    Ghash g;
    KYB_HD Gcm(const RK& rk_, const uint8_t* sbox_, const uint32_t nonce[3]) : rk(rk_), sbox(sbox_) {
        const uint32_t zero[4] = {0, 0, 0, 0};
        uint32_t h[4];
        aes256_encrypt(h, zero, rk, sbox);
        g.init(h);
        ctr[0] = nonce[0];
        ctr[1] = nonce[1];
        ctr[2] = nonce[2];
        ctr[3] = 1;
    }
    KYB_HD void keystream(uint32_t (&ks)[4], uint32_t counter) {
        const uint32_t in[4] = {ctr[0], ctr[1], ctr[2], counter};
        aes256_encrypt(ks, in, rk, sbox);
    }
    // the tag once every ciphertext block has been hashed: GHASH's length block (no additional data), then the mask
    KYB_HD void tag(uint32_t (&t)[4], uint64_t len) {
        const uint64_t bits = len * 8;
        const uint32_t lb[4] = {0, 0, (uint32_t)(bits >> 32), (uint32_t)bits};
        g.update(lb);
        uint32_t ks[4];
        keystream(ks, 1);
        t[0] = (uint32_t)(g.yh >> 32) ^ ks[0];
        t[1] = (uint32_t)g.yh ^ ks[1];
        t[2] = (uint32_t)(g.yl >> 32) ^ ks[2];
        t[3] = (uint32_t)g.yl ^ ks[3];
    }
};

// out[0 .. len + 16) = Seal(nonce, msg[0 .. len), no additional data): ciphertext, then the tag
template <class RK>
KYB_HD void gcm_seal(uint8_t* out, const uint8_t* msg, uint64_t len, const uint32_t nonce[3], const RK& rk, const uint8_t* sbox) {
    Gcm<RK> gcm(rk, sbox, nonce);
    uint32_t counter = 2;
#pragma unroll 1
    for (uint64_t pos = 0; pos < len; pos += 16, counter++) {
        const size_t cnt = len - pos < 16 ? (size_t)(len - pos) : 16;
        uint32_t b[4], ks[4];
        gcm_load_block(b, msg + pos, cnt);
        gcm.keystream(ks, counter);
#pragma unroll
        for (int c = 0; c < 4; c++) b[c] ^= ks[c];
        gcm_store_block(out + pos, b, cnt);
#pragma unroll
        for (int c = 0; c < 4; c++) {  // the hash takes the ciphertext zero-padded: the keystream's tail is cut off
            const int nb = (int)cnt - 4 * c;
            b[c] &= nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : ~(0xffffffffu >> (8 * nb)));
        }
        gcm.g.update(b);
    }
    uint32_t t[4];
    gcm.tag(t, len);
    gcm_store_block(out + len, t, 16);
}

// ct[0 .. len) is the ciphertext and ct[len .. len + 16) its tag.  True and out[0 .. len) = the plaintext when the tag
// is right; otherwise false and out[0 .. len) zero: two passes, so that no unauthenticated byte is ever written.
template <class RK>
KYB_HD bool gcm_open(uint8_t* out, const uint8_t* ct, uint64_t len, const uint32_t nonce[3], const RK& rk, const uint8_t* sbox) {
    Gcm<RK> gcm(rk, sbox, nonce);
#pragma unroll 1
    for (uint64_t pos = 0; pos < len; pos += 16) {
        uint32_t b[4];
        gcm_load_block(b, ct + pos, len - pos < 16 ? (size_t)(len - pos) : 16);
        gcm.g.update(b);
    }
    uint32_t t[4], want[4];
    gcm.tag(t, len);
    gcm_load_block(want, ct + len, 16);
    const bool ok = ((t[0] ^ want[0]) | (t[1] ^ want[1]) | (t[2] ^ want[2]) | (t[3] ^ want[3])) == 0;
    uint32_t counter = 2;
#pragma unroll 1
    for (uint64_t pos = 0; pos < len; pos += 16, counter++) {
        const size_t cnt = len - pos < 16 ? (size_t)(len - pos) : 16;
        uint32_t b[4] = {0, 0, 0, 0}, ks[4];
        if (ok) {
            gcm_load_block(b, ct + pos, cnt);
            gcm.keystream(ks, counter);
#pragma unroll
            for (int c = 0; c < 4; c++) b[c] ^= ks[c];
        }
        gcm_store_block(out + pos, b, cnt);
    }
    return ok;
}

// ---------------------------------------------------------------------------------- with additional data (share/vss)
// Seal / Open with additional data of aad_blocks whole 16-byte blocks, hashed in front of the ciphertext; the length
// block then carries both bit lengths (SP 800-38D section 7.1).  aad(i): big-endian word i of the data, four per block
// (a callable: the caller reads the words from wherever they live).  What Go's gcm.Seal(nil, nonce, msg, aad) / gcm.Open
// compute for share/vss (vss.go:246, 453), whose context is 32 bytes (pedersen) or 128 (rabin).
template <class RK>
KYB_HD void gcm_tag_aad(uint32_t (&t)[4], Gcm<RK>& gcm, int aad_blocks, uint64_t len) {
    const uint64_t abits = (uint64_t)aad_blocks * 128, bits = len * 8;
    const uint32_t lb[4] = {(uint32_t)(abits >> 32), (uint32_t)abits, (uint32_t)(bits >> 32), (uint32_t)bits};
    gcm.g.update(lb);
    uint32_t ks[4];
    gcm.keystream(ks, 1);
    t[0] = (uint32_t)(gcm.g.yh >> 32) ^ ks[0];
    t[1] = (uint32_t)gcm.g.yh ^ ks[1];
    t[2] = (uint32_t)(gcm.g.yl >> 32) ^ ks[2];
    t[3] = (uint32_t)gcm.g.yl ^ ks[3];
}
template <class RK, class Aad>
KYB_HD void gcm_hash_aad(Gcm<RK>& gcm, Aad aad, int aad_blocks) {
#pragma unroll 1
    for (int b = 0; b < aad_blocks; b++) {
        const uint32_t x[4] = {aad(4 * b), aad(4 * b + 1), aad(4 * b + 2), aad(4 * b + 3)};
        gcm.g.update(x);
    }
}

// out[0 .. len + 16) = Seal(nonce, msg[0 .. len), aad): ciphertext, then the tag
template <class RK, class Aad>
KYB_HD void gcm_seal_aad(uint8_t* out, const uint8_t* msg, uint64_t len, const uint32_t nonce[3], const RK& rk, const uint8_t* sbox,
                         Aad aad, int aad_blocks) {
    Gcm<RK> gcm(rk, sbox, nonce);
    gcm_hash_aad(gcm, aad, aad_blocks);
    uint32_t counter = 2;
#pragma unroll 1
    for (uint64_t pos = 0; pos < len; pos += 16, counter++) {
        const size_t cnt = len - pos < 16 ? (size_t)(len - pos) : 16;
        uint32_t b[4], ks[4];
        gcm_load_block(b, msg + pos, cnt);
        gcm.keystream(ks, counter);
#pragma unroll
        for (int c = 0; c < 4; c++) b[c] ^= ks[c];
        gcm_store_block(out + pos, b, cnt);
#pragma unroll
        for (int c = 0; c < 4; c++) {  // as in gcm_seal: the hash takes the ciphertext zero-padded
            const int nb = (int)cnt - 4 * c;
            b[c] &= nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : ~(0xffffffffu >> (8 * nb)));
        }
        gcm.g.update(b);
    }
    uint32_t t[4];
    gcm_tag_aad(t, gcm, aad_blocks, len);
    gcm_store_block(out + len, t, 16);
}

// As gcm_open, under additional data: the tag is decided before the first plaintext byte is written
template <class RK, class Aad>
KYB_HD bool gcm_open_aad(uint8_t* out, const uint8_t* ct, uint64_t len, const uint32_t nonce[3], const RK& rk, const uint8_t* sbox,
                         Aad aad, int aad_blocks) {
    Gcm<RK> gcm(rk, sbox, nonce);
    gcm_hash_aad(gcm, aad, aad_blocks);
#pragma unroll 1
    for (uint64_t pos = 0; pos < len; pos += 16) {
        uint32_t b[4];
        gcm_load_block(b, ct + pos, len - pos < 16 ? (size_t)(len - pos) : 16);
        gcm.g.update(b);
    }
    uint32_t t[4], want[4];
    gcm_tag_aad(t, gcm, aad_blocks, len);
    gcm_load_block(want, ct + len, 16);
    const bool ok = ((t[0] ^ want[0]) | (t[1] ^ want[1]) | (t[2] ^ want[2]) | (t[3] ^ want[3])) == 0;
    uint32_t counter = 2;
#pragma unroll 1
    for (uint64_t pos = 0; pos < len; pos += 16, counter++) {
        const size_t cnt = len - pos < 16 ? (size_t)(len - pos) : 16;
        uint32_t b[4] = {0, 0, 0, 0}, ks[4];
        if (ok) {
            gcm_load_block(b, ct + pos, cnt);
            gcm.keystream(ks, counter);
#pragma unroll
            for (int c = 0; c < 4; c++) b[c] ^= ks[c];
        }
        gcm_store_block(out + pos, b, cnt);
    }
    return ok;
}

}  // namespace kyb
