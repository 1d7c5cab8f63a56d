// kyber_amd/csrc/aes256gcm.cuh and ed25519_dkg.cuh compiled for the CPU (test infrastructure, never linked into
// libkyberhip.so): tests/test_ecies_host.py runs the cipher, the key schedule, GCM, the HKDF, the ECIES lane programs
// with their AEAD pass and the deal-check lane program through these entry points against the fixtures, hashlib and the
// big-integer oracle.  Window tables live in a TabGlobal slab and round keys in the [word][lane] layout of the kernels
// (a block of 64 lanes, this element in lane 5); the rows of the standard base's wide comb that a scalar reads are built
// on demand with the row code of the device's table kernel (ed_comb_row).  With -DDKG_HARNESS_MAIN the file is a
// stand-alone program over the same entry points, for a sanitizer build (tests/test_dkg_harness_sanitizers.py).
#include "../kyber_amd/csrc/ed25519_dkg.cuh"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace kyb;

static void words(uint32_t w[8], const uint8_t* p) { memcpy(w, p, 32); }  // little-endian host

static int32_t* g_wide = nullptr;
static std::vector<bool> g_have;
static void need_comb_rows(const uint32_t sw[8]) {
    if (!g_wide) {
        g_wide = (int32_t*)calloc(ED_WIDE_WORDS, sizeof(int32_t));
        g_have.assign(EdWide::ROWS, false);
    }
    ge_p3 B;
    B.X = fe_bx(); B.Y = fe_by(); fe_1(B.Z); B.T = fe_bt();
    int8_t e[65];
    recode16(e, sw, false);
    for (int k = 0; k < EdWide::POS_CT; k++) {
        int d = 0;
        for (int i = ED_COMB_G - 1; i >= 0; i--)
            if (ED_COMB_G * k + i < 64) d = 16 * d + (int)e[ED_COMB_G * k + i];
        if (d == 0) continue;
        const int t = k * EdWide::ENT + (d < 0 ? -d : d) - 1;
        if (g_have[t]) continue;
        ed_comb_row<ED_COMB_G>(g_wide + (size_t)t * ED_TAB_STRIDE, t, B);
        g_have[t] = true;
    }
}

// the kernels' memory: a block's S-box and round-key columns, one lane's window table
struct Lane {
    uint8_t sbox[256];
    std::vector<uint32_t> keys;
    std::vector<int4> slab;
    AesKeysLds<64> rk;
    Lane() : keys(AesKeysLds<64>::WORDS), slab(80), rk{nullptr} {
        for (int t = 0; t < 64; t++) aes_fill_sbox(sbox, t, 64);  // as 64 lanes fill it
        rk.col = keys.data() + 5;
    }
};

static void be_words(uint32_t* w, const uint8_t* p, int n) {
    for (int i = 0; i < n; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
}
static void be_bytes(uint8_t* p, const uint32_t* w, int n) {
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 4; k++) p[4 * i + k] = (uint8_t)(w[i] >> (24 - 8 * k));
}

extern "C" {
void dkg_sbox(uint8_t* out) {
    Lane l;
    memcpy(out, l.sbox, 256);
}
// out = the 60 round-key words (240 bytes), through the LDS layout and through the plain one: both must agree
int dkg_aes_expand(const uint8_t* key, uint8_t* out) {
    Lane l;
    uint32_t k[8], w[60];
    be_words(k, key, 8);
    aes256_expand(l.rk, k, l.sbox);
    AesKeysLocal loc;
    aes256_expand(loc, k, l.sbox);
    int same = 1;
    for (int i = 0; i < 60; i++) {
        w[i] = l.rk.get(i);
        same &= w[i] == loc.get(i);
    }
    be_bytes(out, w, 60);
    return same;
}
void dkg_aes_block(const uint8_t* key, const uint8_t* in, uint8_t* out) {
    Lane l;
    uint32_t k[8], b[4], o[4];
    be_words(k, key, 8);
    be_words(b, in, 4);
    aes256_expand(l.rk, k, l.sbox);
    aes256_encrypt(o, b, l.rk, l.sbox);
    be_bytes(out, o, 4);
}
// out: len + 16 bytes
void dkg_gcm_seal(const uint8_t* key, const uint8_t* nonce, const uint8_t* msg, size_t len, uint8_t* out) {
    Lane l;
    uint32_t k[8], nw[3];
    be_words(k, key, 8);
    be_words(nw, nonce, 3);
    aes256_expand(l.rk, k, l.sbox);
    gcm_seal(out, msg, len, nw, l.rk, l.sbox);
}
// sealed: len + 16 bytes; out: len bytes.  1 when the tag is right.
int dkg_gcm_open(const uint8_t* key, const uint8_t* nonce, const uint8_t* sealed, size_t len, uint8_t* out) {
    Lane l;
    uint32_t k[8], nw[3];
    be_words(k, key, 8);
    be_words(nw, nonce, 3);
    aes256_expand(l.rk, k, l.sbox);
    return gcm_open(out, sealed, len, nw, l.rk, l.sbox) ? 1 : 0;
}
// out = HKDF-SHA256(secret (n <= 32 bytes), no salt, no info)[0 .. 64)
void dkg_hkdf(const uint8_t* secret, int n, uint8_t* out) {
    uint8_t padded[32] = {0};
    memcpy(padded, secret, (size_t)n);
    uint32_t s[8], okm[16];
    be_words(s, padded, 8);
    hkdf_sha256_64(okm, s, n);
    be_bytes(out, okm, 16);
}
// the seal kernels' three passes for one element: out = len + 48 bytes; returns the status
int dkg_ecies_seal(const uint8_t* r, const uint8_t* pub, const uint8_t* msg, size_t len, uint8_t* out) {
    Lane l;
    uint32_t rw[8], pw[8], Rw[8], dh[8];
    words(rw, r);
    words(pw, pub);
    need_comb_rows(rw);
    TabGlobal tab{l.slab.data()};
    ge_p3 R, D;
    const int st = ed_ecies_seal_lane(R, D, rw, pw, g_wide, tab);
    ge_p3_towords(Rw, R);
    ge_p3_towords(dh, D);
    ed_ecies_seal_element(out, msg, len, Rw, dh, st, l.rk, l.sbox);
    return st;
}
// the open kernels' three passes for one element of len bytes: out = len bytes; returns the status
int dkg_ecies_open(const uint8_t* priv, const uint8_t* ct, size_t len, uint8_t* out) {
    Lane l;
    uint32_t xw[8], dh[8];
    words(xw, priv);
    TabGlobal tab{l.slab.data()};
    ge_p3 D;
    const int st = ed_ecies_open_lane(D, xw, ct, len, tab);
    ge_p3_towords(dh, D);
    return ed_ecies_open_element(out, ct, len, dh, st, l.rk, l.sbox);
}
// the deal kernels for one check of a polynomial of t commitments: 1 / 0, or -1 when a commitment does not decode
int dkg_deal_check(const uint8_t* share, uint32_t idx, size_t t, const uint8_t* commits) {
    std::vector<ge_precomp> aff(t ? t : 1);
    bool good = true;
    for (size_t j = 0; j < t; j++) {
        uint32_t w[8];
        words(w, commits + 32 * j);
        good &= ed_deal_decode(aff[j], w);
    }
    if (!good) return -1;
    uint32_t sw[8];
    words(sw, share);
    need_comb_rows(sw);
    return ed_deal_check_lane(sw, aff.data(), t, idx, g_wide) ? 1 : 0;
}
}

#ifdef DKG_HARNESS_MAIN
// Every length of the tests through seal, open and the tampered opens, with exactly sized heap buffers: a byte read or
// written past an element is the sanitizer's to report.  Prints "ok" and returns 0 when every round trip held.
int main() {
    static const size_t LENGTHS[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 255, 256, 257, 1000};
    uint8_t r[32], x[32], pub[32];
    for (int i = 0; i < 32; i++) {
        r[i] = (uint8_t)(7 * i + 3);
        x[i] = (uint8_t)(11 * i + 5);
    }
    r[31] &= 0x0f;
    x[31] &= 0x0f;
    {   // pub = x B, through the harness's own comb
        uint32_t xw[8], w[8];
        words(xw, x);
        need_comb_rows(xw);
        int8_t e[65];
        recode16(e, xw, false);
        ge_p3 P;
        ed_comb_mul_base(P, e, g_wide);
        ge_p3_towords(w, P);
        memcpy(pub, w, 32);
    }
    int bad = 0;
    for (size_t len : LENGTHS) {
        std::vector<uint8_t> msg(len), ct(len + 48), back(len + 48);
        for (size_t i = 0; i < len; i++) msg[i] = (uint8_t)(i * 31 + len);
        bad |= dkg_ecies_seal(r, pub, msg.data(), len, ct.data()) != 0;
        bad |= dkg_ecies_open(x, ct.data(), len + 48, back.data()) != 0;
        bad |= len && memcmp(back.data(), msg.data(), len) != 0;
        for (size_t at : {(size_t)32, len + 31, len + 47}) {  // first and last ciphertext byte, last tag byte
            if (len == 0 && at != 47) continue;                  // (an empty message has no ciphertext byte: its tag alone)
            std::vector<uint8_t> t(ct);
            t[at] ^= 1;
            bad |= dkg_ecies_open(x, t.data(), len + 48, back.data()) != ED_ST_ECIES_AUTH;
            for (size_t i = 0; i < len + 48; i++) bad |= back[i] != 0;
        }
        // the plain GCM entry points on exactly sized buffers
        std::vector<uint8_t> sealed(len + 16), plain(len);
        dkg_gcm_seal(r, x, msg.data(), len, sealed.data());
        bad |= dkg_gcm_open(r, x, sealed.data(), len, plain.data()) != 1;
        bad |= len && memcmp(plain.data(), msg.data(), len) != 0;
    }
    for (size_t len : {(size_t)0, (size_t)31, (size_t)32, (size_t)47}) {
        std::vector<uint8_t> ct(len, 0x5a), out(len, 0xff);
        bad |= dkg_ecies_open(x, ct.data(), len, out.data()) != ED_ST_ECIES_SHORT;
        for (size_t i = 0; i < len; i++) bad |= out[i] != 0;
    }
    {   // a deal check: the polynomial (B, B, B) at index 1 (x = 2) is 7 B
        uint8_t commits[96], share[32] = {7};
        uint8_t one[32] = {1};
        uint32_t ow[8], w[8];
        words(ow, one);
        need_comb_rows(ow);
        int8_t e[65];
        recode16(e, ow, false);
        ge_p3 P;
        ed_comb_mul_base(P, e, g_wide);
        ge_p3_towords(w, P);
        for (int j = 0; j < 3; j++) memcpy(commits + 32 * j, w, 32);
        bad |= dkg_deal_check(share, 1, 3, commits) != 1;
        share[0] = 8;
        bad |= dkg_deal_check(share, 1, 3, commits) != 0;
    }
    free(g_wide);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
