// kyber_amd/csrc/ed25519_vss.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_vss_host.py runs the four lane programs -- batched schnorr.Sign, the deal's seal and open, Rabin's share
// check -- and their parts (GCM with additional data, the key derivation) through these entry points against the
// oracle (tests/_vss_oracle.py) and the fixtures.  The entry points take the arguments of the C ABI's host calls and lay
// memory out as the kernels do: a lane's window table in a TabGlobal slab, the encoder's bytes in front of it, round keys
// in the [word][lane] layout (a block of 64 lanes, this element in lane 5), H's tables parked one per polynomial behind
// the decoded commitments.  With -DVSS_HARNESS_MAIN the file is a stand-alone program over the same entry points, for a
// sanitizer build (tests/test_vss_harness_sanitizers.py).
#include "../kyber_amd/csrc/ed25519_vss.cuh"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace kyb;

static void words(uint32_t w[8], const uint8_t* p) { memcpy(w, p, 32); }  // little-endian host

static const sf::Mod& order() {
    static const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    return m;
}

// the rows of the standard base's wide comb that a scalar reads, built on demand with the device's row code
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

// the AEAD kernels' memory: a block's S-box and round-key columns; a lane's window table
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

extern "C" {
// out: len + 16 bytes.  aad: 16 * aad_blocks bytes.
void vsh_gcm_seal_aad(const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, int aad_blocks, const uint8_t* msg, size_t len,
                      uint8_t* out) {
    Lane l;
    uint32_t k[8], nw[3];
    std::vector<uint32_t> a(4 * aad_blocks + 1);
    be_words(k, key, 8);
    be_words(nw, nonce, 3);
    be_words(a.data(), aad, 4 * aad_blocks);
    aes256_expand(l.rk, k, l.sbox);
    const uint32_t* aw = a.data();
    gcm_seal_aad(out, msg, len, nw, l.rk, l.sbox, [aw](int i) { return aw[i]; }, aad_blocks);
}
// sealed: len + 16 bytes; out: len bytes.  1 when the tag is right.
int vsh_gcm_open_aad(const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, int aad_blocks, const uint8_t* sealed, size_t len,
                     uint8_t* out) {
    Lane l;
    uint32_t k[8], nw[3];
    std::vector<uint32_t> a(4 * aad_blocks + 1);
    be_words(k, key, 8);
    be_words(nw, nonce, 3);
    be_words(a.data(), aad, 4 * aad_blocks);
    aes256_expand(l.rk, k, l.sbox);
    const uint32_t* aw = a.data();
    return gcm_open_aad(out, sealed, len, nw, l.rk, l.sbox, [aw](int i) { return aw[i]; }, aad_blocks) ? 1 : 0;
}
// out = newAEAD's key: HKDF-SHA256(pre, nil, ctx)[0 .. 32) for a context of ctx_len bytes (a multiple of 4)
void vsh_kdf(const uint8_t* pre, const uint8_t* ctx, size_t ctx_len, uint8_t* out) {
    uint32_t pw[8], key[8];
    std::vector<uint32_t> cw(ctx_len / 4);  // exactly sized: a word read past the context is the sanitizer's to report
    words(pw, pre);
    memcpy(cw.data(), ctx, ctx_len);
    vss_kdf(key, pw, cw.data(), (int)(ctx_len / 4));
    for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(key[i] >> (24 - 8 * k));
}

// kyb_ed25519_schnorr_sign's value, element by element through the three passes.  status may be NULL.
void vsh_schnorr_sign(size_t n, const uint8_t* k, const uint8_t* privs, size_t priv_stride, const uint8_t* msgs, const uint64_t* off,
                      uint8_t* sigs, uint8_t* status) {
    std::vector<int32_t> proj(60);
    for (size_t i = 0; i < n; i++) {
        uint32_t kw[8], xw[8], rw[8], aw[8], sig[16];
        words(kw, k + 32 * i);
        words(xw, privs + i * priv_stride);
        need_comb_rows(kw);
        need_comb_rows(xw);
        ge_p3 R, A;
        ed_schnorr_points_lane(R, A, kw, xw, g_wide);
        store_proj(proj.data(), 0, R);
        store_proj(proj.data(), 1, A);
        ge_p3_towords(rw, R);
        ge_p3_towords(aw, A);
        ed_schnorr_sign_element(sig, rw, aw, kw, xw, msgs + off[i], (size_t)element_len(off, i), order());
        memcpy(sigs + 64 * i, sig, 64);
        if (status) status[i] = 0;
    }
}

// kyb_ed25519_vss_seal's value: cipher i at ciphers + off[i] + 16 i.  status may be NULL.
void vsh_vss_seal(size_t n, const uint8_t* dh, const uint8_t* k, const uint8_t* priv, const uint8_t* pub, const uint8_t* pubs,
                  const uint8_t* ctx, size_t ctx_stride, size_t ctx_len, const uint8_t* msgs, const uint64_t* off, uint8_t* dhkeys,
                  uint8_t* sigs, uint8_t* ciphers, uint8_t* status) {
    Lane l;
    std::vector<uint32_t> cw(ctx_len / 4);
    for (size_t i = 0; i < n; i++) {
        uint32_t dw[8], kw[8], pw[8], xw[8], aw[8], enc[24], dhkey[8], sig[16];
        words(dw, dh + 32 * i);
        words(kw, k + 32 * i);
        words(pw, pubs + 32 * i);
        words(xw, priv);
        words(aw, pub);
        memcpy(cw.data(), ctx + i * ctx_stride, ctx_len);
        need_comb_rows(dw);
        need_comb_rows(kw);
        TabGlobal tab{l.slab.data()};
        ge_p3 K, D, R;
        const int st = ed_vss_seal_lane(K, D, dw, pw, g_wide, tab);
        ed_vss_seal_nonce_point(R, kw, st, g_wide);
        ge_p3_towords(enc, K);
        ge_p3_towords(enc + 8, R);
        ge_p3_towords(enc + 16, D);
        memcpy(l.slab.data(), enc, 96);  // the encoder's bytes over the front of the table, read back from there
        memcpy(enc, l.slab.data(), 96);
        ed_vss_seal_element(ciphers + off[i] + VSS_OVERHEAD * i, dhkey, sig, msgs + off[i], element_len(off, i), enc, kw, xw, aw, cw.data(),
                            (int)(ctx_len / 4), st, order(), l.rk, l.sbox);
        memcpy(dhkeys + 32 * i, dhkey, 32);
        memcpy(sigs + 64 * i, sig, 64);
        if (status) status[i] = (uint8_t)st;
    }
}

// kyb_ed25519_vss_open's value: out is as large as the ciphers.  status may be NULL.
void vsh_vss_open(size_t n, const uint8_t* privs, size_t priv_stride, const uint8_t* dhkeys, const uint8_t* ctx, size_t ctx_stride,
                  size_t ctx_len, const uint8_t* ciphers, const uint64_t* off, uint8_t* out, uint8_t* status) {
    Lane l;
    std::vector<uint32_t> cw(ctx_len / 4);
    for (size_t i = 0; i < n; i++) {
        uint32_t xw[8], kw[8], pre[8];
        words(xw, privs + i * priv_stride);
        words(kw, dhkeys + 32 * i);
        memcpy(cw.data(), ctx + i * ctx_stride, ctx_len);
        TabGlobal tab{l.slab.data()};
        ge_p3 D;
        int st = ed_vss_open_lane(D, xw, kw, element_len(off, i), tab);
        ge_p3_towords(pre, D);
        st = ed_vss_open_element(out + off[i], ciphers + off[i], element_len(off, i), pre, cw.data(), (int)(ctx_len / 4), st, l.rk, l.sbox);
        if (status) status[i] = (uint8_t)st;
    }
}

// kyb_ed25519_deal_check2's value; a check that names no polynomial of the table gives 0 (the _dev rule).  status (m
// entries) may be NULL.
void vsh_deal_check2(size_t n, const uint32_t* poly, const uint32_t* idx, const uint8_t* f, const uint8_t* g, size_t m, size_t t,
                     const uint8_t* commits, const uint8_t* H, size_t h_stride, uint8_t* ok, uint8_t* status) {
    const size_t nh = m ? (h_stride ? m : 1) : 0;
    std::vector<ge_precomp> aff(m * t ? m * t : 1);
    std::vector<int4> htab(80 * (nh ? nh : 1));
    std::vector<uint8_t> bad(m ? m : 1, 0);
    if (status) memset(status, 0, m);
    for (size_t j = 0; j < m * t; j++) {
        uint32_t w[8];
        words(w, commits + 32 * j);
        if (!ed_deal_decode(aff[j], w)) bad[j / t] = 1;
    }
    for (size_t k = 0; k < nh; k++) {
        uint32_t w[8];
        words(w, H + 32 * k);
        TabGlobal tab{htab.data() + 80 * k};
        if (ed_vss_htab(tab, w)) continue;
        for (size_t p = nh == 1 ? 0 : k; p < (nh == 1 ? m : k + 1); p++) bad[p] = 1;
    }
    for (size_t k = 0; k < m; k++)
        if (bad[k] && status) status[k] = ED_DKG_ST_BAD_POINT;
    for (size_t i = 0; i < n; i++) {
        const size_t k = poly[i];
        if (k >= m || bad[k]) {
            ok[i] = 0;
            continue;
        }
        uint32_t fw[8], gw[8];
        words(fw, f + 32 * i);
        words(gw, g + 32 * i);
        need_comb_rows(fw);
        const TabGlobal tab{htab.data() + 80 * (h_stride ? k : 0)};
        ok[i] = ed_deal_check2_lane(fw, gw, aff.data() + k * t, t, idx[i], g_wide, tab) ? 1 : 0;
    }
}
}

#ifdef VSS_HARNESS_MAIN
// Every entry over exactly sized heap buffers: the last message and the last cipher end their buffers, an odd byte
// offset stands in front of the first element and the first element is empty.  Values are checked by
// tests/test_vss_host.py; this program is for the sanitizers, and checks only that what it sealed opens again.
static uint8_t* filled(size_t bytes, uint32_t& seed) {
    uint8_t* p = new uint8_t[bytes ? bytes : 1];
    for (size_t i = 0; i < bytes; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
static void undecodable(uint8_t* out) {  // the smallest y >= 2 with no x
    memset(out, 0, 32);
    for (out[0] = 2;; out[0]++) {
        uint32_t w[8];
        words(w, out);
        ge_p3 P;
        if (!ge_p3_fromwords(P, w)) return;
    }
}
int main() {
    static const size_t LENGTHS[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 109, 1069};
    const size_t n = sizeof(LENGTHS) / sizeof(LENGTHS[0]);
    uint32_t seed = 23;
    int bad = 0;
    for (size_t shape = 0; shape < 4; shape++) {  // a context of 32 or 128 bytes, one for the batch or one per element
        const size_t clen = shape < 2 ? 32 : 128, stride = shape % 2 ? clen : 0;
        uint64_t off[n + 1], coff[n + 1];
        off[0] = 3;  // an odd byte offset in front of the first element, which is empty
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + LENGTHS[i];
        for (size_t i = 0; i <= n; i++) coff[i] = off[i] + 16 * i;
        uint8_t* msgs = filled((size_t)off[n], seed);
        uint8_t *dh = filled(32 * n, seed), *k = filled(32 * n, seed), *x = filled(32 * n, seed), *priv = filled(32, seed);
        uint8_t* ctx = filled(stride ? clen * n : clen, seed);
        uint8_t *pubs = new uint8_t[32 * n], *pub = new uint8_t[32];
        for (size_t i = 0; i < n; i++) {  // pubs_i = x_i B, pub = priv B, through the harness's own comb
            uint32_t xw[8], w[8];
            words(xw, x + 32 * i);
            need_comb_rows(xw);
            int8_t e[65];
            recode16(e, xw, false);
            ge_p3 P;
            ed_comb_mul_base(P, e, g_wide);
            ge_p3_towords(w, P);
            memcpy(pubs + 32 * i, w, 32);
        }
        {
            uint8_t* sig = new uint8_t[64];
            const uint64_t o2[2] = {0, 0};
            uint8_t none[1];
            vsh_schnorr_sign(1, priv, priv, 32, none, o2, sig, nullptr);  // (only to have the rows of priv built)
            uint32_t xw[8], w[8];
            words(xw, priv);
            int8_t e[65];
            recode16(e, xw, false);
            ge_p3 P;
            ed_comb_mul_base(P, e, g_wide);
            ge_p3_towords(w, P);
            memcpy(pub, w, 32);
            delete[] sig;
        }
        undecodable(pubs + 32 * 4);  // a planted reject
        uint8_t *dhkeys = new uint8_t[32 * n], *sigs = new uint8_t[64 * n], *ciphers = new uint8_t[(size_t)coff[n]], *st = new uint8_t[n];
        uint8_t* back = new uint8_t[(size_t)coff[n]];
        vsh_vss_seal(n, dh, k, priv, pub, pubs, ctx, stride, clen, msgs, off, dhkeys, sigs, ciphers, st);
        vsh_vss_seal(n, dh, k, priv, pub, pubs, ctx, stride, clen, msgs, off, dhkeys, sigs, ciphers, nullptr);
        for (size_t i = 0; i < n; i++) bad |= st[i] != (i == 4 ? 1 : 0);
        vsh_vss_open(n, x, 32, dhkeys, ctx, stride, clen, ciphers, coff, back, st);
        for (size_t i = 0; i < n; i++) {
            if (i == 4) {
                bad |= st[i] == 0;
                continue;
            }
            bad |= st[i] != 0;
            bad |= LENGTHS[i] && memcmp(back + coff[i], msgs + off[i], LENGTHS[i]) != 0;
            for (size_t b = LENGTHS[i]; b < LENGTHS[i] + 16; b++) bad |= back[coff[i] + b] != 0;
        }
        ciphers[coff[n] - 1] ^= 1;  // the last tag byte, the last byte of its buffer
        vsh_vss_open(n, x, 32, dhkeys, ctx, stride, clen, ciphers, coff, back, st);
        bad |= st[n - 1] != ED_ST_ECIES_AUTH;
        {   // ciphers shorter than a tag, the last one ending the buffer
            const uint64_t so[4] = {0, 0, 15, 30};
            uint8_t *sc = filled(30, seed), *so_out = new uint8_t[30], sst[3];
            vsh_vss_open(3, x, 0, dhkeys, ctx, stride, clen, sc, so, so_out, sst);
            bad |= sst[0] != ED_ST_ECIES_SHORT || sst[1] != ED_ST_ECIES_SHORT || sst[2] != ED_ST_ECIES_SHORT;
            delete[] sc; delete[] so_out;
        }
        // signatures over the same messages: one signer and one per element
        vsh_schnorr_sign(n, k, x, 32, msgs, off, sigs, st);
        vsh_schnorr_sign(n, k, priv, 0, msgs, off, sigs, nullptr);
        delete[] msgs; delete[] dh; delete[] k; delete[] x; delete[] priv; delete[] ctx; delete[] pubs; delete[] pub;
        delete[] dhkeys; delete[] sigs; delete[] ciphers; delete[] st; delete[] back;
    }
    for (size_t hs = 0; hs <= 32; hs += 32)
        for (size_t t = 0; t <= 3; t++) {
            const size_t m = 3, nchk = 5;
            uint8_t* commits = new uint8_t[32 * m * t ? 32 * m * t : 1];
            uint8_t* H = new uint8_t[hs ? 32 * m : 32];
            for (size_t j = 0; j < m * t; j++) {
                memset(commits + 32 * j, 0, 32);
                commits[32 * j] = (uint8_t)(3 + j);
            }
            for (size_t j = 0; j < (hs ? m : 1); j++) {  // the identity, a y without x, a small y
                memset(H + 32 * j, 0, 32);
                H[32 * j] = (uint8_t)(1 + 3 * j);
                if (j == 1) undecodable(H + 32 * j);
            }
            uint32_t poly[nchk] = {0, 1, 2, 7, 2}, idx[nchk] = {0, 1, 0xffffffffu, 3, 16};
            uint8_t *f = filled(32 * nchk, seed), *g = filled(32 * nchk, seed), *ok = new uint8_t[nchk], *pst = new uint8_t[m];
            memset(g, 0xff, 32);
            vsh_deal_check2(nchk, poly, idx, f, g, m, t, commits, H, hs, ok, pst);
            vsh_deal_check2(nchk, poly, idx, f, g, m, t, commits, H, hs, ok, nullptr);
            bad |= ok[3] != 0;
            delete[] commits; delete[] H; delete[] f; delete[] g; delete[] ok; delete[] pst;
        }
    free(g_wide);
    puts(bad ? "FAILED" : "ok");
    return bad;
}
#endif
