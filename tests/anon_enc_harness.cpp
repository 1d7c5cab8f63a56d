// kyber_amd/csrc/ed25519_anonenc.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_anon_enc_host.py runs sign/anon's seal and open and their parts -- the 32-byte stream, the keystream, the
// MAC -- through these entry points against the oracle (tests/_anon_enc_oracle.py) and the two ciphertexts the reference
// prints.  The entry points take the arguments of the C ABI's host calls and lay memory out as the kernels do: an
// element's ring + 1 lanes side by side, a lane's window table in a TabGlobal slab, its parked point, its 16 words; the
// shared set's tables built once; the passes in the kernels' order over the whole batch, the encodings through the
// shared-inversion encoder with the kernels' block geometry.  With -DANON_ENC_HARNESS_MAIN the file is a stand-alone
// program over the same entry points, for a sanitizer build (tests/test_anon_enc_harness_sanitizers.py).
#include "../kyber_amd/csrc/ed25519_anonenc.cuh"

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

// a call's memory: the slab of n elements of ring + 1 lanes, exactly sized, and the shared set's workspace
struct Slab {
    size_t ring, lanes;
    std::vector<int4> gtab, shared;
    std::vector<int32_t> proj;
    std::vector<uint32_t> lane_words;
    std::vector<uint8_t> st;
    uint8_t shared_bad = 0;
    Slab(size_t n, size_t r) : ring(r), lanes(n * (r + 1)), gtab(80 * lanes), proj(30 * lanes), lane_words(16 * lanes), st(n ? n : 1) {}
    void tables(const uint8_t* keys) {  // ed25519_anon_tables_kernel
        shared.resize(80 * ring);
        for (size_t k = 0; k < ring; k++) {
            uint32_t w[8];
            words(w, keys + 32 * k);
            if (!ed_anon_table(shared.data() + 80 * k, w)) shared_bad = 1;
        }
    }
    // ed25519_anon_points_kernel: scal(e) gives element e's scalar words
    template <class Scal>
    void points(const uint8_t* keys, size_t key_stride, Scal scal) {
        for (size_t j = 0; j < lanes; j++) {
            const size_t e = j / (ring + 1), k = j % (ring + 1);
            if (k == 0) continue;
            if (!key_stride && shared_bad && st[e] == 0) st[e] = ED_DKG_ST_BAD_POINT;
            ge29_p3 S;
            if (st[e] != 0) {
                ge_p3_0(S);
                store_proj(proj.data(), j, S);
                continue;
            }
            uint32_t sw[8];
            scal(sw, e);
            if (!key_stride) {
                ed_anon_product_shared(S, sw, shared.data() + 80 * (k - 1));
            } else {
                uint32_t yw[8];
                words(yw, keys + e * key_stride + 32 * (k - 1));
                if (!ed_anon_product_own(S, sw, yw, gtab.data() + 80 * j)) st[e] = ED_DKG_ST_BAD_POINT;
            }
            store_proj(proj.data(), j, S);
        }
    }
    void encode() {  // ed25519_anon_encode_kernel: blocks of 64 lanes, ENC_CHUNK points a lane, interleaved
        const size_t span = 64 * (size_t)ENC_CHUNK;
        for (size_t b = 0; b * span < lanes; b++)
            for (size_t t = 0; t < 64; t++) {
                EncPreScratch pre;
                ed_encode_chunk(lanes, proj.data(), b * span + t, 64, pre,
                                [&](size_t i, uint32_t(&w)[8]) { memcpy(lane_words.data() + 16 * i, w, 32); });
            }
    }
    const uint32_t* xb(size_t e) const { return lane_words.data() + e * (ring + 1) * 16 + 8; }
};

extern "C" {
void aeh_stream32(const uint8_t* seed, uint8_t* out) {
    uint32_t s[8], ks[8];
    words(s, seed);
    ed_anon_stream32(ks, s);
    memcpy(out, ks, 32);
}
void aeh_xor_stream(uint8_t* dst, const uint8_t* src, size_t len, const uint8_t* xb) {
    uint32_t k[8];
    words(k, xb);
    ed_anon_xor_stream(dst, src, len, k);
}
void aeh_mac(const uint8_t* ctx, size_t len, uint8_t* out) {
    uint32_t mac[4];
    ed_anon_mac(mac, ctx, len);
    memcpy(out, mac, 16);
}
void aeh_reduce(const uint8_t* x, uint8_t* out) {
    uint32_t xw[8], r[8];
    words(xw, x);
    ed_anon_reduce(r, xw, order());
    memcpy(out, r, 32);
}

// kyb_ed25519_anon_seal's value: ciphertext i at out + off[i] + i (48 + 32 ring).  status may be NULL.
void aeh_anon_seal(size_t n, size_t ring, const uint8_t* keys, size_t key_stride, const uint8_t* x, const uint8_t* msgs,
                   const uint64_t* off, uint8_t* out, uint8_t* status) {
    Slab w(n, ring);
    if (!key_stride) w.tables(keys);
    for (size_t e = 0; e < n; e++) {  // ed25519_anon_seal_head_kernel
        uint32_t xw[8], xb[8];
        words(xw, x + 32 * e);
        need_comb_rows(xw);
        ge_p3 X;
        ed_anon_seal_head(X, xb, xw, g_wide, order());
        store_proj(w.proj.data(), e * (ring + 1), X);
        memcpy(w.lane_words.data() + e * (ring + 1) * 16 + 8, xb, 32);
        w.st[e] = w.shared_bad ? ED_DKG_ST_BAD_POINT : 0;
    }
    w.points(keys, key_stride, [&](uint32_t(&sw)[8], size_t e) { words(sw, x + 32 * e); });
    w.encode();
    for (size_t j = 0; j < w.lanes; j++) {  // ed25519_anon_slot_kernel<false>
        const size_t e = j / (ring + 1), k = j % (ring + 1);
        uint8_t* at = out + off[e] + e * anon_overhead(ring) + 32 * k;
        uint32_t enc[8], s[8];
        memcpy(enc, w.lane_words.data() + 16 * j, 32);
        if (k == 0)
            memcpy(s, enc, 32);
        else
            ed_anon_slot(s, enc, w.xb(e));
        if (w.st[e]) memset(s, 0, 32);
        ed_anon_store32(at, s);
    }
    for (size_t e = 0; e < n; e++) {  // ed25519_anon_body_kernel<false>
        ed_anon_seal_body(out + off[e] + e * anon_overhead(ring) + 32 + 32 * ring, msgs + off[e], element_len(off, e), w.xb(e), w.st[e]);
        if (status) status[e] = w.st[e];
    }
}

// kyb_ed25519_anon_open's value: out is as large as the ciphertexts.  mine is taken modulo ring (the _dev rule).
void aeh_anon_open(size_t n, size_t ring, const uint8_t* keys, size_t key_stride, const uint32_t* mine, const uint8_t* privs,
                   size_t priv_stride, const uint8_t* cts, const uint64_t* off, uint8_t* out, uint8_t* status) {
    Slab w(n, ring);
    if (!key_stride) w.tables(keys);
    for (size_t e = 0; e < n; e++) {  // ed25519_anon_open_head_kernel
        uint32_t pw[8], xb[8];
        words(pw, privs + e * priv_stride);
        const size_t j = e * (ring + 1);
        Tab29 tab{w.gtab.data() + 80 * j};
        // (the comb rows of xb are known only inside the head: build those of every scalar it can meet first)
        ge_p3 XB;
        struct Rows {
            static void of(const uint8_t* ct, uint64_t len, size_t ring, size_t mine, const uint32_t pw[8], std::vector<int4>& scratch) {
                if (len < 32 + 32 * (uint64_t)ring) return;
                uint32_t xw[8], sw[8], slot[8], xb[8];
                ed_anon_load32(xw, ct);
                ge29_p3 A, S;
                if (!ge_p3_fromwords(A, xw)) return;
                int8_t e[65];
                recode16(e, pw, false);
                Tab29 t{scratch.data()};
                ge_scalarmult_w4<false, true>(S, e, A, false, t, 63);
                ge_p3_towords(sw, S);
                ed_anon_load32(slot, ct + 32 + 32 * mine);
                ed_anon_slot(xb, sw, slot);
                need_comb_rows(xb);
            }
        };
        std::vector<int4> scratch(80);
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        need_comb_rows(zero);
        Rows::of(cts + off[e], element_len(off, e), ring, mine[e] % ring, pw, scratch);
        const int s = ed_anon_open_head(XB, xb, pw, cts + off[e], element_len(off, e), ring, mine[e] % ring, g_wide, tab);
        store_proj(w.proj.data(), j, XB);
        memcpy(w.lane_words.data() + j * 16 + 8, xb, 32);
        w.st[e] = (uint8_t)s;
    }
    w.points(keys, key_stride, [&](uint32_t(&sw)[8], size_t e) { memcpy(sw, w.xb(e), 32); });
    w.encode();
    for (size_t j = 0; j < w.lanes; j++) {  // ed25519_anon_slot_kernel<true>
        const size_t e = j / (ring + 1), k = j % (ring + 1);
        if (w.st[e]) continue;
        const uint8_t* at = cts + off[e] + 32 * k;
        uint32_t enc[8], s[8], have[8];
        memcpy(enc, w.lane_words.data() + 16 * j, 32);
        ed_anon_load32(have, at);
        if (k == 0) {
            ed_canon_point_bytes(s, have);
            if (!ed_words8_equal(s, enc)) w.st[e] = ED_ST_ANON_INVALID;
        } else {
            ed_anon_slot(s, enc, w.xb(e));
            if (!ed_words8_equal(s, have)) w.st[e] = ED_ST_ANON_INVALID;
        }
    }
    for (size_t e = 0; e < n; e++) {  // ed25519_anon_body_kernel<true>
        const int s = ed_anon_open_body(out + off[e], cts + off[e], element_len(off, e), 32 + 32 * (uint64_t)ring, w.xb(e), w.st[e]);
        if (status) status[e] = (uint8_t)s;
    }
}
}

#ifdef ANON_ENC_HARNESS_MAIN
// Both entries over exactly sized heap buffers: every message length of the keystream's and the MAC's block edges, an
// odd byte offset in front of an empty first element, the last message and the last ciphertext ending their buffers,
// ciphertexts cut at every boundary of Decrypt's length checks, both values of each stride.  Values are checked by
// tests/test_anon_enc_host.py; this program is for the sanitizers, and checks only that what it sealed opens again and
// that a cut ciphertext is refused.
static uint8_t* filled(size_t bytes, uint32_t& seed) {
    uint8_t* p = new uint8_t[bytes ? bytes : 1];
    for (size_t i = 0; i < bytes; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
static void base_mul(uint8_t* out, const uint8_t* x) {
    uint32_t xw[8], w[8];
    words(xw, x);
    need_comb_rows(xw);
    int8_t e[65];
    recode16(e, xw, false);
    ge_p3 P;
    ed_comb_mul_base(P, e, g_wide);
    ge_p3_towords(w, P);
    memcpy(out, w, 32);
}
int main() {
    static const size_t LENGTHS[] = {0, 1, 12, 63, 64, 65, 127, 128, 129, 191, 192, 193, 320, 321};
    const size_t n = sizeof(LENGTHS) / sizeof(LENGTHS[0]), ring = 3;
    const size_t over = anon_overhead(ring), hdr = 32 + 32 * ring;
    uint32_t seed = 29;
    int bad = 0;
    for (size_t shape = 0; shape < 4; shape++) {  // one set or one per element; one receiver or one per element
        const size_t key_stride = shape & 1 ? 32 * ring : 0, priv_stride = shape & 2 ? 32 : 0;
        uint64_t off[n + 1], coff[n + 1];
        off[0] = 3;  // an odd byte offset in front of the first element, which is empty
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + LENGTHS[i];
        for (size_t i = 0; i <= n; i++) coff[i] = off[i] + over * i;
        uint8_t* msgs = filled((size_t)off[n], seed);
        uint8_t *x = filled(32 * n, seed), *privs = filled(priv_stride ? 32 * n : 32, seed);
        for (size_t i = 0; i < n; i++) x[32 * i + 31] &= 0x7f;
        const size_t sets = key_stride ? n : 1;
        uint8_t* keys = filled(32 * ring * sets, seed);
        uint32_t* mine = new uint32_t[n];
        for (size_t i = 0; i < n; i++) mine[i] = (uint32_t)(i % ring);
        for (size_t k = 0; k < ring * sets; k++) {  // every member a real key
            uint8_t* sk = filled(32, seed);
            base_mul(keys + 32 * k, sk);
            delete[] sk;
        }
        for (size_t i = 0; i < n; i++)  // receiver i's key at its position of its set (a later one may take the place)
            base_mul(keys + 32 * (ring * (key_stride ? i : 0) + mine[i]), privs + (priv_stride ? 32 * i : 0));
        // with one shared set and a key per element only the last receiver of a position finds its own key there:
        // valid[i] says where this shape's keys line up, and the others must be refused
        bool* valid = new bool[n];
        for (size_t i = 0; i < n; i++) {
            uint8_t pub[32];
            base_mul(pub, privs + (priv_stride ? 32 * i : 0));
            valid[i] = memcmp(pub, keys + 32 * (ring * (key_stride ? i : 0) + mine[i]), 32) == 0;
        }
        uint8_t *cts = new uint8_t[(size_t)coff[n]], *st = new uint8_t[n], *back = new uint8_t[(size_t)coff[n]];
        aeh_anon_seal(n, ring, keys, key_stride, x, msgs, off, cts, st);
        aeh_anon_seal(n, ring, keys, key_stride, x, msgs, off, cts, nullptr);
        for (size_t i = 0; i < n; i++) bad |= st[i] != 0;
        aeh_anon_open(n, ring, keys, key_stride, mine, privs, priv_stride, cts, coff, back, st);
        for (size_t i = 0; i < n; i++) {
            if (!valid[i]) {
                bad |= st[i] != ED_ST_ANON_INVALID;
                continue;
            }
            bad |= st[i] != 0;
            bad |= LENGTHS[i] && memcmp(back + coff[i], msgs + off[i], LENGTHS[i]) != 0;
            for (size_t b = LENGTHS[i]; b < LENGTHS[i] + over; b++) bad |= back[coff[i] + b] != 0;
        }
        cts[coff[n] - 1] ^= 1;  // the last MAC byte, the last byte of its buffer
        aeh_anon_open(n, ring, keys, key_stride, mine, privs, priv_stride, cts, coff, back, nullptr);
        aeh_anon_open(n, ring, keys, key_stride, mine, privs, priv_stride, cts, coff, back, st);
        bad |= valid[n - 1] && st[n - 1] != ED_ST_ANON_MAC;
        {   // the first valid ciphertext cut at every boundary, each cut a buffer of its own that it ends
            size_t v = 0;
            while (v < n && !valid[v]) v++;
            static const size_t CUTS[] = {0, 31, 32, hdr - 1, hdr, hdr + 15, hdr + 16};
            for (size_t c = 0; v < n && c < sizeof(CUTS) / sizeof(CUTS[0]); c++) {
                uint8_t *cut = new uint8_t[CUTS[c] ? CUTS[c] : 1], *o = new uint8_t[CUTS[c] ? CUTS[c] : 1], s1;
                memcpy(cut, cts + coff[v], CUTS[c]);
                const uint64_t co[2] = {0, CUTS[c]};
                aeh_anon_open(1, ring, keys + (key_stride ? key_stride * v : 0), key_stride, mine + v, privs + (priv_stride ? 32 * v : 0),
                              priv_stride, cut, co, o, &s1);
                // (cut behind the header and 16 bytes: an empty message's whole ciphertext, or a MAC that cannot match)
                const int want = CUTS[c] < hdr + 16 ? ED_ST_ANON_SHORT : (LENGTHS[v] ? ED_ST_ANON_MAC : 0);
                bad |= s1 != want;
                delete[] cut; delete[] o;
            }
        }
        delete[] msgs; delete[] x; delete[] privs; delete[] keys; delete[] mine; delete[] valid; delete[] cts; delete[] st; delete[] back;
    }
    free(g_wide);
    puts(bad ? "FAILED" : "ok");
    return bad;
}
#endif
