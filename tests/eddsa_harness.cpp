// kyber_amd/csrc/ed25519_eddsa.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_eddsa_host.py runs the lane programs -- the key expansion, the nonce pass, the sign pass -- through these
// entry points against the oracle (tests/_eddsa_oracle.py) and the reference's sign.input.  The entry points take the
// arguments of the C ABI's host calls and lay memory out as the kernels do: an element's parked (X, Y, Z), and its 64 B
// of the digit field with R's bytes in front of r.  With -DEDDSA_HARNESS_MAIN the file is a stand-alone program over the
// same entry points, for a sanitizer build.
#include "../kyber_amd/csrc/ed25519_eddsa.cuh"

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

// the encoder's value for one parked point
static void encode_parked(uint32_t w[8], const int32_t* proj) {
    ge_p3 P;
    load_fe(P.X, proj);
    load_fe(P.Y, proj + 10);
    load_fe(P.Z, proj + 20);
    fe_mul(P.T, P.X, P.Y);  // (not read by the encoding)
    ge_p3_towords(w, P);
}

extern "C" {
// kyb_ed25519_eddsa_expand's value, element by element through the two passes
void esh_expand(size_t n, const uint8_t* seeds, uint8_t* secrets, uint8_t* prefixes, uint8_t* pubs) {
    std::vector<int32_t> proj(30);
    for (size_t i = 0; i < n; i++) {
        uint32_t seed[8], secret[8], prefix[8], w[8];
        words(seed, seeds + 32 * i);
        ed_eddsa_expand_seed(secret, prefix, seed);  // (only to know which rows of the comb the lane will read)
        need_comb_rows(secret);
        ge_p3 A;
        ed_eddsa_expand_lane(A, secret, prefix, seed, g_wide);
        store_proj(proj.data(), 0, A);
        encode_parked(w, proj.data());
        memcpy(secrets + 32 * i, secret, 32);
        memcpy(prefixes + 32 * i, prefix, 32);
        memcpy(pubs + 32 * i, w, 32);
    }
}

// kyb_ed25519_eddsa_sign's value, element by element through the three passes.  status may be NULL.  r_out and h_out
// (n x 32 each, may be NULL) receive the two intermediate scalars.
void esh_sign(size_t n, const uint8_t* secrets, const uint8_t* prefixes, const uint8_t* pubs, size_t key_stride, const uint8_t* msgs,
              const uint64_t* off, uint8_t* sigs, uint8_t* status, uint8_t* r_out, uint8_t* h_out) {
    std::vector<int32_t> proj(30);
    std::vector<uint32_t> park(16);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* msg = msgs + off[i];
        const size_t len = (size_t)element_len(off, i);
        uint32_t pw[8], sw[8], aw[8], rw[8], rb[8], sig[16];
        words(pw, prefixes + i * key_stride);
        ed_eddsa_nonce(rw, pw, msg, len, order());  // (only to know which rows of the comb the lane will read)
        need_comb_rows(rw);
        ge_p3 R;
        ed_eddsa_nonce_lane(R, rw, pw, msg, len, g_wide, order());
        store_proj(proj.data(), 0, R);
        memcpy(park.data() + 8, rw, 32);
        encode_parked(rb, proj.data());
        memcpy(park.data(), rb, 32);
        // the sign pass reads the key and the element's 64 parked bytes
        words(sw, secrets + i * key_stride);
        words(aw, pubs + i * key_stride);
        memcpy(rb, park.data(), 32);
        memcpy(rw, park.data() + 8, 32);
        ed_eddsa_sign_element(sig, rb, aw, rw, sw, msg, len, order());
        memcpy(sigs + 64 * i, sig, 64);
        if (status) status[i] = 0;
        if (r_out) memcpy(r_out + 32 * i, rw, 32);
        if (h_out) {
            uint32_t hw[8];
            ed_hram(hw, rb, aw, msg, len, order());
            memcpy(h_out + 32 * i, hw, 32);
        }
    }
}
}

#ifdef EDDSA_HARNESS_MAIN
// Both entries over exactly sized heap buffers: the last message ends its buffer, an odd byte offset stands in front of
// the first element and the first element is empty; the lengths sit on either side of every block and padding boundary
// of both hashes.  Values are checked by tests/test_eddsa_host.py; this program is for the sanitizers and checks only
// that one key for the batch and the same key repeated sign alike.
int main() {
    static const size_t LENGTHS[] = {0, 1, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 175, 176, 191, 192, 207, 208, 239, 240, 1023};
    const size_t n = sizeof(LENGTHS) / sizeof(LENGTHS[0]);
    uint32_t seed = 29;
    auto filled = [&](size_t bytes) {
        uint8_t* p = new uint8_t[bytes ? bytes : 1];
        for (size_t i = 0; i < bytes; i++) {
            seed = seed * 1664525u + 1013904223u;
            p[i] = (uint8_t)(seed >> 24);
        }
        return p;
    };
    uint64_t off[n + 1];
    off[0] = 3;
    for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + LENGTHS[i];
    uint8_t *msgs = filled((size_t)off[n]), *seeds = filled(32 * n);
    uint8_t *secrets = new uint8_t[32 * n], *prefixes = new uint8_t[32 * n], *pubs = new uint8_t[32 * n];
    uint8_t *sigs = new uint8_t[64 * n], *one = new uint8_t[64 * n], *st = new uint8_t[n], *r = new uint8_t[32 * n], *h = new uint8_t[32 * n];
    esh_expand(n, seeds, secrets, prefixes, pubs);
    esh_sign(n, secrets, prefixes, pubs, 32, msgs, off, sigs, st, r, h);
    esh_sign(n, secrets, prefixes, pubs, 32, msgs, off, sigs, nullptr, nullptr, nullptr);
    esh_sign(n, secrets, prefixes, pubs, 0, msgs, off, one, st, nullptr, nullptr);
    int bad = memcmp(one, sigs, 64) != 0;
    for (size_t i = 0; i < n; i++) bad |= st[i] != 0;
    delete[] msgs; delete[] seeds; delete[] secrets; delete[] prefixes; delete[] pubs;
    delete[] sigs; delete[] one; delete[] st; delete[] r; delete[] h;
    free(g_wide);
    puts(bad ? "FAILED" : "ok");
    return bad;
}
#endif
