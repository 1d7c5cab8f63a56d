// The lane programs of kyber_amd/csrc/ed25519_verify.cuh compiled for the CPU (test infrastructure, never linked into
// libkyberhip.so): tests/test_ed_verify_host.py runs the hash, the reduction, the verify program and the Straus chain
// through these entry points against hashlib and the big-integer oracle.  Window tables live in a TabGlobal slab, as in
// the kernels; the rows of the standard base's wide comb that a signature reads are built on demand with the row code
// of the device's table kernel (ed_comb_row).
#include "../kyber_amd/csrc/ed25519_verify.cuh"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace kyb;

static const sf::Mod& order() {
    static const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    return m;
}
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

extern "C" {
// out = x mod l, x 64 bytes little-endian
void edv_reduce512(const uint8_t* x, uint8_t* out) {
    uint32_t w[16], r[8];
    memcpy(w, x, 64);
    sc_reduce512(r, w, order());
    memcpy(out, r, 32);
}
// out = SHA-512(R || A || msg) mod l
void edv_hram(const uint8_t* R, const uint8_t* A, const uint8_t* msg, size_t len, uint8_t* out) {
    uint32_t rw[8], aw[8], h[8];
    words(rw, R);
    words(aw, A);
    ed_hram(h, rw, aw, msg, len, order());
    memcpy(out, h, 32);
}
int edv_point_is_canonical(const uint8_t* enc) {
    uint32_t w[8];
    words(w, enc);
    return ed_point_is_canonical(w);
}
int edv_point_has_small_order(const uint8_t* enc) {
    uint32_t w[8];
    words(w, enc);
    return ed_point_has_small_order(w);
}
// the verify kernel's lane program + the encode pass's verdict, element by element
void edv_verify(size_t n, const uint8_t* pubs, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, uint8_t* ok,
                uint8_t* status) {
    std::vector<int4> slab(80);
    for (size_t i = 0; i < n; i++) {
        uint32_t aw[8], rw[8], sw[8], w[8];
        words(aw, pubs + 32 * i);
        words(rw, sigs + 64 * i);
        words(sw, sigs + 64 * i + 32);
        need_comb_rows(sw);
        TabGlobal tab{slab.data()};
        ge_p3 T;
        const int st = ed_verify_lane(T, rw, sw, aw, msgs + off[i], (size_t)(off[i + 1] - off[i]), g_wide, order(), tab);
        ge_p3_towords(w, T);
        status[i] = (uint8_t)st;
        ok[i] = st == ED_ST_OK && memcmp(w, rw, 32) == 0;
    }
}
// out = a P + b Q (zero bytes and status 1 where a point does not decode); full: KYB_F_VARTIME's digits
void edv_mul2(size_t n, const uint8_t* a, const uint8_t* P, const uint8_t* b, const uint8_t* Q, int full, uint8_t* out,
              uint8_t* status) {
    std::vector<int4> slab(160);
    for (size_t i = 0; i < n; i++) {
        uint32_t aw[8], pw[8], bw[8], qw[8], w[8];
        words(aw, a + 32 * i);
        words(pw, P + 32 * i);
        words(bw, b + 32 * i);
        words(qw, Q + 32 * i);
        TabGlobal tp{slab.data()}, tq{slab.data() + 80};
        ge_p3 h;
        const bool good = ed_mul2_lane(h, aw, pw, bw, qw, full != 0, tp, tq);
        ge_p3_towords(w, h);
        if (!good) memset(w, 0, 32);
        memcpy(out + 32 * i, w, 32);
        status[i] = good ? 0 : 1;
    }
}
}
