// kyber_amd/csrc/ed25519_cosi.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_cosi_host.py runs the roster decode, the table build at either width, the aggregate lane in both polarities
// and the check lane through these entry points against the oracle's table.  Memory is laid out as the kernels lay it
// out: the decoded roster, the subset tables built round by round, T_all by the block's tree of 256 partial sums, a
// lane's window table in a TabGlobal slab, the parked (X, Y, Z) read by the check lane, and the verdict taken on
// canonical bytes.  Every buffer is a heap allocation of exactly the size the layout states, so that the sanitizer
// build (-DCOSI_HARNESS_MAIN, tests/test_cosi_harness_sanitizers.py) sees a byte read or written past one.
#include "../kyber_amd/csrc/ed25519_cosi.cuh"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace kyb;

constexpr size_t CSH_TREE = 256;  // lanes of the T_all kernel's block

static const sf::Mod& order() {
    static const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    return m;
}

// the rows of the standard base's wide comb that r reads, built on demand with the device's row code
static int32_t* g_wide = nullptr;
static std::vector<bool> g_have;
static void need_comb_rows(const uint32_t rw[8]) {
    if (!g_wide) {
        g_wide = (int32_t*)calloc(ED_WIDE_WORDS, sizeof(int32_t));
        g_have.assign(EdWide::ROWS, false);
    }
    uint32_t x[16], sw[8];
    for (int i = 0; i < 8; i++) {
        x[i] = rw[i];
        x[8 + i] = 0;
    }
    sc_reduce512(sw, x, order());
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

// what the roster, table and T_all kernels leave in the call's workspace
struct Built {
    std::vector<int32_t> keys;
    std::vector<int4> tables, tall;
    bool bad = false;
};
static void build(Built& w, size_t m, int g, const uint8_t* roster) {
    const size_t nb = ed_cosi_groups(m, g);
    w.keys.resize(m * ED_COSI_KEY_WORDS);
    w.tables.resize((nb << g) * ED_COSI_ENTRY_INT4);
    w.tall.resize(ED_COSI_ENTRY_INT4);
    std::vector<uint32_t> rw(8 * m);
    memcpy(rw.data(), roster, 32 * m);
    for (size_t j = 0; j < m; j++) w.bad |= !ed_cosi_roster_lane(w.keys.data() + j * ED_COSI_KEY_WORDS, rw.data() + 8 * j);
    for (size_t b = 0; b < nb; b++) {
        ed_cosi_table_identity(w.tables.data(), g, b);
        for (int k = 0; k < g; k++)  // the rounds the block's barrier separates
            for (int s = 1 << k; s < 2 << k; s++) ed_cosi_table_round(w.tables.data(), w.keys.data(), m, g, b, s, k);
    }
    std::vector<ge_p3> acc(CSH_TREE);
    for (size_t t = 0; t < CSH_TREE; t++) ed_cosi_total_partial(acc[t], w.tables.data(), m, g, t, CSH_TREE);
    for (size_t half = CSH_TREE / 2; half >= 1; half >>= 1)
        for (size_t t = 0; t < half; t++) ed_cosi_total_combine(acc[t], acc[t + half]);
    ge_cached c;
    ge_p3_to_cached(c, acc[0]);
    TabGlobal out{w.tall.data()};
    out.put(0, c);
}

extern "C" {
int csh_group_width(size_t n, size_t m) { return ed_cosi_group_width(n, m); }
size_t csh_additions(size_t n, size_t m, int g) { return ed_cosi_additions(n, m, g); }

// kyb_ed25519_mask_aggregate's value at table width g, element by element.  count, status: each may be NULL.
void csh_mask_aggregate(size_t n, size_t m, int g, const uint8_t* roster, const uint8_t* masks, size_t stride, uint8_t* out,
                        uint32_t* count, uint8_t* status) {
    Built w;
    build(w, m, g, roster);
    for (size_t i = 0; i < n; i++) {
        ge_p3 acc;
        const uint32_t cnt = ed_cosi_aggregate_lane(acc, masks + i * stride, m, g, w.tables.data(), w.tall.data());
        uint32_t enc[8];
        ge_p3_towords(enc, acc);
        if (w.bad) memset(enc, 0, 32);
        memcpy(out + 32 * i, enc, 32);
        if (count) count[i] = cnt;
        if (status) status[i] = w.bad ? ED_ST_BAD_POINT : ED_ST_OK;
    }
}

// kyb_ed25519_cosi_verify's value at table width g, element by element.  agg, count, status: each may be NULL.
void csh_cosi_verify(size_t n, size_t m, int g, const uint8_t* roster, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                     const uint8_t* masks, size_t stride, uint8_t* agg, uint32_t* count, uint8_t* ok, uint8_t* status) {
    Built w;
    build(w, m, g, roster);
    std::vector<int4> slab(80);
    std::vector<int32_t> triple(30);
    for (size_t i = 0; i < n; i++) {
        ge_p3 acc, T;
        const uint32_t cnt = ed_cosi_aggregate_lane(acc, masks + i * stride, m, g, w.tables.data(), w.tall.data());
        if (w.bad) ge_p3_0(acc);
        store_proj(triple.data(), 0, acc);
        uint32_t aw[8], vw[8], rw[8], enc[8], cv[8];
        ge_p3_towords(aw, acc);
        if (w.bad) memset(aw, 0, 32);
        memcpy(vw, sigs + 64 * i, 32);
        memcpy(rw, sigs + 64 * i + 32, 32);
        need_comb_rows(rw);
        TabGlobal tab{slab.data()};
        ed_cosi_check_lane(T, vw, rw, aw, triple.data(), msgs + off[i], (size_t)(off[i + 1] - off[i]), g_wide, order(), tab);
        if (w.bad) ge_p3_0(T);
        ge_p3_towords(enc, T);
        ed_canon_point_bytes(cv, vw);
        ok[i] = !w.bad && ed_words8_equal(cv, enc);
        if (agg) memcpy(agg + 32 * i, aw, 32);
        if (count) count[i] = cnt;
        if (status) status[i] = w.bad ? ED_ST_BAD_POINT : ED_ST_OK;
    }
}
}

#ifdef COSI_HARNESS_MAIN
// Rosters at every group edge of both widths, both widths each, masks of both polarities with stray bits, at the
// exact stride and at an odd one, message lengths at the padding edges, all over exactly sized buffers.  Values are
// checked by tests/test_cosi_host.py: this program is for the sanitizers.
static uint8_t* filled(size_t bytes, uint32_t& seed) {
    uint8_t* p = new uint8_t[bytes ? bytes : 1];
    for (size_t i = 0; i < bytes; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
int main() {
    uint32_t seed = 11;
    const size_t ms[] = {1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33}, lens[] = {0, 47, 48, 63, 64, 65, 191, 192};
    const size_t n = 8;
    for (size_t m : ms)
        for (int g = 4; g <= 8; g += 4)
            for (size_t slack = 0; slack <= 3; slack += 3) {
                const size_t L = (m + 7) >> 3, stride = L + slack;
                uint8_t* roster = new uint8_t[32 * m];
                for (size_t j = 0; j < m; j++) {  // small y: most decode, and where one does not the roster is a bad one
                    memset(roster + 32 * j, 0, 32);
                    roster[32 * j] = (uint8_t)(3 + j);
                    roster[32 * j + 31] = (uint8_t)((j & 1) << 7);
                }
                uint8_t* masks = filled((n - 1) * stride + L, seed);  // the last mask ends the buffer
                memset(masks, 0xff, L);                                // full, stray bits included
                if (n > 1) memset(masks + stride, 0, L);               // empty
                uint64_t off[n + 1];
                off[0] = 0;
                for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + lens[i % 8];
                uint8_t* msgs = filled((size_t)off[n], seed);
                uint8_t* sigs = filled(64 * n, seed);
                uint8_t *out = new uint8_t[32 * n], *ok = new uint8_t[n], *st = new uint8_t[n];
                uint32_t* cnt = new uint32_t[n];
                csh_mask_aggregate(n, m, g, roster, masks, stride, out, cnt, st);
                csh_mask_aggregate(n, m, g, roster, masks, stride, out, nullptr, nullptr);
                csh_cosi_verify(n, m, g, roster, msgs, off, sigs, masks, stride, out, cnt, ok, st);
                csh_cosi_verify(n, m, g, roster, msgs, off, sigs, masks, stride, nullptr, nullptr, ok, nullptr);
                delete[] roster; delete[] masks; delete[] msgs; delete[] sigs; delete[] out; delete[] ok; delete[] st; delete[] cnt;
            }
    free(g_wide);
    puts("ok");
    return 0;
}
#endif
