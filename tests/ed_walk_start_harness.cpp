// Stand-alone host program over the two Ed25519 walks of kyber_amd/csrc/ed25519_dev.cuh and the way each of them starts
// (tests/test_ed25519_walk_start_host.py builds and runs it, plain with the bound audit and once more under
// -fsanitize=undefined,signed-integer-overflow): the variable-base ladder on fe29 from its top digit's table entry, the
// fixed-base comb from position 0's row.  One request per line of the file named on the command line, one answer each:
//   walk <flags> <tab> <scalar: 8 words> <point: 8 words>
//        -> status and eight words: ed25519_mul_kernel's lane (flags 0, 1 = KYB_F_VARTIME, 8 = KYB_F_UNIFORM; tab 0 =
//           TabScratch, 1 = TabGlobal's slab).  The completed point the ladder leaves is encoded as the kernel does it,
//           through (X, Y, Z), and once more through ge_scalarmult_w4's extended point: the two must agree (exit 4).
//   base <G> <full> <scalar: 8 words>
//        -> eight words: ed25519_mul_base_kernel<G>'s lane (ed_comb_walk), G = 2 or ED_COMB_G; the rows it reads are
//           built on demand with the row code of the device's table kernel (ed_comb_row)
//   audit -> largest m_f m_g and largest squared m_f of fe29, largest m_f m_g and largest 19-fold operand of fe, met
//            since the last audit, in millionths (KYB_FE_AUDIT; -1 without it)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../kyber_amd/csrc/ed25519_dev.cuh"

using namespace kyb;

static void print_words(const uint32_t w[8]) {
    for (int i = 0; i < 8; i++) printf("%u ", w[i]);
}
static bool read_words(std::istringstream& in, uint32_t w[8]) {
    for (int i = 0; i < 8; i++) {
        unsigned long long x;
        if (!(in >> x)) return false;
        w[i] = (uint32_t)x;
    }
    return true;
}

template <bool UNI, class Tab>
static bool walk(uint32_t w[8], const int8_t e[65], const ge29_p3& A, bool full, Tab& tab, int top) {
    ge29_p1p1 t;
    ge_scalarmult_w4_p1p1<UNI, true>(t, e, A, full, tab, top);
    ge29_p2 h;
    ge_p1p1_to_p2(h, t);
    ge_p3_towords(w, h);
    // what the deferred path parks: ten-limb (X, Y, Z)
    int32_t proj[30];
    store_proj(proj, 0, h);
    fe X, Y, Z, zi;
    load_fe(X, proj);
    load_fe(Y, proj + 10);
    load_fe(Z, proj + 20);
    fe_invert(zi, Z);
    uint32_t w10[8], w3[8];
    ge_encode_with_zinv(w10, X, Y, zi);
    // the extended point of the callers that go on adding
    ge29_p3 h3;
    ge_scalarmult_w4<UNI, true>(h3, e, A, full, tab, top);
    ge_p3_towords(w3, h3);
    return !memcmp(w, w10, sizeof w10) && !memcmp(w, w3, sizeof w3);
}

template <int G>
struct CombRows {
    std::vector<int32_t> tab = std::vector<int32_t>((size_t)EdComb<G>::POS * EdComb<G>::ENT * ED_TAB_STRIDE);
    std::vector<bool> have = std::vector<bool>(EdComb<G>::POS * EdComb<G>::ENT, false);
    void need(const int8_t e[65]) {
        ge_p3 B;
        B.X = fe_bx(); B.Y = fe_by(); fe_1(B.Z); B.T = fe_bt();
        for (int k = 0; k < EdComb<G>::POS; k++) {
            int d = 0;
            for (int i = G - 1; i >= 0; i--)
                if (G * k + i <= 64) d = 16 * d + (int)e[G * k + i];
            if (d == 0) continue;
            const int t = k * EdComb<G>::ENT + (d < 0 ? -d : d) - 1;
            if (have[t]) continue;
            ed_comb_row<G>(tab.data() + (size_t)t * ED_TAB_STRIDE, t, B);
            have[t] = true;
        }
    }
};

template <int G>
static void base(uint32_t w[8], const uint32_t a[8], bool full) {
    static CombRows<G> rows;
    int8_t e[65];
    recode16(e, a, full);
#if defined(KYB_FE_AUDIT)
    // the audit is about the walk: what building a row meets (the table kernel's code, run once per device) is put back
    const double keep[2] = {fe_audit_max(), fe_audit_max19()};
    rows.need(e);
    fe_audit_max() = keep[0];
    fe_audit_max19() = keep[1];
#else
    rows.need(e);
#endif
    ge_p3 h;
    ed_comb_walk<G>(h, e, full, rows.tab.data());
    ge_p3_towords(w, h);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "r");
    if (!fp) return 2;
    static char buf[4096];
    static int4 slab[80];
    while (fgets(buf, sizeof buf, fp)) {
        std::istringstream in(buf);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "walk") {
            int flags, gtab;
            uint32_t a[8], pw[8], w[8];
            if (!(in >> flags >> gtab) || !read_words(in, a) || !read_words(in, pw)) return 3;
            const bool uni = (flags & 8) != 0, full = !uni && (flags & 1) != 0;
            ge29_p3 A;
            const bool ok = ge_p3_fromwords(A, pw);
            int8_t e[65];
            recode16(e, a, full);
            const int top = full ? wave_top_digit(a) : 63;
            bool same;
            if (gtab) {
                TabGlobal_t<fe29> tab{slab};
                same = uni ? walk<true>(w, e, A, full, tab, top) : walk<false>(w, e, A, full, tab, top);
            } else {
                TabScratch_t<fe29> tab;
                same = uni ? walk<true>(w, e, A, full, tab, top) : walk<false>(w, e, A, full, tab, top);
            }
            if (!same) return 4;
            if (!ok) memset(w, 0, sizeof w);
            printf("%d ", ok ? 0 : 1);
            print_words(w);
        } else if (op == "base") {
            int g, full;
            uint32_t a[8], w[8];
            if (!(in >> g >> full) || !read_words(in, a)) return 3;
            if (g == 2)
                base<2>(w, a, full != 0);
            else if (g == ED_COMB_G)
                base<ED_COMB_G>(w, a, full != 0);
            else
                return 3;
            print_words(w);
        } else if (op == "audit") {
#if defined(KYB_FE_AUDIT)
            printf("%lld %lld %lld %lld", (long long)(fe29_audit_max() * 1e6), (long long)(fe29_audit_max_sq() * 1e6),
                   (long long)(fe_audit_max() * 1e6), (long long)(fe_audit_max19() * 1e6));
            fe29_audit_max() = fe29_audit_max_sq() = fe_audit_max() = fe_audit_max19() = 0;
#else
            printf("-1 -1 -1 -1");
#endif
        } else {
            return 3;
        }
        printf("\n");
    }
    fclose(fp);
    return 0;
}
