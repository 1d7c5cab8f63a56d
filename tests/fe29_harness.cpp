// Stand-alone host program over kyber_amd/csrc/fe29.cuh and the ladder of ed25519_dev.cuh instantiated on fe29
// (tests/test_fe29_host.py builds and runs it; a second build under -fsanitize=undefined,signed-integer-overflow turns a
// wrapped 64-bit column into a failure).  It reads one request per line from the file named on the command line and
// answers each with one line; the test computes every expected value with Python integers.
//   <op> <9 limbs> [<9 limbs>]   add sub mul | neg sq sq2 invert pow22523 | cmov0 cmov1 cswap0 cswap1
//                                -> the result's limbs (two results for cswap)
//   towords <9 limbs>            -> eight words          fromwords <8 words> -> nine limbs
//   tofe <9 limbs>               -> ten limbs            fromfe <10 limbs>   -> nine limbs
//   const                        -> d, 2d, sqrt(-1): 27 limbs
//   walk <flags> <tab> <scalar: 8 words> <point: 8 words>
//                                -> status and eight words: ed25519_mul_kernel's walk (flags 0, 1 = KYB_F_VARTIME,
//                                   8 = KYB_F_UNIFORM; tab 0 = TabScratch, 1 = TabGlobal's slab layout)
//   audit                        -> largest m_f m_g and largest squared m_f met so far, in millionths (KYB_FE_AUDIT)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>

#include "../kyber_amd/csrc/ed25519_dev.cuh"

using namespace kyb;

static bool read_fe(std::istringstream& in, fe29& f, double mag) {
    for (int i = 0; i < 9; i++) {
        long long x;
        if (!(in >> x)) return false;
        f.v[i] = (int32_t)x;
    }
    KYB_FE_MAG_SET(f, mag);
    return true;
}
static void print_fe(const fe29& f) {
    for (int i = 0; i < 9; i++) printf("%d ", f.v[i]);
}
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
static void walk(ge29_p3& h, const int8_t e[65], const ge29_p3& A, bool full, Tab& tab, int top) {
    ge_scalarmult_w4<UNI, true>(h, e, A, full, tab, top);
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
        fe29 f, g, h;
        // operands arrive with the magnitude the test chose for them: the audit is about the walk, reset before it
        if (op == "add" || op == "sub" || op == "mul") {
            if (!read_fe(in, f, 1.0) || !read_fe(in, g, 1.0)) return 3;
            if (op == "add") fe_add(h, f, g);
            if (op == "sub") fe_sub(h, f, g);
            if (op == "mul") fe_mul(h, f, g);
            print_fe(h);
        } else if (op == "neg" || op == "sq" || op == "sq2" || op == "invert" || op == "pow22523") {
            if (!read_fe(in, f, 1.0)) return 3;
            if (op == "neg") fe_neg(h, f);
            if (op == "sq") fe_sq(h, f);
            if (op == "sq2") fe_sq2(h, f);
            if (op == "invert") fe_invert(h, f);
            if (op == "pow22523") fe_pow22523(h, f);
            print_fe(h);
        } else if (op == "cmov0" || op == "cmov1") {
            if (!read_fe(in, f, 1.0) || !read_fe(in, g, 1.0)) return 3;
            fe_cmov(f, g, op == "cmov1");
            print_fe(f);
        } else if (op == "cswap0" || op == "cswap1") {
            if (!read_fe(in, f, 1.0) || !read_fe(in, g, 1.0)) return 3;
            fe_cswap(f, g, op == "cswap1");
            print_fe(f);
            print_fe(g);
        } else if (op == "towords") {
            if (!read_fe(in, f, 1.0)) return 3;
            uint32_t w[8];
            fe_towords(w, f);
            print_words(w);
            printf("%d %d", (int)fe_isnegative(f), (int)fe_isnonzero(f));
        } else if (op == "fromwords") {
            uint32_t w[8];
            if (!read_words(in, w)) return 3;
            fe_fromwords(h, w);
            print_fe(h);
        } else if (op == "tofe") {
            if (!read_fe(in, f, 1.0)) return 3;
            fe t;
            fe29_to_fe(t, f);
            for (int i = 0; i < 10; i++) printf("%d ", t.v[i]);
        } else if (op == "fromfe") {
            fe t;
            for (int i = 0; i < 10; i++) {
                long long x;
                if (!(in >> x)) return 3;
                t.v[i] = (int32_t)x;
            }
            fe29_from_fe(h, t);
            print_fe(h);
        } else if (op == "const") {
            print_fe(fe_k<fe29>::d());
            print_fe(fe_k<fe29>::d2());
            print_fe(fe_k<fe29>::sqrtm1());
        } else if (op == "walk") {
            int flags, gtab;
            uint32_t a[8], pw[8], w[8];
            if (!(in >> flags >> gtab) || !read_words(in, a) || !read_words(in, pw)) return 3;
            const bool uni = (flags & 8) != 0, full = !uni && (flags & 1) != 0;
            ge29_p3 A, r;
            const bool ok = ge_p3_fromwords(A, pw);
            int8_t e[65];
            recode16(e, a, full);
            const int top = full ? wave_top_digit(a) : 63;
            if (gtab) {
                TabGlobal_t<fe29> tab{slab};
                uni ? walk<true>(r, e, A, full, tab, top) : walk<false>(r, e, A, full, tab, top);
            } else {
                TabScratch_t<fe29> tab;
                uni ? walk<true>(r, e, A, full, tab, top) : walk<false>(r, e, A, full, tab, top);
            }
            ge_p3_towords(w, r);
            // the deferred path parks ten-limb (X, Y, Z): its encoding must be the same bytes
            ge_p3 t;
            uint32_t w10[8];
            fe29_to_fe(t.X, r.X);
            fe29_to_fe(t.Y, r.Y);
            fe29_to_fe(t.Z, r.Z);
            ge_p3_towords(w10, t);
            if (memcmp(w, w10, sizeof w)) return 4;
            if (!ok) memset(w, 0, sizeof w);
            printf("%d ", ok ? 0 : 1);
            print_words(w);
        } else if (op == "audit") {
#if defined(KYB_FE_AUDIT)
            printf("%lld %lld", (long long)(fe29_audit_max() * 1e6), (long long)(fe29_audit_max_sq() * 1e6));
            fe29_audit_max() = fe29_audit_max_sq() = 0;
#else
            printf("-1 -1");
#endif
        } else {
            return 3;
        }
        printf("\n");
    }
    fclose(fp);
    return 0;
}
