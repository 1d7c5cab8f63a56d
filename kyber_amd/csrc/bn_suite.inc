// Barreto-Naehrig suites of the reference -- pairing/bn256 (dclxvi parameters) and pairing/bn254 (alt_bn128; the same
// package over other constants, with stricter decoding) -- as ONE device library, instantiated per curve by the
// wrapper that includes this file (bn256.cuh, bn254.cuh) after defining
//     KYB_BN_NS      namespace of the instance (kyb::bn, kyb::bn4)
//     KYB_BN_PARAMS  prefix of the parameter structs of <curve>_params.h (Bn256 -> Bn256Fp / Bn256Tower / Bn256Curve)
//     KYB_BN_MUL_WAVES  register budget of group_mul_kernel<G1> / <G2> in waves per SIMD (set by the wrapper header, not by a
//                    translation unit, so that every unit sees one definition of the group policies)
//     KYB_BN_FB_SUITE  the suite's index among the fixed-base workspace kinds (context.h WS_FB: bn256 1, bn254 2)
// G1 / G2 / GT wire formats and acceptance rules, scalar multiplication, GT exponentiation.
//
// Replaces (bn256 citations; bn254's files are line-shifted copies): pointG1/G2.Mul + (Un)MarshalBinary
// (point.go:154-238, 405-499), curvePoint/twistPoint.Mul (curve.go:189, twist.go:162), pointGT.Mul + (Un)MarshalBinary
// (point.go:613-716).  Suite.Pair / ValidatePairing are not here: they run on the tower machine (bn_pair.inc).
// CC::STRICT (bn254): gfP.Unmarshal rejects coordinates >= p (bn254/gfp.go:101-118) and twistPoint.IsOnCurve also
// requires [Order]Q = infinity (bn254/twist.go:47-66); bn256 reduces the former and never checks the latter.
#include "curve.cuh"
#include "fixed_base.cuh"
#include "jac_lazy.cuh"

#define KYB_BN_CAT_(a, b) a##b
#define KYB_BN_CAT(a, b) KYB_BN_CAT_(a, b)

namespace kyb {
namespace KYB_BN_NS {

using FC = KYB_BN_CAT(KYB_BN_PARAMS, Fp);
using TC = KYB_BN_CAT(KYB_BN_PARAMS, Tower);
using CC = KYB_BN_CAT(KYB_BN_PARAMS, Curve);
using fp = Fp<FC>;
using fp2 = Fp2<TC>;
using fp6 = Fp6<TC>;
using fp12 = Fp12<TC>;
using g1_aff = Aff<fp>;
using g2_aff = Aff<fp2>;
using g1_jac = Jac<fp>;
using g2_jac = Jac<fp2>;

constexpr int ST_OK = 0, ST_BAD_POINT = 1, ST_NOT_IN_SUBGROUP = 2;


KYB_HD void fp_const(fp& r, const uint32_t (&c)[FC::NWORDS]) {
#pragma unroll
    for (int l = 0; l < FC::NWORDS; l++) r.v[l] = c[l];
}

// ------------------------------------------------------------------ decoding
// 32-byte big-endian coordinate, reduced mod p like montEncode does (bn256 point.go:218-221: values >= p are
// accepted); returns whether it was canonical -- which is all a STRICT suite accepts (bn254 gfp.go:101-118).
KYB_HD bool fp_decode(fp& r, const uint8_t* in) {
    uint32_t w[8];
    words_from_be<8>(w, in);
    const bool canon = fp_words_lt_p<FC>(w);
    fp_from_words<FC>(r, w);
    return canon;
}
KYB_HD void fp_encode(uint8_t* out, const fp& a) {
    uint32_t w[8];
    fp_to_words<FC>(w, a);
    words_to_be<8>(out, w);
}
// pointG1.UnmarshalBinary (point.go:206-238): (0, 0) is infinity; otherwise y^2 = x^3 + 3.
// bn256's wire format is already uncompressed affine and its UnmarshalBinary has no subgroup check
// (point.go:206-238, 466-499), so the flags of the shared ABI change nothing here.
KYB_HD size_t g1_wire_size(uint32_t) { return 64; }
KYB_HD size_t g2_wire_size(uint32_t) { return 128; }
// bn256's UnmarshalBinary checks the curve equation only (point.go:466-499): a decoded G2 point is NOT thereby a point
// of the order-n subgroup, and KYB_F_TRUSTED(0) -- which selects the GLS walk in g2_mul_wire -- must not be inferred from it
constexpr bool g2_decode_proves_subgroup() { return CC::STRICT; }
KYB_HD size_t g1_out_size(uint32_t) { return 64; }
KYB_HD size_t g2_out_size(uint32_t) { return 128; }
KYB_HD_NOINLINE int g1_decode(g1_aff& a, const uint8_t* in) {
    bool canon = fp_decode(a.x, in);
    canon &= fp_decode(a.y, in + 32);
    a.inf = fp_is_zero(a.x) & fp_is_zero(a.y);
    if (CC::STRICT && !canon) {
        a.inf = true;
        return ST_BAD_POINT;
    }
    fp y2, x3, b;
    fp_const(b, CC::B1);
    fp_sqr(y2, a.y);
    fp_sqr(x3, a.x);
    fp_mul(x3, x3, a.x);
    fp_add(x3, x3, b);
    return (a.inf || fp_eq(y2, x3)) ? ST_OK : ST_BAD_POINT;
}
// psi = twist^-1 o Frobenius o twist on a Jacobian point of E'(Fp2): (conj(X) PSI_X, conj(Y) PSI_Y, conj(Z))
KYB_HD void g2_psi(g2_jac& r, const g2_jac& p) {
    fp2 k, t;
    fp2_load_const<TC>(k, CC::PSI_X);
    fp2_conj(t, p.X);
    fp2_mul_c(r.X, t, k);
    fp2_load_const<TC>(k, CC::PSI_Y);
    fp2_conj(t, p.Y);
    fp2_mul_c(r.Y, t, k);
    fp2_conj(r.Z, p.Z);
}
// [Order]Q = infinity (bn254 twist.go:62-65) for a point Q of the twist, decided by
//     [u + 1]Q + psi([u]Q) + psi^2([u]Q) = psi^3([2u]Q)
// -- one 63-bit multiplication instead of a 254-bit one.  On G2 psi is [p] and (u + 1) + u p + u p^2 - 2u p^3 = 0 mod n.
// Conversely #E'(Fp2) = n h with h = 2p - n squarefree and prime to n, so the group is cyclic and psi acts on its
// q-part (q | h prime) as a root mu of X^2 - t X + p; the polynomial (u + 1) + u mu + u mu^2 - 2u mu^3 is non-zero
// mod q for every such root (alt_bn128: h = 10069 * 5864401 * 1875725156269 * (a 178-bit prime), checked in
// tests/test_constants.py), so the relation fails on any point with a component outside G2: equivalent to the
// reference's test, not an approximation of it.
KYB_HD_NOINLINE bool g2_in_subgroup(const g2_aff& a) {
    g2_jac xq, b, lhs, rhs;
#ifdef KYB_BN_PACKED_LADDER
    jac_mul_u64_aff(xq, a, CC::U);
#else
    jaclz_mul_u64_aff<LzFp2<Limb30<FC>, TC>>(xq, a, CC::U);  // [u] Q on lazy limbs (jac_lazy.cuh): nine tenths of this test
#endif
    g2_psi(b, xq);           // psi([u]Q)
    jac_madd(lhs, xq, a.x, a.y, a.inf);  // [u + 1]Q
    jac_add(lhs, lhs, b);
    g2_psi(rhs, b);          // psi^2([u]Q)
    jac_add(lhs, lhs, rhs);
    g2_psi(rhs, rhs);        // psi^3([u]Q)
    jac_dbl(rhs, rhs);
    return jac_eq(lhs, rhs);
}
// pointG2.UnmarshalBinary (point.go:466-499): x.x, x.y, y.x, y.y with gfP2{x, y} = x i + y; on the twist.  bn256 never
// checks the subgroup; a STRICT suite does (bn254 twist.go:62-65: [Order]Q = infinity, decided by g2_in_subgroup)
// unless the caller vouches for the operand (KYB_F_TRUSTED: it unmarshalled the point before).
KYB_HD_NOINLINE int g2_decode(g2_aff& a, const uint8_t* in, bool check_subgroup = true) {
    bool canon = fp_decode(a.x.c1, in);
    canon &= fp_decode(a.x.c0, in + 32);
    canon &= fp_decode(a.y.c1, in + 64);
    canon &= fp_decode(a.y.c0, in + 96);
    a.inf = fp2_is_zero(a.x) & fp2_is_zero(a.y);
    if (CC::STRICT && !canon) {
        a.inf = true;
        return ST_BAD_POINT;
    }
    fp2 y2, x3, b;
    fp2_load_const<TC>(b, CC::B2);
    fp2_sqr_c(y2, a.y);
    fp2_sqr_c(x3, a.x);
    fp2_mul_c(x3, x3, a.x);
    fp2_add(x3, x3, b);
    if (!(a.inf || fp2_eq(y2, x3))) return ST_BAD_POINT;
    if (CC::STRICT && check_subgroup && !a.inf && !g2_in_subgroup(a)) return ST_NOT_IN_SUBGROUP;
    return ST_OK;
}
KYB_HD int g2_decode_f(g2_aff& a, const uint8_t* in, uint32_t flags, int arg) { return g2_decode(a, in, !flag_trusted(flags, arg)); }
// the flag-taking names of the shared ABI (pairing_abi.cuh, fixed_base.cuh): this suite's wire format has one form
KYB_HD int g1_decode_f(g1_aff& a, const uint8_t* in, uint32_t, int) { return g1_decode(a, in); }
// fixed-base table policies (fixed_base.cuh): the plain integer multiple on both groups -- G1 has prime order (every
// point of the curve is a member), and bn256's G2 accepts points outside the order-n subgroup, which must multiply as
// the reference's double-and-add does.  A STRICT suite's G2 rule -- [Order] Q = infinity (bn254/twist.go:62-65) -- is
// read off the finished table: one walk of the plain image with the order as the scalar.
struct fb_g1_policy : fb::Plain<fp> {
    KYB_HD static int decode_on_curve(g1_aff& a, const uint8_t* in, uint32_t) { return g1_decode(a, in); }
    KYB_HD static bool needs_member(uint32_t) { return false; }
    KYB_HD static bool member(const g1_aff&, const fb::Entry<fp, 1>*) { return true; }
};
struct fb_g2_policy : fb::Plain<fp2> {
    KYB_HD static int decode_on_curve(g2_aff& a, const uint8_t* in, uint32_t) { return g2_decode(a, in, false); }
    KYB_HD static bool needs_member(uint32_t flags) { return CC::STRICT && !flag_trusted(flags, 0); }
    KYB_HD static bool member(const g2_aff&, const fb::Entry<fp2, 1>* __restrict__ tab) {
        uint32_t n[8];
#pragma unroll
        for (int i = 0; i < 8; i++) n[i] = CC::ORDER[i];
        g2_jac q;
        fb::mul_plain<1>(q, n, NW, tab);
        return jac_is_inf(q);
    }
};
// MarshalBinary: infinity is all zero bytes (point.go:170-192, 423-452)
KYB_HD_NOINLINE void g1_encode(uint8_t* out, const g1_aff& a) {
    fp x = a.x, y = a.y;
    if (a.inf) {
        fp_zero(x);
        fp_zero(y);
    }
    fp_encode(out, x);
    fp_encode(out + 32, y);
}
KYB_HD_NOINLINE void g2_encode(uint8_t* out, const g2_aff& a) {
    fp2 x = a.x, y = a.y;
    if (a.inf) {
        fp2_zero(x);
        fp2_zero(y);
    }
    fp_encode(out, x.c1);
    fp_encode(out + 32, x.c0);
    fp_encode(out + 64, y.c1);
    fp_encode(out + 96, y.c0);
}
KYB_HD void g1_encode_f(uint8_t* out, const g1_aff& a, uint32_t) { g1_encode(out, a); }
KYB_HD void g2_encode_f(uint8_t* out, const g2_aff& a, uint32_t) { g2_encode(out, a); }
KYB_HD void scalar_from_be(uint32_t (&k)[8], const uint8_t* in) { words_from_be<8>(k, in); }
// pointGT.MarshalBinary (point.go:630-662): x.x.x, x.x.y, ..., y.z.y  ==  omega-coefficient
// first, tau^2 / tau / 1 order inside, imaginary part before real part.
KYB_HD_NOINLINE void gt_encode(uint8_t* out, const fp12& f) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const fp6& s = h == 0 ? f.c1 : f.c0;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const fp2& c = m == 0 ? s.c2 : (m == 1 ? s.c1 : s.c0);
            fp_encode(out + (h * 3 + m) * 64, c.c1);
            fp_encode(out + (h * 3 + m) * 64 + 32, c.c0);
        }
    }
}

// pointGT.UnmarshalBinary (point.go:664-716): twelve coefficients reduced mod p, no membership check
KYB_HD_NOINLINE int gt_decode(fp12& f, const uint8_t* in) {
    bool canon = true;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        fp6& s = h == 0 ? f.c1 : f.c0;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            fp2& c = m == 0 ? s.c2 : (m == 1 ? s.c1 : s.c0);
            canon &= fp_decode(c.c1, in + (h * 3 + m) * 64);
            canon &= fp_decode(c.c0, in + (h * 3 + m) * 64 + 32);
        }
    }
    return (CC::STRICT && !canon) ? ST_BAD_POINT : ST_OK;
}

// ------------------------------------------------- GLV scalar multiplication on G1
// G1 = E(Fp) has prime order n (cofactor 1), so phi(x, y) = (beta x, y) acts as [lambda] on every accepted point and
// k P = k1 P + k2 phi(P) for the Babai-rounded split k = k1 + k2 lambda (mod n), |k1|, |k2| < 2^130 (constants and
// their derivation: gen_consts.py bn256()).  34 windows of (4 doublings + 2 additions) instead of 65 x (4 + 1).
// G2: bn256's UnmarshalBinary accepts twist points outside the order-n subgroup, where the Frobenius eigenvalue relation
// does not hold and the reference's double-and-add result must be reproduced -- g2_mul_wire decides membership first
// and keeps the plain ladder for the points that fail.
//
// r (NR low words) = a (NA words) * b (NB words)
template <int NR, int NA, int NB>
KYB_HD void mul_words(uint32_t (&r)[NR], const uint32_t* a, const uint32_t* b) {
    uint64_t acc = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < NR; k++) {
        // column k: sum a[i] b[k - i]; 96-bit accumulation in (hi : acc)
#pragma unroll
        for (int i = 0; i < NA; i++) {
            const int j = k - i;
            if (j < 0 || j >= NB) continue;
            const uint64_t pr = (uint64_t)a[i] * b[j];
            acc += pr;
            hi += acc < pr ? 1u : 0u;
        }
        r[k] = (uint32_t)acc;
        acc = (acc >> 32) | (hi << 32);
        hi = 0;
    }
}
KYB_HD bool abs_words5(uint32_t (&x)[5]) {  // 160-bit two's complement -> magnitude, returns the sign
    const bool neg = (x[4] >> 31) != 0;
    uint32_t b = 0, t[5];
#pragma unroll
    for (int i = 0; i < 5; i++) t[i] = sbb32(0u, x[i], b);
#pragma unroll
    for (int i = 0; i < 5; i++) x[i] = neg ? t[i] : x[i];
    return neg;
}
// k -> (|k1|, sign1, |k2|, sign2)
KYB_HD void glv_split(uint32_t (&m1)[5], bool& n1, uint32_t (&m2)[5], bool& n2, const uint32_t (&k)[8]) {
    uint32_t g1[3], g2[5], a1[2], a2[4], b1n[4], b2[2];
#pragma unroll
    for (int i = 0; i < 3; i++) g1[i] = CC::GLV_G1[i];
#pragma unroll
    for (int i = 0; i < 5; i++) g2[i] = CC::GLV_G2[i];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        a1[i] = CC::GLV_A1[i];
        b2[i] = CC::GLV_B2[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        a2[i] = CC::GLV_A2[i];
        b1n[i] = CC::GLV_B1N[i];
    }
    uint32_t p1[11], p2[13];
    mul_words<11, 8, 3>(p1, k, g1);
    mul_words<13, 8, 5>(p2, k, g2);
    uint32_t c1[3] = {p1[8], p1[9], p1[10]};
    uint32_t c2[5] = {p2[8], p2[9], p2[10], p2[11], p2[12]};
    uint32_t t1[5], t2[5], t3[5], t4[5];
    mul_words<5, 3, 2>(t1, c1, a1);   // c1 A1
    mul_words<5, 5, 4>(t2, c2, a2);   // c2 A2
    mul_words<5, 3, 4>(t3, c1, b1n);  // c1 |B1|
    mul_words<5, 5, 2>(t4, c2, b2);   // c2 B2
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) m1[i] = sbb32(k[i], t1[i], b);
    b = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) m1[i] = sbb32(m1[i], t2[i], b);  // k1 = k - c1 A1 - c2 A2   (mod 2^160, |k1| < 2^130)
    b = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) m2[i] = sbb32(t3[i], t4[i], b);  // k2 = c1 |B1| - c2 B2
    n1 = abs_words5(m1);
    n2 = abs_words5(m2);
}
KYB_HD_NOINLINE void g1_mul_glv(g1_jac& r, const g1_jac& p, const uint32_t (&k)[8]) {
    uint32_t m1[5], m2[5];
    bool n1, n2;
    glv_split(m1, n1, m2, n2, k);
    uint32_t w1[8], w2[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        w1[i] = i < 5 ? m1[i] : 0u;
        w2[i] = i < 5 ? m2[i] : 0u;
    }
    int8_t e1[65], e2[65];
    recode16_u256(e1, w1);
    recode16_u256(e2, w2);
    g1_jac tab[8];  // (j + 1) * P
    tab[0] = p;
    jac_dbl(tab[1], p);
#pragma unroll 1
    for (int j = 2; j < 8; j++) jac_add(tab[j], tab[j - 1], p);
    jac_table8_to_affine(tab);  // the 66 table additions below are mixed additions
    fp beta;
    fp_const(beta, CC::BETA);
    // (fusing the window into one out-of-line step, as BLS12-381 G1 does, cost 13 % here: left as separate calls)
    g1_jac acc;
    fp tx, ty;
    bool tinf;
    jac_set_inf(acc);
#pragma unroll 1
    for (int i = 33; i >= 0; i--) {
        if (i != 33) jac_dbl_n(acc, acc, 4);
        jac_select8_xy(tx, ty, tinf, tab, n1 ? -e1[i] : e1[i]);
        jac_madd_if(acc, tx, ty, tinf, e1[i] != 0);
        jac_select8_xy(tx, ty, tinf, tab, n2 ? -e2[i] : e2[i]);
        fp_mul(tx, tx, beta);
        jac_madd_if(acc, tx, ty, tinf, e2[i] != 0);
    }
    r = acc;
}

// ------------------------------------------------- GLS scalar multiplication on G2
// On the order-n subgroup of the twist psi acts as [6u^2]: k Q = k0 Q + k1 psi(Q) + k2 psi^2(Q) + k3 psi^3(Q) with the
// Babai-rounded split of gen_consts.py (|kj| < 2^66): 17 windows of (4 doublings + 4 additions), one table of Q's
// multiples whose entries go through psi^j on the way into the addition -- against 65 windows of (4 + 1) for the plain
// ladder.  Only for points of the subgroup: every point a STRICT suite decodes (bn254), and on bn256 the points the
// caller vouches for (KYB_F_TRUSTED); bn256's unchecked G2 inputs keep the plain ladder, whose result the reference's
// double-and-add defines there.
KYB_HD void gls_split(uint32_t (&m)[4][3], bool (&neg)[4], const uint32_t (&k)[8]) {
    uint32_t c[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t g[7], pr[11];
#pragma unroll
        for (int w = 0; w < 7; w++) g[w] = CC::GLS_G[i][w];
        mul_words<11, 8, 7>(pr, k, g);
        c[i][0] = pr[8];
        c[i][1] = pr[9];
        c[i][2] = pr[10];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t v[3] = {j == 0 ? k[0] : 0u, j == 0 ? k[1] : 0u, j == 0 ? k[2] : 0u};  // everything mod 2^96: |kj| < 2^66
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t b[3], t[3];
#pragma unroll
            for (int w = 0; w < 3; w++) b[w] = CC::GLS_B[i][j][w];
            mul_words<3, 3, 3>(t, c[i], b);
            const bool minus = (((CC::GLS_G_NEG >> i) ^ (CC::GLS_B_NEG[i] >> j)) & 1u) == 0;  // v -= (+c)(+b) or (-c)(-b)
            uint32_t cy = 0;
            if (minus) {
#pragma unroll
                for (int w = 0; w < 3; w++) v[w] = sbb32(v[w], t[w], cy);
            } else {
#pragma unroll
                for (int w = 0; w < 3; w++) v[w] = adc32(v[w], t[w], cy);
            }
        }
        neg[j] = (v[2] >> 31) != 0;
        uint32_t b = 0, z[3];
#pragma unroll
        for (int w = 0; w < 3; w++) z[w] = sbb32(0u, v[w], b);
#pragma unroll
        for (int w = 0; w < 3; w++) m[j][w] = neg[j] ? z[w] : v[w];
    }
}
KYB_HD_NOINLINE void g2_mul_gls(g2_jac& r, const g2_jac& p, const uint32_t (&k)[8]) {
    uint32_t m[4][3];
    bool neg[4];
    gls_split(m, neg, k);
    int8_t e[4][65];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = i < 3 ? m[j][i] : 0u;
        recode16_u256(e[j], w);
    }
    g2_jac tab[8];  // (i + 1) Q
    tab[0] = p;
    jac_dbl(tab[1], p);
#pragma unroll 1
    for (int i = 2; i < 8; i++) jac_add(tab[i], tab[i - 1], p);
    jac_table8_to_affine(tab);  // psi^j acts on the affine entry; the 68 table additions are mixed additions
    // psi(x, y) = (cx conj x, cy conj y) on the affine entry; psi^2 scales X, Y by the norms of cx, cy; psi^3 = psi^2 o psi
    fp2 cx, cy, cx3, cy3, t2;
    fp nx, ny, u;
    fp2_load_const<TC>(cx, CC::PSI_X);
    fp2_load_const<TC>(cy, CC::PSI_Y);
    fp_sqr(nx, cx.c0);
    fp_sqr(u, cx.c1);
    fp_add(nx, nx, u);
    fp_sqr(ny, cy.c0);
    fp_sqr(u, cy.c1);
    fp_add(ny, ny, u);
    fp2_mul_fp(cx3, cx, nx);
    fp2_mul_fp(cy3, cy, ny);
    g2_jac acc;
    fp2 tx, ty;
    bool tinf;
    jac_set_inf(acc);
#pragma unroll 1
    for (int i = 16; i >= 0; i--) {
        if (i != 16) jac_dbl_n(acc, acc, 4);
        jac_select8_xy(tx, ty, tinf, tab, neg[0] ? -e[0][i] : e[0][i]);
        jac_madd_if(acc, tx, ty, tinf, e[0][i] != 0);
        jac_select8_xy(tx, ty, tinf, tab, neg[1] ? -e[1][i] : e[1][i]);
        fp2_conj(t2, tx);
        fp2_mul_c(tx, t2, cx);
        fp2_conj(t2, ty);
        fp2_mul_c(ty, t2, cy);
        jac_madd_if(acc, tx, ty, tinf, e[1][i] != 0);
        jac_select8_xy(tx, ty, tinf, tab, neg[2] ? -e[2][i] : e[2][i]);
        fp2_mul_fp(tx, tx, nx);
        fp2_mul_fp(ty, ty, ny);
        jac_madd_if(acc, tx, ty, tinf, e[2][i] != 0);
        jac_select8_xy(tx, ty, tinf, tab, neg[3] ? -e[3][i] : e[3][i]);
        fp2_conj(t2, tx);
        fp2_mul_c(tx, t2, cx3);
        fp2_conj(t2, ty);
        fp2_mul_c(ty, t2, cy3);
        jac_madd_if(acc, tx, ty, tinf, e[3][i] != 0);
    }
    r = acc;
}

// ------------------------------------------------- the same two walks in lazy limb form (jac_lazy.cuh)
// Since round 5 the ladders of Point.Mul run on 30-bit limbs with no reduction between the products of a formula and
// no out-of-line multiplier: the window table is built by the packed code as before (eight multiples, one shared
// inversion), its entries -- and their images under the endomorphism: beta x on G1, psi^j on G2 -- enter the limb form
// once, and the walk is two inlined loop bodies (a doubling, a mixed addition).  -DKYB_BN_PACKED_LADDER keeps the
// packed walks (A/B builds).
#ifndef KYB_LZ_LADDER_ATTR
#define KYB_LZ_LADDER_ATTR KYB_HD_NOINLINE
#endif
using L30 = Limb30<FC>;
using lz1 = LzFp<L30>;
using lz2 = LzFp2<L30, TC>;

// (inlined into its one caller: as an out-of-line function the G1 walk came back wrong on the device -- every lane, dbl and
// madd each correct on their own, the host build and the inlined device build correct; tools/lz_probe.hip.  The code
// generation fault of DESIGN.md section 9 item 5 in another guise: the function writes its caller's private point
// through a reference.)
KYB_HD void g1_mul_glv_lz(g1_jac& r, const g1_jac& p, const uint32_t (&k)[8]) {
    uint32_t m1[5], m2[5];
    bool n1, n2;
    glv_split(m1, n1, m2, n2, k);
    uint32_t w1[8], w2[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        w1[i] = i < 5 ? m1[i] : 0u;
        w2[i] = i < 5 ? m2[i] : 0u;
    }
    int8_t e1[65], e2[65];
    recode16_u256(e1, w1);
    recode16_u256(e2, w2);
    if (jac_is_inf(p)) {
        jac_set_inf(r);
        return;
    }
    typename lz1::E tx[2][8], ty[8], beta;  // (j + 1) P and its image (beta x, y), affine, in limb form
    uint32_t infmask;
    jaclz_table8<lz1, false>(tx[0], ty, infmask, p.X, p.Y);  // p comes from jac_from_aff: Z = 1
    {
        fp b;
        fp_const(b, CC::BETA);
        lz1::enter(beta, b);
    }
#pragma unroll 1
    for (int j = 0; j < 8; j++) lz1::template mul<2>(tx[1][j], tx[0][j], beta);
    JacLz<lz1> acc;
    jaclz_set_inf(acc);
#pragma unroll 1
    for (int i = 33; i >= 0; i--) {
        if (i != 33) {
#pragma unroll 1
            for (int d = 0; d < 4; d++) jaclz_dbl(acc);
        }
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            const int d = h == 0 ? e1[i] : e2[i];
            if (d == 0) continue;
            const int idx = (d < 0 ? -d : d) - 1;
            if ((infmask >> idx) & 1u) continue;
            jaclz_madd(acc, tx[h][idx], ty[idx], (d < 0) != (h == 0 ? n1 : n2));
        }
    }
    jaclz_leave(r, acc);
}

// The 32 table entries of the walk (8 multiples x 4 psi images, (x, y) of 36 limb words each = 4 608 bytes per lane) are
// read by the lane's own digits.  In private scratch -- interleaved per dword across the lanes of a wave -- an indexed
// entry read drags in up to eight rows per dword: 14.5 GB fetched and written per 2^18 multiplications against 75 MB of
// operands (VERDICT r5: 192 x, VALU busy 0.85).  TAB = true keeps them in a lane-contiguous slab of global memory
// instead (`tab`: this lane's G2_TAB_WORDS words; an entry is nine 16-byte loads from three cache lines), the layout that
// took the Ed25519 window table from 40.9 to 5.5 GB (DESIGN.md section 3).  TAB = false (the host harness, and the
// reference point for A/B runs: -DKYB_BN_G2_TAB_SCRATCH) keeps the arrays.
constexpr size_t G2_TAB_ENTRY_WORDS = 4 * L30::N;                 // x.c0, x.c1, y.c0, y.c1
constexpr size_t G2_TAB_WORDS = 4 * 8 * G2_TAB_ENTRY_WORDS;       // per lane
static_assert(G2_TAB_ENTRY_WORDS % 4 == 0, "an entry is a whole number of 16-byte pieces");
KYB_HD void g2_tab_put(uint32_t* __restrict__ tab, int j, int i, const typename lz2::E& x, const typename lz2::E& y) {
    uint32_t w[G2_TAB_ENTRY_WORDS];
#pragma unroll
    for (int l = 0; l < L30::N; l++) {
        w[l] = x.c0.l[l];
        w[L30::N + l] = x.c1.l[l];
        w[2 * L30::N + l] = y.c0.l[l];
        w[3 * L30::N + l] = y.c1.l[l];
    }
    uint32_t* q = tab + (size_t)(j * 8 + i) * G2_TAB_ENTRY_WORDS;
#if defined(__HIPCC__)
#pragma unroll
    for (int v = 0; v < (int)G2_TAB_ENTRY_WORDS / 4; v++)
        reinterpret_cast<uint4*>(q)[v] = make_uint4(w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]);
#else
    for (int v = 0; v < (int)G2_TAB_ENTRY_WORDS; v++) q[v] = w[v];
#endif
}
KYB_HD void g2_tab_get(typename lz2::E& x, typename lz2::E& y, const uint32_t* __restrict__ tab, int j, int i) {
    uint32_t w[G2_TAB_ENTRY_WORDS];
    const uint32_t* q = tab + (size_t)(j * 8 + i) * G2_TAB_ENTRY_WORDS;
#if defined(__HIPCC__)
#pragma unroll
    for (int v = 0; v < (int)G2_TAB_ENTRY_WORDS / 4; v++) {
        const uint4 t = reinterpret_cast<const uint4*>(q)[v];
        w[4 * v] = t.x;
        w[4 * v + 1] = t.y;
        w[4 * v + 2] = t.z;
        w[4 * v + 3] = t.w;
    }
#else
    for (int v = 0; v < (int)G2_TAB_ENTRY_WORDS; v++) w[v] = q[v];
#endif
#pragma unroll
    for (int l = 0; l < L30::N; l++) {
        x.c0.l[l] = w[l];
        x.c1.l[l] = w[L30::N + l];
        y.c0.l[l] = w[2 * L30::N + l];
        y.c1.l[l] = w[3 * L30::N + l];
    }
    KYB_LZ_K(x.c0.k = x.c1.k = y.c0.k = y.c1.k = 2.0;)
}
template <bool TAB>
KYB_LZ_LADDER_ATTR void g2_mul_gls_lz(g2_jac& r, const g2_jac& p, const uint32_t (&k)[8], uint32_t* __restrict__ tab = nullptr) {
    uint32_t m[4][3];
    bool neg[4];
    gls_split(m, neg, k);
    int8_t e[4][65];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = i < 3 ? m[j][i] : 0u;
        recode16_u256(e[j], w);
    }
    if (jac_is_inf(p)) {
        jac_set_inf(r);
        return;
    }
    // psi(x, y) = (cx conj x, cy conj y); psi^2 scales x, y by the norms of cx, cy; psi^3 = psi^2 o psi: the four images
    // of every table entry are made once, in limb form
    constexpr int NT = TAB ? 1 : 4;
    typename lz2::E tx[NT][8], ty[NT][8], cx, cy, cx3, cy3, t2;
    FpL<L30> nx, ny;
    uint32_t infmask;
    jaclz_table8<lz2, false>(tx[0], ty[0], infmask, p.X, p.Y);  // (i + 1) Q, affine, in limb form (p: Z = 1)
    {
        fp2 pcx, pcy, pcx3, pcy3;
        fp pnx, pny, u;
        fp2_load_const<TC>(pcx, CC::PSI_X);
        fp2_load_const<TC>(pcy, CC::PSI_Y);
        fp_sqr(pnx, pcx.c0);
        fp_sqr(u, pcx.c1);
        fp_add(pnx, pnx, u);
        fp_sqr(pny, pcy.c0);
        fp_sqr(u, pcy.c1);
        fp_add(pny, pny, u);
        fp2_mul_fp(pcx3, pcx, pnx);
        fp2_mul_fp(pcy3, pcy, pny);
        lz2::enter(cx, pcx);
        lz2::enter(cy, pcy);
        lz2::enter(cx3, pcx3);
        lz2::enter(cy3, pcy3);
        lz_enter(nx, pnx);
        lz_enter(ny, pny);
    }
#pragma unroll 1
    for (int i = 0; i < 8; i++) {
        typename lz2::E x1, y1, x2, y2, x3, y3;
        lz2::template conj<2>(t2, tx[0][i]);
        lz2::template mul<2>(x1, t2, cx);
        lz2::template mul<2>(x3, t2, cx3);
        lz2::template conj<2>(t2, ty[0][i]);
        lz2::template mul<2>(y1, t2, cy);
        lz2::template mul<2>(y3, t2, cy3);
        lz2::mul_fp(x2, tx[0][i], nx);
        lz2::mul_fp(y2, ty[0][i], ny);
        if constexpr (TAB) {
            g2_tab_put(tab, 0, i, tx[0][i], ty[0][i]);
            g2_tab_put(tab, 1, i, x1, y1);
            g2_tab_put(tab, 2, i, x2, y2);
            g2_tab_put(tab, 3, i, x3, y3);
        } else {
            tx[NT - 1 < 1 ? 0 : 1][i] = x1;
            ty[NT - 1 < 1 ? 0 : 1][i] = y1;
            tx[NT - 1 < 2 ? 0 : 2][i] = x2;
            ty[NT - 1 < 2 ? 0 : 2][i] = y2;
            tx[NT - 1 < 3 ? 0 : 3][i] = x3;
            ty[NT - 1 < 3 ? 0 : 3][i] = y3;
        }
    }
    JacLz<lz2> acc;
    jaclz_set_inf(acc);
#pragma unroll 1
    for (int i = 16; i >= 0; i--) {
        if (i != 16) {
#pragma unroll 1
            for (int d = 0; d < 4; d++) jaclz_dbl(acc);
        }
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            const int d = e[j][i];
            if (d == 0) continue;
            const int idx = (d < 0 ? -d : d) - 1;
            if ((infmask >> idx) & 1u) continue;
            if constexpr (TAB) {
                typename lz2::E ex, ey;
                g2_tab_get(ex, ey, tab, j, idx);
                jaclz_madd(acc, ex, ey, (d < 0) != neg[j]);
            } else {
                jaclz_madd(acc, tx[NT - 1 < j ? 0 : j][idx], ty[NT - 1 < j ? 0 : j][idx], (d < 0) != neg[j]);
            }
        }
    }
    jaclz_leave(r, acc);
}

// ------------------------------------------------- per-element wire-level operations
KYB_HD void zero_bytes(uint8_t* out, int n) {
    uint32_t* q = reinterpret_cast<uint32_t*>(out);
    for (int k = 0; k < n / 4; k++) q[k] = 0;
}
constexpr size_t G1_TAB_WORDS = 0;  // (pairing_abi.cuh: the G1 ladder keeps its table in private arrays -- VALU busy 0.95 as it is)
KYB_HD int g1_mul_wire(uint8_t* out, const uint8_t* scalar_be, const uint8_t* pt, uint32_t = 0, uint32_t* = nullptr) {
    g1_aff a;
    const int st = g1_decode(a, pt);
    if (st != ST_OK) {
        zero_bytes(out, 64);
        return st;
    }
    uint32_t k[8];
    words_from_be<8>(k, scalar_be);
    g1_jac p, r;
    jac_from_aff(p, a);
#ifdef KYB_BN_PACKED_LADDER
    g1_mul_glv(r, p, k);
#else
    g1_mul_glv_lz(r, p, k);
#endif
    jac_to_aff(a, r);
    g1_encode(out, a);
    return ST_OK;
}
// `tab`: this lane's table slab (G2_TAB_WORDS words of global memory) or nullptr (the tables in private arrays)
KYB_HD int g2_mul_wire(uint8_t* out, const uint8_t* scalar_be, const uint8_t* pt, uint32_t flags = 0, uint32_t* tab = nullptr) {
    g2_aff a;
    const int st = g2_decode_f(a, pt, flags, 0);
    if (st != ST_OK) {
        zero_bytes(out, 128);
        return st;
    }
    uint32_t k[8];
    words_from_be<8>(k, scalar_be);
    g2_jac p, r;
    jac_from_aff(p, a);
    // GLS needs a point of the order-n subgroup: every point a STRICT suite decodes, one the caller vouches for -- and on
    // bn256, whose UnmarshalBinary accepts the whole twist, one that passes the membership relation HERE (exact on this
    // curve: tests/test_constants.py; [u]Q + 4 additions, a third of the plain ladder's 256 doublings it saves).  Any
    // other point multiplies as the reference's double-and-add does, by the plain integer.
#ifdef KYB_BN_PACKED_LADDER
    if (CC::STRICT || flag_trusted(flags, 0) || g2_in_subgroup(a)) g2_mul_gls(r, p, k);
#else
    if (CC::STRICT || flag_trusted(flags, 0) || g2_in_subgroup(a)) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(KYB_BN_G2_TAB_SCRATCH)
        g2_mul_gls_lz<true>(r, p, k, tab);  // (device code: the kernel always passes a slab)
#else
        (void)tab;
        g2_mul_gls_lz<false>(r, p, k);
#endif
    }
#endif
    else jac_mul_u256(r, p, k);
    jac_to_aff(a, r);
    g2_encode(out, a);
    return ST_OK;
}
// out = Marshal(Unmarshal(in)): pointG1/pointG2.UnmarshalBinary (pairing/bn256/point.go:206-238, 466-499): coordinates
// < p, on the curve (G2: on the twist, no subgroup check), all-zero bytes = infinity.
KYB_HD int g1_unmarshal_wire(uint8_t* out, const uint8_t* pt, uint32_t = 0) {
    g1_aff a;
    const int st = g1_decode(a, pt);
    if (st != ST_OK) {
        zero_bytes(out, 64);
        return st;
    }
    g1_encode(out, a);
    return ST_OK;
}
KYB_HD int g2_unmarshal_wire(uint8_t* out, const uint8_t* pt, uint32_t flags = 0) {
    g2_aff a;
    const int st = g2_decode_f(a, pt, flags, 0);
    if (st != ST_OK) {
        zero_bytes(out, 128);
        return st;
    }
    g2_encode(out, a);
    return ST_OK;
}
// out = a + b   (Point.Add: kilic/g1.go:90-96, pairing/bn256/point.go:130-140 -> curve.go:69)
KYB_HD int g1_add_wire(uint8_t* out, const uint8_t* pa, const uint8_t* pb) {
    g1_aff a, b;
    int st = g1_decode(a, pa);
    const int st2 = g1_decode(b, pb);
    if (st == ST_OK) st = st2;
    if (st != ST_OK) {
        zero_bytes(out, 64);
        return st;
    }
    g1_jac p, q, r;
    jac_from_aff(p, a);
    jac_from_aff(q, b);
    jac_add(r, p, q);
    jac_to_aff(a, r);
    g1_encode(out, a);
    return ST_OK;
}
// (operands of Add are point objects, validated when they were unmarshalled: no subgroup re-check on a STRICT suite)
KYB_HD int g2_add_wire(uint8_t* out, const uint8_t* pa, const uint8_t* pb) {
    g2_aff a, b;
    int st = g2_decode(a, pa, false);
    const int st2 = g2_decode(b, pb, false);
    if (st == ST_OK) st = st2;
    if (st != ST_OK) {
        zero_bytes(out, 128);
        return st;
    }
    g2_jac p, q, r;
    jac_from_aff(p, a);
    jac_from_aff(q, b);
    jac_add(r, p, q);
    jac_to_aff(a, r);
    g2_encode(out, a);
    return ST_OK;
}

// ------------------------------------------------- the suite's policies (pairing_abi.cuh)
// What the shared batch kernels, the fixed-base traits and the C-ABI entry points need from a group, as static members that
// forward to the functions above (a kernel's template argument is the group policy; the fixed-base policy is a member type).
struct G1 {
    using F = fp;
    using Fb = fb_g1_policy;
    static constexpr bool IS_G2 = false;
    static constexpr size_t POINT = 64;                 // wire size (this suite has one form)
    static constexpr size_t TAB_WORDS = G1_TAB_WORDS;   // per-lane table slab of the ladder, in (WS_TAB, stream)
    static constexpr int WS_TAB = WS_G1TAB;
    static constexpr int MUL_WAVES = KYB_BN_MUL_WAVES;  // register budget of group_mul_kernel<G1> in waves per SIMD
    static constexpr bool decode_proves_subgroup() { return true; }
    KYB_HD static size_t wire_size(uint32_t flags) { return g1_wire_size(flags); }
    KYB_HD static size_t out_size(uint32_t flags) { return g1_out_size(flags); }
    KYB_HD static int mul_wire(uint8_t* out, const uint8_t* k, const uint8_t* pt, uint32_t flags, uint32_t* tab) { return g1_mul_wire(out, k, pt, flags, tab); }
    KYB_HD static int unmarshal_wire(uint8_t* out, const uint8_t* pt, uint32_t flags) { return g1_unmarshal_wire(out, pt, flags); }
    KYB_HD static int add_wire(uint8_t* out, const uint8_t* a, const uint8_t* b) { return g1_add_wire(out, a, b); }
    KYB_HD static int decode(g1_aff& a, const uint8_t* in, uint32_t flags) { return g1_decode_f(a, in, flags, 0); }  // UnmarshalBinary's checks (bdn.cuh)
    KYB_HD static void encode(uint8_t* out, const g1_aff& a, uint32_t flags) { g1_encode_f(out, a, flags); }
    KYB_HD static void scalar_from_be(uint32_t (&k)[8], const uint8_t* in) { KYB_BN_NS::scalar_from_be(k, in); }
    static void generator(g1_aff& a) {
        fp_const(a.x, CC::G1X);
        fp_const(a.y, CC::G1Y);
        a.inf = false;
    }
};
struct G2 {
    using F = fp2;
    using Fb = fb_g2_policy;
    static constexpr bool IS_G2 = true;
    static constexpr size_t POINT = 128;
    static constexpr size_t TAB_WORDS = G2_TAB_WORDS;
    static constexpr int WS_TAB = WS_G2TAB;
    static constexpr int MUL_WAVES = KYB_BN_MUL_WAVES;
    static constexpr bool decode_proves_subgroup() { return g2_decode_proves_subgroup(); }
    KYB_HD static size_t wire_size(uint32_t flags) { return g2_wire_size(flags); }
    KYB_HD static size_t out_size(uint32_t flags) { return g2_out_size(flags); }
    KYB_HD static int mul_wire(uint8_t* out, const uint8_t* k, const uint8_t* pt, uint32_t flags, uint32_t* tab) { return g2_mul_wire(out, k, pt, flags, tab); }
    KYB_HD static int unmarshal_wire(uint8_t* out, const uint8_t* pt, uint32_t flags) { return g2_unmarshal_wire(out, pt, flags); }
    KYB_HD static int add_wire(uint8_t* out, const uint8_t* a, const uint8_t* b) { return g2_add_wire(out, a, b); }
    KYB_HD static int decode(g2_aff& a, const uint8_t* in, uint32_t flags) { return g2_decode_f(a, in, flags, 0); }  // UnmarshalBinary's checks (bdn.cuh)
    KYB_HD static void encode(uint8_t* out, const g2_aff& a, uint32_t flags) { g2_encode_f(out, a, flags); }
    KYB_HD static void scalar_from_be(uint32_t (&k)[8], const uint8_t* in) { KYB_BN_NS::scalar_from_be(k, in); }
    static void generator(g2_aff& a) {
        fp2_load_const<TC>(a.x, CC::G2X);
        fp2_load_const<TC>(a.y, CC::G2Y);
        a.inf = false;
    }
};
struct Suite {
    using FC = KYB_BN_NS::FC;
    using G1 = KYB_BN_NS::G1;
    using G2 = KYB_BN_NS::G2;
    static constexpr int FB_SUITE = KYB_BN_FB_SUITE;  // the suite's index among the fixed-base workspace kinds (WS_FB + 2 * suite + group)
    static constexpr size_t GT_SIZE = 384;
#if defined(__HIPCC__)
    // The dispatch hooks of mul_dev / unmarshal_dev.  The lane machine of bls12381_lvm.cuh has no BN programs yet and
    // there are no small-batch kernels: every element goes to the per-lane kernels, unmasked.
    static int lvm_mul(bool, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint32_t, hipStream_t, const uint8_t** only,
                       bool* handled) {
        *only = nullptr;
        *handled = false;
        return KYB_OK;
    }
    static int unmarshal_small(bool, size_t, const uint8_t*, uint8_t*, uint8_t*, uint32_t, hipStream_t, bool* handled) {
        *handled = false;
        return KYB_OK;
    }
#endif
};
}  // namespace KYB_BN_NS
}  // namespace kyb
