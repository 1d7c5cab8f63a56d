// GF(2^255-19) on nine signed limbs in uniform radix 2^29: the field type of the variable-base ladder
// (ed25519_mul_kernel).  Every other user keeps the ten-limb `fe` of fe25519.cuh; the functions here are overloads
// of the same names, so the point formulas of ge25519.cuh and the ladder of ed25519_dev.cuh are written once.
//
// An element is sum v[i] 2^(29 i), any representative of its class of magnitude below 2^261, with
// 2^261 = 2^6 2^255 = 64 * 19 = 1216 (mod p).  Nine limbs make a product 81 v_mad_i64_i32 where ten make 100, and a
// uniform radix has no doubled odd x odd terms and no operand premultiplied by 19.  The columns 9 .. 16 of the
// schoolbook product are summed each on its own, as 64-bit words H_k that take no carry in, and folded as words:
// H = hi 2^32 + lo with lo the low word unsigned and hi = H >> 32 signed, and 2^32 = 8 * 2^29, so
//     2^(29 k) H_k  =  2^(29 (k - 9)) 1216 lo  +  2^(29 (k - 8)) 9728 hi   (mod p):
// low column j takes 1216 * lo(H_(j+9)) (j < 8, one v_mad_u64_u32) and 9728 * hi(H_(j+8)) (j > 0, one v_mad_i64_i32) --
// 81 + 16 = 97 multiply-adds, no 32-bit multiplication, and no chain, shift or mask on the high columns, against
// 100 + 9 on ten limbs.  (Premultiplying g by 1216 instead would make a column 1216 * 2^56 wide: DESIGN.md section 5
// item 16.)
//
// Bounds, in units of 2^28 per limb ("m"): a carried limb lies in [-2^28, 2^28) (limb 1 takes the last carry, at most
// 2^17, on top: m = 1.001), a decoded value has limbs in [0, 2^29): m = 2, sums add up.  A product f g needs
//     9 m_f m_g 2^56 + 2^44.6 + 2^35 < 2^63,   i.e.   m_f m_g <= 14.2
// (column 8: nine products, the fold terms below 1216 * 2^32 + 9728 * 2^31 < 2^44.6, the carry out of column 7 below
// 2^35; the even columns 0 .. 6 hold at most seven products, the same fold terms and a bias of 2^57).  A high column
// holds at most eight products, 8 m_f m_g 2^56 < 2^63 for m_f m_g < 16, and its high word fits 32 bits by construction.
// A squaring doubles its operand in 32 bits: m_f < 4.  FE29_MUL_LIMIT below is what the audit (KYB_FE_AUDIT,
// tests/test_fe29_host.py) holds the ladder to; its worst product is 3 x 3.
#pragma once
#include "fe25519.cuh"

namespace kyb {

struct fe29 {
    static constexpr int N = 9;
    int32_t v[9];
#if defined(KYB_FE_AUDIT)
    double mag = 2.0;  // host-only bound audit: limbs are below mag * 2^28 in magnitude
#endif
};

constexpr double FE29_MUL_LIMIT = 14.0;  // m_f * m_g (doubled for 2 f^2) of any product
constexpr double FE29_SQ_LIMIT = 3.99;   // m_f of a squaring (2 f in 32 bits)
constexpr int32_t FE29_MASK = (1 << 29) - 1;
constexpr int32_t FE29_FOLD = 1216;             // 2^261 mod p
constexpr int32_t FE29_FOLD_HI = 8 * FE29_FOLD;  // 2^(261 + 32) = 2^29 * 9728 mod p

#if defined(KYB_FE_AUDIT)
inline double& fe29_audit_max() {
    static double m = 0;
    return m;
}
inline double& fe29_audit_max_sq() {
    static double m = 0;
    return m;
}
inline void fe29_audit_note(double pf, double pg, double scale, bool sq) {
    const double x = pf * pg * scale;
    if (x > fe29_audit_max()) fe29_audit_max() = x;
    if (sq && pf > fe29_audit_max_sq()) fe29_audit_max_sq() = pf;
}
#define KYB_FE29_NOTE(pf, pg, scale, sq) fe29_audit_note(pf, pg, scale, sq)
#else
#define KYB_FE29_NOTE(pf, pg, scale, sq) ((void)0)
#endif

KYB_DEV void fe_0(fe29& h) {
#pragma unroll
    for (int i = 0; i < 9; i++) h.v[i] = 0;
    KYB_FE_MAG_SET(h, 0.0);
}
KYB_DEV void fe_1(fe29& h) {
    fe_0(h);
    h.v[0] = 1;
    KYB_FE_MAG_SET(h, 1.0 / (1 << 28));
}
KYB_DEV void fe_add(fe29& h, const fe29& f, const fe29& g) {
    const double m_ = KYB_FE_MAG(f) + KYB_FE_MAG(g);
#pragma unroll
    for (int i = 0; i < 9; i++) h.v[i] = f.v[i] + g.v[i];
    KYB_FE_MAG_SET(h, m_);
    (void)m_;
}
KYB_DEV void fe_sub(fe29& h, const fe29& f, const fe29& g) {
    const double m_ = KYB_FE_MAG(f) + KYB_FE_MAG(g);
#pragma unroll
    for (int i = 0; i < 9; i++) h.v[i] = f.v[i] - g.v[i];
    KYB_FE_MAG_SET(h, m_);
    (void)m_;
}
KYB_DEV void fe_neg(fe29& h, const fe29& f) {
    const double m_ = KYB_FE_MAG(f);
#pragma unroll
    for (int i = 0; i < 9; i++) h.v[i] = -f.v[i];
    KYB_FE_MAG_SET(h, m_);
    (void)m_;
}
// f = b ? g : f
KYB_DEV void fe_cmov(fe29& f, const fe29& g, bool b) {
#pragma unroll
    for (int i = 0; i < 9; i++) f.v[i] = b ? g.v[i] : f.v[i];
    KYB_FE_MAG_SET(f, KYB_FE_MAG(f) > KYB_FE_MAG(g) ? KYB_FE_MAG(f) : KYB_FE_MAG(g));  // either operand, whatever b
}
KYB_DEV void fe_cswap(fe29& f, fe29& g, bool b) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        int32_t x = f.v[i], y = g.v[i];
        f.v[i] = b ? y : x;
        g.v[i] = b ? x : y;
    }
    const double m_ = KYB_FE_MAG(f) > KYB_FE_MAG(g) ? KYB_FE_MAG(f) : KYB_FE_MAG(g);
    KYB_FE_MAG_SET(f, m_);
    KYB_FE_MAG_SET(g, m_);
    (void)m_;
}

// A fold multiplier (1216, 9728) as a value the compiler cannot see through: a 64-bit multiplication by the constant is
// otherwise strength-reduced into shifts and 64-bit adds, each of which costs what the multiply-add costs.
KYB_DEV int32_t fe29_fold(int32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(k));
#endif
    return k;
}

// Half-limb bias of the rounded carry chain, as in fe25519.cuh: a column enters the chain as T = t + 2^28, its carry is
// T >> 29 and its limb the low 29 bits minus 2^28.  Even columns are handed 2^28 + (2^28 << 29): the second term arrives
// in the odd column above as that column's bias, inside the carry.  Column 8 has no column above it.
KYB_DEV constexpr int64_t fe29_bias(int k) {
    return (k & 1) ? 0 : ((int64_t)1 << 28) + (k < 8 ? ((int64_t)1 << 57) : 0);
}

// One product, columns 0 .. 16: prod(k, addend) returns addend + (the products of column k).  Step k = 0 .. 8 first sums
// the high column H = column k + 9 (none for k = 8) from zero, then low column k onto its start value (the carry from
// below for an odd k, the bias for an even one), adds 1216 * (the low word of H, unsigned) and 9728 * (the high word of
// the step before's H, signed), the carry on an even k > 0, and cuts the limb: ONE rounded carry chain
// 0 -> 1 -> ... -> 8 -> (x 1216) 0 -> 1 (fe_chain_store of fe25519.cuh).  Only that high word lives across a step, and
// the two sums of a step do not depend on each other.
template <class ProdF>
KYB_DEV void fe29_fold_store(fe29& h, ProdF prod) {
    const int32_t fold = fe29_fold(FE29_FOLD), fold_hi = fe29_fold(FE29_FOLD_HI);
    int32_t r[9];
    int32_t hi = 0;
    int64_t c = 0;
    uint32_t b0 = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int64_t H = k < 8 ? prod(k + 9, (int64_t)0) : 0;
        int64_t T = prod(k, (k & 1) ? c : fe29_bias(k));
        if (k < 8) {
            T += (int64_t)((uint64_t)(uint32_t)H * (uint64_t)(uint32_t)fold);
            KYB_PIN64(T);
        }
        if (k > 0) {
            T += (int64_t)hi * (int64_t)fold_hi;
            KYB_PIN64(T);
        }
        if (k > 0 && !(k & 1)) T += c;
        hi = (int32_t)(H >> 32);
        c = T >> 29;
        if (k == 0)
            b0 = (uint32_t)T & (uint32_t)FE29_MASK;
        else
            r[k] = (int32_t)((uint32_t)T & (uint32_t)FE29_MASK) - (1 << 28);
    }
    const int64_t t0 = (int64_t)b0 + c * FE29_FOLD;
    c = t0 >> 29;
    r[0] = (int32_t)((uint32_t)t0 & (uint32_t)FE29_MASK) - (1 << 28);
    r[1] += (int32_t)c;
#pragma unroll
    for (int i = 0; i < 9; i++) h.v[i] = r[i];
}

// h = f * g   (81 products + 16 folds)
KYB_DEV void fe_mul(fe29& h, const fe29& f, const fe29& g) {
    KYB_FE29_NOTE(KYB_FE_MAG(f), KYB_FE_MAG(g), 1.0, false);
    fe29_fold_store(h, [&](int k, int64_t acc) {
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); i++) {
            acc += (int64_t)f.v[i] * (int64_t)g.v[k - i];
            KYB_PIN64(acc);
        }
        return acc;
    });
    KYB_FE_MAG_SET(h, 1.001);
}

// h = (DBL ? 2 : 1) * f^2   (45 products + 16 folds): off-diagonal products take 2 f_i, doubled once; 2 f^2 takes
// (2 f_i) (2 f_j) off the diagonal and (2 f_i) f_i on it
template <bool DBL>
KYB_DEV void fe29_sq_t(fe29& h, const fe29& f) {
    KYB_FE29_NOTE(KYB_FE_MAG(f), KYB_FE_MAG(f), DBL ? 2.0 : 1.0, true);
    int32_t f2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) f2[i] = 2 * f.v[i];
    fe29_fold_store(h, [&](int k, int64_t acc) {
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); 2 * i <= k; i++) {
            const int j = k - i;
            const int32_t a = (i == j && !DBL) ? f.v[i] : f2[i];
            const int32_t b = (i == j || !DBL) ? f.v[j] : f2[j];
            acc += (int64_t)a * (int64_t)b;
            KYB_PIN64(acc);
        }
        return acc;
    });
    KYB_FE_MAG_SET(h, 1.001);
}
KYB_DEV void fe_sq(fe29& h, const fe29& f) { fe29_sq_t<false>(h, f); }
KYB_DEV void fe_sq2(fe29& h, const fe29& f) { fe29_sq_t<true>(h, f); }

// Limbs from eight little-endian words; bit 255 is ignored (fe.go:91).
KYB_DEV void fe_fromwords(fe29& h, const uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int o = 29 * i, j = o / 32, s = o % 32;
        uint32_t x = w[j] >> s;
        if (s + 29 > 32 && j + 1 < 8) x |= w[j + 1] << (32 - s);
        h.v[i] = (int32_t)(x & (uint32_t)(i < 8 ? FE29_MASK : (1 << 23) - 1));
    }
    KYB_FE_MAG_SET(h, 2.0);
}
// Canonical little-endian bytes as eight 32-bit words, for limbs of at most 7 * 2^28 in magnitude.
KYB_DEV void fe_towords(uint32_t w[8], const fe29& f) {
    int32_t h[9];
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] = f.v[i];
    // twice: limbs 0 .. 7 to [0, 2^29), the bits from 2^255 up folded into limb 0 times 19.  The first pass leaves
    // -2^13 < h < 2^255 + 2^13, the second 0 <= h < 2^255 with limb 0 in [-19, 2^29 + 19).
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            h[i + 1] += h[i] >> 29;
            h[i] &= FE29_MASK;
        }
        h[0] += 19 * (h[8] >> 23);
        h[8] &= (1 << 23) - 1;
    }
    // q = floor((h + 19) / 2^255) limb by limb: 1 exactly when h >= p
    int32_t q = (h[0] + 19) >> 29;
#pragma unroll
    for (int i = 1; i < 8; i++) q = (h[i] + q) >> 29;
    q = (h[8] + q) >> 23;
    h[0] += 19 * q;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h[i + 1] += h[i] >> 29;
        h[i] &= FE29_MASK;
    }
    h[8] &= (1 << 23) - 1;  // drop 2^255 * q
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int o = 29 * i, j = o / 32, s = o % 32;
        w[j] |= (uint32_t)h[i] << s;
        if (s + 29 > 32 && j + 1 < 8) w[j + 1] |= (uint32_t)h[i] >> (32 - s);
    }
}
KYB_DEV bool fe_isnegative(const fe29& f) {
    uint32_t w[8];
    fe_towords(w, f);
    return w[0] & 1;
}
KYB_DEV bool fe_isnonzero(const fe29& f) {
    uint32_t w[8];
    fe_towords(w, f);
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) r |= w[i];
    return r != 0;
}

// To and from the ten-limb type, through the canonical words: both happen once per element (the parked triple of
// store_proj), where 150 instructions do not show; the result is the decoded form of either type.
KYB_DEV void fe29_to_fe(fe& h, const fe29& f) {
    uint32_t w[8];
    fe_towords(w, f);
    fe_fromwords(h, w);
}
KYB_DEV void fe29_from_fe(fe29& h, const fe& f) {
    uint32_t w[8];
    fe_towords(w, f);
    fe_fromwords(h, w);
}

}  // namespace kyb
