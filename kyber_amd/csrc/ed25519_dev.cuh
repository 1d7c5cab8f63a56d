// Ed25519 device functions shared by the translation units that run ladders and combs (ed25519.hip: the tuned
// multiplication kernels; ed25519_verify.hip: fused signature verification and a*P + b*Q): table geometry, the
// fixed-base row selection, the per-lane window tables and the signed radix-16 ladder, the parked (X, Y, Z) triples of
// the shared-inversion encoder.  Kernels stay in their units: an out-of-line callee takes the loosest register budget
// of the kernels that reach it, so units do not share kernels, only inlined code.
// Like the other arithmetic headers this one also compiles with g++ (tests/ed_verify_harness.cpp).
#pragma once
#include "ge25519.cuh"

#if !defined(__HIPCC__)
#include <type_traits>
// host build: the vector types of the HIP runtime that the table accessors use
struct int4 { int32_t x, y, z, w; };
struct uint4 { uint32_t x, y, z, w; };
inline int4 make_int4(int32_t x, int32_t y, int32_t z, int32_t w) { return int4{x, y, z, w}; }
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
#define KYB_DEV_CONST static
#else
#define KYB_DEV_CONST __device__
#endif

namespace kyb {

// Fixed-base table: entry (pos, j) = (j + 1) * 256^pos * B in affine (y+x, y-x, 2dxy) form, j < 136: a signed
// radix-256 digit is d0 + 16 d1 of two signed radix-16 digits in [-8, 8], so |digit| <= 136.  One entry is one
// 128-byte line (30 limbs + 2 pad words); the 574 KB table is read through L2 -- it does not fit LDS, but it
// halves the additions of the reference's 32 x 8 table (ge.go:373-417: 64 additions + 4 doublings) to 32.
constexpr int ED_TAB_POS = 33;  // 32 byte positions + 2^256*B for the 65th radix-16 digit
constexpr int ED_TAB_ENT = 136;
constexpr int ED_TAB_STRIDE = 32;
constexpr int ED_TAB_WORDS = ED_TAB_POS * ED_TAB_ENT * ED_TAB_STRIDE;

// Comb of G signed radix-16 digits per position: D_k = sum_{i < G} e[G k + i] 16^i, |D_k| <= 8 (16^G - 1) / 15, and
// position k holds j 16^(G k) B for j = 1 .. ENT.  G = 2 is the radix-256 table above (its last position keeps all
// 136 rows); the standard base also gets a wide comb, G = ED_COMB_G, whose last position holds only the rows that the
// digits left for it can reach.
template <int G>
struct EdComb {
    static constexpr int POS = (65 + G - 1) / G;           // positions for all 65 digits (KYB_F_VARTIME)
    static constexpr int POS_CT = (64 + G - 1) / G;        // ... for the 64 of the constant-structure recoding
    static constexpr int ENT = 8 * ((1 << (4 * G)) - 1) / 15;
    static constexpr int LAST_D = 65 - G * (POS - 1);      // digits of the last position
    static constexpr int LAST_ENT = 8 * ((1 << (4 * LAST_D)) - 1) / 15;
    static constexpr int ROWS = (POS - 1) * ENT + LAST_ENT;
};
// Radix 2^16: 16 additions instead of 32 for a 72 MB table, which stays in the Infinity Cache.
#ifndef ED_COMB_G
#define ED_COMB_G 4
#endif
using EdWide = EdComb<ED_COMB_G>;
constexpr size_t ED_WIDE_WORDS = (size_t)EdWide::ROWS * ED_TAB_STRIDE;

KYB_DEV void load_words8(uint32_t w[8], const uint32_t* __restrict__ p) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0];
    const uint4 b = reinterpret_cast<const uint4*>(p)[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
KYB_DEV void store_words8(uint32_t* __restrict__ p, const uint32_t w[8]) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// element i of a batch whose offsets the caller vouches for: a decreasing pair is an empty element.  A template, so that
// a translation unit that defines a plain function of this name and signature after `using namespace kyb` compiles and
// calls its own (a plain function is the better match; two plain ones would be ambiguous).
template <class = void>
KYB_HD uint64_t element_len(const uint64_t* __restrict__ off, size_t i) {
    const uint64_t a = off[i], b = off[i + 1];
    return b >= a ? b - a : 0;
}

// Row t = (pos, j) of a comb table of the base B: (j+1) * 16^(G pos) * B by MSB-first double-and-add, stored in affine
// (y+x, y-x, 2dxy) form, 30 limbs + 2 pad words (ed25519_build_base_table_kernel; the host harness of the verify
// program fills the rows it reads with the same code).
template <int G>
KYB_DEV void ed_comb_row(int32_t* __restrict__ o, int t, const ge_p3& B) {
    constexpr int ENT = EdComb<G>::ENT;
    const int pos = t / ENT, j = t - pos * ENT;
    ge_cached cB;
    ge_p3_to_cached(cB, B);
    ge_p3 acc;
    ge_p3_0(acc);
    ge_p1p1 r;
    // multiplier = (j+1) << (4G*pos): 4G significant bits then 4G*pos doublings
#pragma unroll 1
    for (int bit = 4 * G - 1; bit >= 0; bit--) {
        ge_dbl(r, acc.X, acc.Y, acc.Z);
        ge_p1p1_to_p3(acc, r);
        if (((j + 1) >> bit) & 1) {
            ge_add(r, acc, cB);
            ge_p1p1_to_p3(acc, r);
        }
    }
#pragma unroll 1
    for (int k = 0; k < 4 * G * pos; k++) {
        ge_dbl(r, acc.X, acc.Y, acc.Z);
        ge_p1p1_to_p3(acc, r);
    }
    fe zi, x, y, ypx, ymx, xy2d, z;
    fe_invert(zi, acc.Z);
    fe_mul(x, acc.X, zi);
    fe_mul(y, acc.Y, zi);
    fe_add(ypx, y, x);
    fe_sub(ymx, y, x);
    fe_mul(xy2d, x, y);
    fe_mul(xy2d, xy2d, fe_d2());
    // one pass through mul-by-one normalises y+x / y-x to reduced limbs
    fe_1(z);
    fe_mul(ypx, ypx, z);
    fe_mul(ymx, ymx, z);
#pragma unroll
    for (int l = 0; l < 10; l++) {
        o[l] = ypx.v[l];
        o[10 + l] = ymx.v[l];
        o[20 + l] = xy2d.v[l];
    }
    o[30] = o[31] = 0;
}

// ------------------------------------------------------ deferred encoding (batched inversion)
// The field inversion of ToBytes (254 squarings, 22 % of a fixed-base and 6 % of a variable-base
// multiplication) is amortised: the multiplication kernels park (X, Y, Z) in HBM (30 limbs, 120 B per
// element) and a second kernel inverts ENC_CHUNK Z's per lane with Montgomery's trick -- 3 multiplications
// per element plus 1/ENC_CHUNK of an inversion -- before encoding.
// Ownership is interleaved: a block of B lanes owns B * ENC_CHUNK consecutive points and lane t takes the points
// base + t + j B, j < ENC_CHUNK, so every load and every emit of a wave covers 64 consecutive records (lane-contiguous
// chunks put the records of one load of a wave 120 B * ENC_CHUNK apart).  The chunk also sets how many waves a batch
// makes -- 2^20 points are 1 024 waves at chunk 16, one per SIMD, and 2 048 at chunk 8 -- and every wave pays a whole
// inversion.  Measured at 2^20 points with the prefixes in LDS: 124 us at chunk 16, 167 us at chunk 8, whatever the
// block size (64 or 128 at chunk 16, 64 to 256 at chunk 8); lane-contiguous chunks of 16 with the prefixes in scratch took 196 us.  The second wave
// of a SIMD does not buy back its own inversion.
constexpr int ENC_CHUNK = 16;

KYB_DEV void store_proj(int32_t* __restrict__ proj, size_t idx, const ge_p3& h) {
    int32_t* o = proj + idx * 30;
#pragma unroll
    for (int l = 0; l < 10; l++) {
        o[l] = h.X.v[l];
        o[10 + l] = h.Y.v[l];
        o[20 + l] = h.Z.v[l];
    }
}
// the ladder on fe29 parks the same ten-limb triple: the encoder does not know which field type made it
KYB_DEV void store_proj(int32_t* __restrict__ proj, size_t idx, const ge29_p2& h) {
    ge_p3 t;
    fe29_to_fe(t.X, h.X);
    fe29_to_fe(t.Y, h.Y);
    fe29_to_fe(t.Z, h.Z);
    store_proj(proj, idx, t);
}
KYB_DEV void store_proj(int32_t* __restrict__ proj, size_t idx, const ge29_p3& h) {
    store_proj(proj, idx, ge29_p2{h.X, h.Y, h.Z});
}
KYB_DEV void load_fe(fe& f, const int32_t* __restrict__ p) {
#pragma unroll
    for (int l = 0; l < 10; l++) f.v[l] = p[l];
}
// Where a lane keeps its prefix products Z_0 ... Z_j between the two passes.  In the lane's private memory they are
// written and then read back in reverse through the dword-interleaved scratch path; in LDS, laid out
// [j][limb][lane], every access of a wave is 64 consecutive words: no bank conflict, 40 B * ENC_CHUNK per lane.
struct EncPreScratch {
    fe pre[ENC_CHUNK];
    KYB_DEV void put(int j, const fe& f) { pre[j] = f; }
    KYB_DEV void get(fe& f, int j) const { f = pre[j]; }
};
template <int LANES>
struct EncPreLds {
    int32_t* col;  // this lane's column: block's array + threadIdx.x
    static constexpr int WORDS = ENC_CHUNK * 10 * LANES;
    KYB_DEV void put(int j, const fe& f) {
#pragma unroll
        for (int l = 0; l < 10; l++) col[(j * 10 + l) * LANES] = f.v[l];
    }
    KYB_DEV void get(fe& f, int j) const {
#pragma unroll
        for (int l = 0; l < 10; l++) f.v[l] = col[(j * 10 + l) * LANES];
        KYB_FE_MAG_SET(f, 1.01);
    }
};
// One lane of the shared-inversion encoder: the canonical encodings of its parked triples, one field inversion for
// all of them; emit(i, w) receives point i's eight words.  The lane owns the records first + j * stride,
// j < ENC_CHUNK / GROUP, that are below n; a record is GROUP consecutive points (point i at proj + 30 i), so n * GROUP
// points are parked.  A kernel passes first = blockIdx.x * blockDim.x * (ENC_CHUNK / GROUP) + threadIdx.x and
// stride = blockDim.x (ed_encode_grid in ed25519_launch.h sizes the grid for that).  The points are emitted from the
// lane's last to its first: record by record downwards, and within a record point GROUP - 1 first.
#if defined(__HIPCC__)
template <int GROUP = 1>
KYB_DEV size_t ed_encode_first() {
    return (size_t)blockIdx.x * blockDim.x * (ENC_CHUNK / GROUP) + threadIdx.x;
}
#endif
template <int GROUP = 1, class Pre, class Emit>
KYB_DEV void ed_encode_chunk(size_t n, const int32_t* __restrict__ proj, size_t first, size_t stride, Pre& pre, Emit emit) {
    // (GROUP = 3, share/vss's seal: five records, 15 of the lane's 16 slots)
    static_assert(GROUP >= 1 && GROUP <= ENC_CHUNK, "whole records per lane");
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < ENC_CHUNK / GROUP; r++) cnt += (first + r * stride < n) ? GROUP : 0;
    if (cnt == 0) return;
    auto point = [&](int j) { return (first + (size_t)(j / GROUP) * stride) * GROUP + (size_t)(j % GROUP); };
    fe z, acc;
    load_fe(acc, proj + point(0) * 30 + 20);
    pre.put(0, acc);  // pre[j] = Z_0 ... Z_j
#pragma unroll 1
    for (int j = 1; j < cnt; j++) {
        load_fe(z, proj + point(j) * 30 + 20);
        fe_mul(acc, acc, z);
        pre.put(j, acc);
    }
    fe inv;
    fe_invert(inv, acc);  // 1 / (Z_0 ... Z_{cnt-1})
#pragma unroll 1
    for (int j = cnt - 1; j >= 0; j--) {
        const size_t i = point(j);
        fe zi, X, Y;
        load_fe(z, proj + i * 30 + 20);
        if (j > 0) {
            pre.get(zi, j - 1);
            fe_mul(zi, inv, zi);  // 1 / Z_j
            fe_mul(inv, inv, z);
        } else {
            zi = inv;
        }
        load_fe(X, proj + i * 30);
        load_fe(Y, proj + i * 30 + 10);
        uint32_t w[8];
        ge_encode_with_zinv(w, X, Y, zi);
        emit(i, w);
    }
}

// ------------------------------------------------------------ fixed-base mul
// Every lane gathers its own 128-byte entry (eight 16-byte loads from one line, served by L2 / the Infinity Cache).
template <int ENT>
KYB_DEV void select_precomp_tab(ge_precomp& t, const int32_t* __restrict__ tab, int pos, int b) {
    const bool neg = b < 0;
    const int babs = neg ? -b : b;
    const int4* e = reinterpret_cast<const int4*>(tab + (size_t)(pos * ENT + (babs ? babs - 1 : 0)) * ED_TAB_STRIDE);
    int32_t w[32];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int4 x = e[i];
        w[4 * i] = x.x;
        w[4 * i + 1] = x.y;
        w[4 * i + 2] = x.z;
        w[4 * i + 3] = x.w;
    }
#pragma unroll
    for (int l = 0; l < 10; l++) {
        t.ypx.v[l] = w[l];
        t.ymx.v[l] = w[10 + l];
        t.xy2d.v[l] = w[20 + l];
    }
    if (babs == 0) {  // identity: (1, 1, 0)
        fe_1(t.ypx);
        fe_1(t.ymx);
        fe_0(t.xy2d);
    }
    ge_precomp_cneg(t, neg);
}

// recode16's digits e[0..63] + 8 as 64 nibbles, digit i in bits 4i .. 4i + 3 of the 256-bit word.  Indexing e[] by a
// loop counter compiles to a select over all 65 digits (e[] lives in registers); a loop shifts the pack instead and
// reads its digit from one end as nibble - 8.  That holds for digits in [-8, 7]: all of e[0..62], and e[63] under
// KYB_F_VARTIME.  On the constant-structure path e[63] may be 8 (scalars >= 2^255), which does not fit, and e[64] is
// not packed: whoever needs these two takes them from e[] by constant index.
KYB_DEV void ed_pack_digits(uint32_t pk[8], const int8_t e[65]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        pk[j] = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) pk[j] |= (uint32_t)((e[8 * j + q] + 8) & 15) << (4 * q);
    }
}

// The digits D_k = sum_{i < G} e[G k + i] 16^i of a comb of G radix-16 digits per position, handed out for
// k = 0, 1, 2, ... in that order.  Positions below PACKED hold digits of e[0..62] only: their D_k is the low 4G bits
// of the pack minus 8 (16^G - 1) / 15 -- the 8 taken off every nibble -- and the pack moves down by 4G bits.  The one
// or two positions that hold e[63] or e[64] are formed once from e[] by constant index and picked by the position
// counter, which is uniform.  G = 1 hands out the digits themselves.
template <int G>
struct EdCombDigits {
    static_assert(G >= 1 && G <= 7, "a position's digits are read from one 32-bit word");
    static constexpr int PACKED = 63 / G;
    static constexpr int TAIL = EdComb<G>::POS - PACKED;
    uint32_t pk[8];
    int tail[TAIL];
    KYB_DEV explicit EdCombDigits(const int8_t e[65]) {
        ed_pack_digits(pk, e);
#pragma unroll
        for (int t = 0; t < TAIL; t++) {
            int d = 0;
#pragma unroll
            for (int i = G - 1; i >= 0; i--)
                if (G * (PACKED + t) + i <= 64) d = 16 * d + (int)e[G * (PACKED + t) + i];
            tail[t] = d;
        }
    }
    KYB_DEV int next(int k) {
        int d = (int)(pk[0] & ((1u << (4 * G)) - 1u)) - EdComb<G>::ENT;
#pragma unroll
        for (int j = 0; j < 7; j++) pk[j] = (pk[j] >> (4 * G)) | (pk[j + 1] << (32 - 4 * G));
        pk[7] >>= 4 * G;
#pragma unroll
        for (int t = 0; t < TAIL; t++)
            if (k == PACKED + t) d = tail[t];
        return d;
    }
};

// One lane of the fixed-base comb: h = sum_k D_k 16^(G k) B from the table `tab` of B (ed25519_mul_base_kernel<G>).
// Position 0's row is the walk's first point as it stands (a zero digit: the identity row, (0 : 2 : 2 : 0)): one product
// for its T, where a mixed addition to the identity and its conversion took seven.  full: KYB_F_VARTIME's digits, and a
// position at which no lane of the wave has anything to add is passed over.
template <int G>
KYB_DEV void ed_comb_walk(ge_p3& h, const int8_t e[65], bool full, const int32_t* __restrict__ tab) {
    ge_precomp t;
    ge_p1p1 r;
    const int npos = full ? EdComb<G>::POS : EdComb<G>::POS_CT;  // uniform across the grid
    EdCombDigits<G> digits(e);  // (e[G * k + i] by the loop counter: a select over all 65 digits, G times a position)
    select_precomp_tab<EdComb<G>::ENT>(t, tab, 0, digits.next(0));
    ge_precomp_to_p3(h, t);
#pragma unroll 1
    for (int k = 1; k < npos; k++) {
        const int d = digits.next(k);
#if defined(__HIP_DEVICE_COMPILE__)
        if (full && __ballot(d != 0) == 0) continue;  // variable-time: nothing to add at this position in any lane
#endif
        select_precomp_tab<EdComb<G>::ENT>(t, tab, k, d);
        ge_madd(r, h, t);
        ge_p1p1_to_p3(h, r);
    }
}

// --------------------------------------------------------- variable-base mul
// Shared ladder: h = sum_i e[i] 16^i * A using an 8-entry cached table.  The table (8 x 160 B) is per-lane state
// that fits neither registers nor LDS at a useful occupancy.  Small batches keep it in the lane's private (scratch)
// memory; large ones in a global slab of 1280 contiguous bytes per lane: scratch is interleaved per dword across
// the lanes of a wave, so an *indexed* entry read drags in up to 8 rows per dword (measured: 40 GB fetched per 2^20
// launch for 11 GB of entries), while a lane-contiguous entry is ten 16-byte loads from two or three cache lines.
// Both tables are templates over the field type of their entries (ge25519.cuh); the plain names are the ten-limb ones.
template <class F = fe>
struct TabScratch_t {
    typedef typename ge_t<F>::cached cached;
    cached tab[8];
    KYB_DEV void put(int j, const cached& c) { tab[j] = c; }
    KYB_DEV void get(cached& c, int j) const { c = tab[j]; }
};
using TabScratch = TabScratch_t<>;
template <class F = fe>
struct TabGlobal_t;
using TabGlobal = TabGlobal_t<>;
// A lane's table in the slab, counted in int4 and in 32-bit words (the encoders write their bytes over its front)
constexpr size_t ED_TAB_INT4 = sizeof(TabScratch) / 16;
constexpr size_t ED_TAB_WORDS32 = sizeof(TabScratch) / 4;
template <>
struct TabGlobal_t<fe> {
    int4* base;  // this lane's 8 x 10 int4
    KYB_DEV void put(int j, const ge_cached& c) {
        int4* q = base + j * 10;
        const fe* f[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
        int32_t w[40];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int l = 0; l < 10; l++) w[10 * k + l] = f[k]->v[l];
#pragma unroll
        for (int i = 0; i < 10; i++) q[i] = make_int4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
    KYB_DEV void get(ge_cached& c, int j) const {
        const int4* q = base + j * 10;
        int32_t w[40];
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const int4 x = q[i];
            w[4 * i] = x.x;
            w[4 * i + 1] = x.y;
            w[4 * i + 2] = x.z;
            w[4 * i + 3] = x.w;
        }
        fe* f[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int l = 0; l < 10; l++) f[k]->v[l] = w[10 * k + l];
    }
    // b * A for a signed digit b in [-8, 8], the sign and the zero taken by the load address instead of selects:
    // -q = (Y-X, Y+X, Z, -2dT) reads Y+X and Y-X from swapped offsets (8-byte loads: the two fields meet inside a
    // 16-byte word), b = 0 reads the identity entry, and -2dT is negated by mask.
    KYB_DEV void get_signed(ge_cached& c, int b) const;
};
KYB_DEV_CONST __attribute__((aligned(16))) const int32_t ED_CACHED_IDENTITY[40] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                                                               1, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                                                               1};  // (1, 1, 1, 0)
KYB_DEV void TabGlobal_t<fe>::get_signed(ge_cached& c, int b) const {
    const bool neg = b < 0;
    const int babs = neg ? -b : b;
    // both candidates are global memory: say so, or the selected pointer is loaded through flat instructions
#if defined(__HIPCC__)
    typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    using gint = const __attribute__((address_space(1))) int32_t;
    using gint2 = const __attribute__((address_space(1))) i32x2;
    using gint4 = const __attribute__((address_space(1))) i32x4;
#else
    struct i32x2 { int32_t x, y; };
    struct i32x4 { int32_t x, y, z, w; };
    using gint = const int32_t;
    using gint2 = const i32x2;
    using gint4 = const i32x4;
#endif
    gint* e = babs ? (gint*)(base + (babs - 1) * 10) : (gint*)ED_CACHED_IDENTITY;
    gint2* p = (gint2*)(e + (neg ? 10 : 0));
    gint2* m = (gint2*)(e + (neg ? 0 : 10));
    gint4* q = (gint4*)(e + 20);
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const i32x2 x = p[i], y = m[i];
        c.YpX.v[2 * i] = x.x;
        c.YpX.v[2 * i + 1] = x.y;
        c.YmX.v[2 * i] = y.x;
        c.YmX.v[2 * i + 1] = y.y;
    }
    int32_t w[20];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const i32x4 x = q[i];
        w[4 * i] = x.x;
        w[4 * i + 1] = x.y;
        w[4 * i + 2] = x.z;
        w[4 * i + 3] = x.w;
    }
    const int32_t s = -(int32_t)neg;
#pragma unroll
    for (int l = 0; l < 10; l++) {
        c.Z.v[l] = w[l];
        c.T2d.v[l] = (w[10 + l] ^ s) - s;
    }
}
// The nine-limb entry: 36 words, nine 16-byte loads, inside the same 80 int4 per lane (entry j at base + 9 j).  Words:
//   0 .. 7  (Y+X)[0 .. 7]    8 .. 15  (Y-X)[0 .. 7]    16, 17  (Y+X)[8], (Y-X)[8]    18 .. 26  Z    27 .. 35  2dT
// so that -q reads its Y+X and Y-X as the same four aligned 16-byte loads from swapped offsets; the two top limbs
// share a word with Z[0 .. 1] and are swapped by two selects.
template <>
struct TabGlobal_t<fe29> {
    int4* base;  // this lane's 80 int4, 8 x 9 of them used
    static constexpr int word(int field, int l) { return field < 2 ? (l < 8 ? 8 * field + l : 16 + field) : 18 + 9 * (field - 2) + l; }
    KYB_DEV void put(int j, const ge29_cached& c) {
        int4* q = base + j * 9;
        const fe29* f[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
        int32_t w[36];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int l = 0; l < 9; l++) w[word(k, l)] = f[k]->v[l];
#pragma unroll
        for (int i = 0; i < 9; i++) q[i] = make_int4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
    KYB_DEV void get(ge29_cached& c, int j) const {
        const int4* q = base + j * 9;
        int32_t w[36];
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const int4 x = q[i];
            w[4 * i] = x.x;
            w[4 * i + 1] = x.y;
            w[4 * i + 2] = x.z;
            w[4 * i + 3] = x.w;
        }
        fe29* f[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int l = 0; l < 9; l++) f[k]->v[l] = w[word(k, l)];
        KYB_FE_MAG_SET(c.YpX, 3.001);  // entry 0 is Y + X of the decoded point: 2 + 1.001
        KYB_FE_MAG_SET(c.YmX, 3.001);
        KYB_FE_MAG_SET(c.Z, 1.001);
        KYB_FE_MAG_SET(c.T2d, 1.001);
    }
    // b * A for a signed digit b in [-8, 8], the sign and the zero taken by the load address (TabGlobal_t<fe> above)
    KYB_DEV void get_signed(ge29_cached& c, int b) const;
};
KYB_DEV_CONST __attribute__((aligned(16))) const int32_t ED_CACHED_IDENTITY29[36] = {1, 0, 0, 0, 0, 0, 0, 0,
                                                                                 1, 0, 0, 0, 0, 0, 0, 0,
                                                                                 0, 0, 1};  // (1, 1, 1, 0)
KYB_DEV void TabGlobal_t<fe29>::get_signed(ge29_cached& c, int b) const {
    const bool neg = b < 0;
    const int babs = neg ? -b : b;
#if defined(__HIPCC__)
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    using gint = const __attribute__((address_space(1))) int32_t;
    using gint4 = const __attribute__((address_space(1))) i32x4;
#else
    struct i32x4 { int32_t x, y, z, w; };
    using gint = const int32_t;
    using gint4 = const i32x4;
#endif
    gint* e = babs ? (gint*)(base + (babs - 1) * 9) : (gint*)ED_CACHED_IDENTITY29;
    gint4* p = (gint4*)(e + (neg ? 8 : 0));
    gint4* m = (gint4*)(e + (neg ? 0 : 8));
    gint4* q = (gint4*)(e + 16);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const i32x4 x = p[i], y = m[i];
        c.YpX.v[4 * i] = x.x;
        c.YpX.v[4 * i + 1] = x.y;
        c.YpX.v[4 * i + 2] = x.z;
        c.YpX.v[4 * i + 3] = x.w;
        c.YmX.v[4 * i] = y.x;
        c.YmX.v[4 * i + 1] = y.y;
        c.YmX.v[4 * i + 2] = y.z;
        c.YmX.v[4 * i + 3] = y.w;
    }
    int32_t w[20];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const i32x4 x = q[i];
        w[4 * i] = x.x;
        w[4 * i + 1] = x.y;
        w[4 * i + 2] = x.z;
        w[4 * i + 3] = x.w;
    }
    c.YpX.v[8] = neg ? w[1] : w[0];
    c.YmX.v[8] = neg ? w[0] : w[1];
    const int32_t s = -(int32_t)neg;
#pragma unroll
    for (int l = 0; l < 9; l++) {
        c.Z.v[l] = w[2 + l];
        c.T2d.v[l] = (w[11 + l] ^ s) - s;
    }
    KYB_FE_MAG_SET(c.YpX, 3.001);
    KYB_FE_MAG_SET(c.YmX, 3.001);
    KYB_FE_MAG_SET(c.Z, 1.001);
    KYB_FE_MAG_SET(c.T2d, 1.001);
}
template <bool UNI = false, class C, class Tab>
KYB_DEV void select_cached(C& c, const Tab& tab, int b) {
    typedef decltype(c.Z) F;
    const bool neg = b < 0;
    const int babs = neg ? -b : b;
    if constexpr (UNI) {
        // KYB_F_UNIFORM: selectCached's scan (ge.go:419-435) -- all eight entries read, one kept by mask
        ge_cached_0(c);
#pragma unroll 1
        for (int m = 1; m <= 8; m++) {
            C x;
            tab.get(x, m - 1);
            const int32_t keep = -(int32_t)(babs == m);
#pragma unroll
            for (int l = 0; l < F::N; l++) {
                c.YpX.v[l] ^= (c.YpX.v[l] ^ x.YpX.v[l]) & keep;
                c.YmX.v[l] ^= (c.YmX.v[l] ^ x.YmX.v[l]) & keep;
                c.Z.v[l] ^= (c.Z.v[l] ^ x.Z.v[l]) & keep;
                c.T2d.v[l] ^= (c.T2d.v[l] ^ x.T2d.v[l]) & keep;
            }
        }
    } else if constexpr (std::is_same_v<Tab, TabGlobal_t<F>>) {
        tab.get_signed(c, b);
        return;
    } else {
        tab.get(c, babs ? babs - 1 : 0);
        if (babs == 0) ge_cached_0(c);
    }
    ge_cached_cneg(c, neg);
}

// Highest radix-16 digit position that can be non-zero for ANY lane of the wave (the recoding may carry one digit past
// the scalar's top nibble).  Wave-uniform by construction: the variable-time path below starts its ladder there.
KYB_DEV int wave_top_digit(const uint32_t a[8]) {
    int bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (a[i]) bits = 32 * i + 32 - __builtin_clz(a[i]);
    int t = (bits + 3) >> 2;  // digits 0 .. t may be non-zero (t: the carry)
    if (t > 64) t = 64;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(t, off, 64);
        t = o > t ? o : t;
    }
    t = __builtin_amdgcn_readfirstlane(t);
#endif
    return t;
}

// tab[j] = (j + 1) A in cached form, j < 8: the window table of a signed radix-16 ladder.
// AFFINE: the caller guarantees A.Z = 1 (A comes straight from ge_p3_fromwords).  (Y+X, Y-X, 2dT) of such a point is
// its precomputed form, so (j + 1) A = j A + A is a mixed addition: ge_add's product Z(A) Z(j A) -- a multiplication
// by one -- is not formed.  The entries are the same points; their projective coordinates may differ.
template <bool AFFINE = false, class P3, class Tab>
KYB_DEV void ge_window_table(Tab& tab, const P3& A) {
    typedef ge_t<decltype(A.X)> G;
    typename G::p1p1 t;
    P3 u;
    typename G::cached c;
    ge_p3_to_cached(c, A);
    tab.put(0, c);
    if constexpr (AFFINE) {
        const typename G::precomp a{c.YpX, c.YmX, c.T2d};
        u = A;
#pragma unroll 1
        for (int i = 0; i < 7; i++) {
            ge_madd(t, u, a);
            ge_p1p1_to_p3(u, t);
            ge_p3_to_cached(c, u);
            tab.put(i + 1, c);
        }
    } else {
#pragma unroll 1
        for (int i = 0; i < 7; i++) {
            ge_add(t, A, c);
            ge_p1p1_to_p3(u, t);
            ge_p3_to_cached(c, u);
            tab.put(i + 1, c);
        }
    }
}

// KYB_F_VARTIME (geScalarMultVartime, ge_mult_vartime.go:11-73: every scalar bit counts, running time depends on the
// scalar).  The reference's sliding-window NAF has its non-zero digits at scalar-dependent positions; 64 lanes in
// lock step would execute the union of all of them -- an addition at nearly every bit.  What IS data-dependent and
// still wave-uniform: the ladder starts at the highest digit any lane of the wave needs (`top`: short scalars -- the
// 128-bit coefficients of sign/bdn, small Lagrange indices -- run proportionally fewer windows) and a window whose
// digit is zero in EVERY lane skips its addition and the conversion that feeds it.  Random 253-bit scalars take the
// same 64 windows as the constant-structure path.
// AFFINE: A.Z = 1 by construction (ge_window_table).
// The walk starts from the top digit's entry itself, not from the identity plus that entry: the first window's first
// doubling takes the entry as it is read (ge_dbl_cached), where an addition to (0 : 1 : 1 : 0) and a conversion -- seven
// products -- led to the same point.  So the loop is entered after the first of a window's four doublings and leaves
// after its last window's addition; a walk of no window at all (top = 0: a wave of all-zero scalars under
// KYB_F_VARTIME) hands the entry on as a completed point.  The result is left completed: the caller converts it to what
// it keeps (ge_scalarmult_w4 below: extended; a kernel that parks or encodes (X, Y, Z): projective, one product less).
template <bool UNI = false, bool AFFINE = false, class P1, class P3, class Tab>
KYB_DEV void ge_scalarmult_w4_p1p1(P1& t, const int8_t e[65], const P3& A, bool full, Tab& tab, int vt_top) {
    typedef ge_t<decltype(A.X)> G;
    // The digit of a window is known before its doublings: the slab's nine-limb entry is asked for there (nine 16-byte
    // loads), not after them where the addition would wait for it.  The 36 words stay live across three doublings; the
    // headline kernel keeps its 168 registers and no loop of it spills.  The other tables keep
    // their read next to the addition: the scan is 8 x 36 words of work, scratch reads have no address to send ahead.
    constexpr bool EARLY = !UNI && std::is_same_v<Tab, TabGlobal_t<fe29>>;
    P3 u;
    typename G::p2 r;
    typename G::cached c;
    ge_window_table<AFFINE>(tab, A);
    int top = 63;
    if (full) top = vt_top;  // uniform across the wave
    select_cached<UNI>(c, tab, e[top]);
    if (top == 0) {
        ge_cached_to_p1p1(t, c);
        return;
    }
    ge_dbl_cached(t, c);
    // The loop reads digit i from the top nibble of pk, then shifts pk up by one nibble: indexing e[i] with the loop
    // counter compiled to a select over all 65 digits in every window (64 v_cndmask + 129 scalar compares / selects).
    // Every digit the loop reads is in [-8, 7] (e[63] = 8 happens only on the constant-structure path, where it is the
    // top digit, consumed above), so e[i] + 8 fits a nibble.
    uint32_t pk[8];
    ed_pack_digits(pk, e);
    auto shl4 = [&pk]() {
#pragma unroll
        for (int j = 7; j > 0; j--) pk[j] = (pk[j] << 4) | (pk[j - 1] >> 28);
        pk[0] <<= 4;
    };
#pragma unroll 1
    for (int i = top; i < 64; i++) shl4();  // digit top - 1 to the top nibble
#pragma unroll 1
    for (int i = top - 1;; i--) {
        const int d = (int)(pk[7] >> 28) - 8;  // e[i]
        shl4();
        if constexpr (EARLY) select_cached<UNI>(c, tab, d);
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        bool add = true;
#if defined(__HIP_DEVICE_COMPILE__)
        if (!UNI && full && __ballot(d != 0) == 0) add = false;  // no lane adds anything in this window
#endif
        if (add) {
            ge_p1p1_to_p3(u, t);
            if constexpr (!EARLY) select_cached<UNI>(c, tab, d);
            ge_add(t, u, c);
        }
        if (i == 0) break;
        ge_p1p1_to_p2(r, t);  // the next window's first doubling
        ge_dbl(t, r.X, r.Y, r.Z);
    }
}
template <bool UNI = false, bool AFFINE = false, class P3, class Tab>
KYB_DEV void ge_scalarmult_w4(P3& h, const int8_t e[65], const P3& A, bool full, Tab& tab, int vt_top) {
    typename ge_t<decltype(A.X)>::p1p1 t;
    ge_scalarmult_w4_p1p1<UNI, AFFINE>(t, e, A, full, tab, vt_top);
    ge_p1p1_to_p3(h, t);
}

}  // namespace kyb
