// Ed25519 signature verification and double-scalar multiplication, one element per lane.
//
// Replaces, in the reference:
//   sign/eddsa VerifyWithChecks     eddsa.go:143-229    -> ed_verify_lane (checks, hash, T = S B - h A)
//   sign/schnorr VerifyWithChecks   schnorr.go:84-160   -> the same program (same bytes hashed, same equation)
//   proof/dleq Proof.Verify         dleq.go:160-172     -> ed_mul2_lane (r G + c xG as one Straus-Shamir chain)
//   scalar.IsCanonical              scalar.go:2308-2333 -> sf::geq against l
//   point.IsCanonical/HasSmallOrder point.go:262-323    -> ed_point_is_canonical / ed_point_has_small_order
//   scalar.SetBytes of a 64-byte hash (scalar.go:187)   -> sc_reduce512
// The verify equation S B = R + h A is checked as encode(S B - h A) == R on bytes: one variable-base ladder on -A, the
// standard base's wide comb added into the same accumulator, and R never decompressed.  That is exact because
// Point.Equal compares canonical encodings (point.go:81-96), R's y has been found canonical, the canonical-y encodings
// that re-encode differently (x = 0 with the sign bit set) are small-order and rejected before, and an R that is no
// curve point equals no point's encoding -- the reference rejects it as well (UnmarshalBinary fails).
// Compiles with g++ too (tests/ed_verify_harness.cpp runs these lane programs on the CPU against the oracle).
#pragma once
#include "ed25519_dev.cuh"
#include "scalar_field.cuh"
#include "sha512.cuh"

namespace kyb {

// per-element status values of kyb_ed25519_verify (include/kyber_hip.h; ed25519_verify.hip static_asserts the match)
constexpr int ED_ST_OK = 0, ED_ST_BAD_POINT = 1, ED_ST_SIG_NONCANONICAL = 5, ED_ST_SIG_SMALL_ORDER = 6;

// y < p = 2^255 - 19, the sign bit ignored (point.go:296-323)
KYB_DEV bool ed_point_is_canonical(const uint32_t w[8]) {
    bool top = (w[7] & 0x7fffffffu) == 0x7fffffffu;
#pragma unroll
    for (int i = 1; i < 7; i++) top &= w[i] == 0xffffffffu;
    return !(top & (w[0] >= 0xffffffedu));
}
// y is one of the five y-coordinates of the eight points of small order (point.go:262-294 with const.go's weakKeys:
// 0, 1, p - 1 and the two of order 8), the sign bit ignored.  Called on canonical encodings only, where the bytes ARE
// the re-encoding HasSmallOrder looks at.  tests/test_ed_verify_host.py checks the list against the oracle's
// [8]P = identity.
KYB_DEV bool ed_point_has_small_order(const uint32_t w[8]) {
    const uint32_t t = w[7] & 0x7fffffffu;
    uint32_t mid = 0, ones = 0xffffffffu;  // words 1..6 all zero / all ones
#pragma unroll
    for (int i = 1; i < 7; i++) {
        mid |= w[i];
        ones &= w[i];
    }
    const bool y01 = (w[0] <= 1u) & (mid == 0) & (t == 0);
    const bool ym1 = (w[0] == 0xffffffecu) & (ones == 0xffffffffu) & (t == 0x7fffffffu);
    const bool o8a = (w[0] == 0x706a17c7u) & (w[1] == 0x4fd84d3du) & (w[2] == 0x760b3cbau) & (w[3] == 0x0f67100du) &
                     (w[4] == 0xfa53202au) & (w[5] == 0xc6cc392cu) & (w[6] == 0x77fdc74eu) & (t == 0x7a03ac92u);
    const bool o8b = (w[0] == 0x8f95e826u) & (w[1] == 0xb027b2c2u) & (w[2] == 0x89f4c345u) & (w[3] == 0xf098eff2u) &
                     (w[4] == 0x05acdfd5u) & (w[5] == 0x3933c6d3u) & (w[6] == 0x880238b1u) & (t == 0x05fc536du);
    return y01 | ym1 | o8a | o8b;
}

// r = x mod q for a 512-bit x (16 little-endian words), r < q.  With R = 2^256 and x = lo + hi R:
// mont_mul(hi, R^2) = hi R and mont_mul(mont_mul(lo, R^2), 1) = lo, both already reduced.
KYB_HD void sc_reduce512(uint32_t (&r)[8], const uint32_t (&x)[16], const sf::Mod& m) {
    uint32_t lo[8], hi[8], t[8], u[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        lo[i] = x[i];
        hi[i] = x[8 + i];
    }
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    sf::mont_mul(t, hi, m.r2, m);
    sf::mont_mul(u, lo, m.r2, m);
    sf::mont_mul(lo, u, one, m);
    sf::add_mod(r, t, lo, m);
}

// SHA-512 compression with the message schedule as a 16-word ring in registers (every index is a compile-time
// constant): the hash of the verify program takes no scratch.  w is consumed.
KYB_DEV void sha512_compress_regs(uint64_t (&h)[8], uint64_t (&w)[16]) {
    constexpr uint64_t K[80] = KYB_SHA512_K;
    uint64_t s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = h[i];
#pragma unroll
    for (int i = 0; i < 80; i++) {
        if (i >= 16) {
            const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (sha512_rotr(w15, 1) ^ sha512_rotr(w15, 8) ^ (w15 >> 7)) + w[(i + 9) & 15] +
                         (sha512_rotr(w2, 19) ^ sha512_rotr(w2, 61) ^ (w2 >> 6));
        }
        // the eight working variables rotate through s by index instead of by copies: a = s[(0 - i) & 7], ...
        uint64_t& a = s[(80 - i) & 7];
        uint64_t& b = s[(81 - i) & 7];
        uint64_t& c = s[(82 - i) & 7];
        uint64_t& d = s[(83 - i) & 7];
        uint64_t& e = s[(84 - i) & 7];
        uint64_t& f = s[(85 - i) & 7];
        uint64_t& g = s[(86 - i) & 7];
        uint64_t& hh = s[(87 - i) & 7];
        const uint64_t t1 = hh + (sha512_rotr(e, 14) ^ sha512_rotr(e, 18) ^ sha512_rotr(e, 41)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const uint64_t t2 = (sha512_rotr(a, 28) ^ sha512_rotr(a, 34) ^ sha512_rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
        d += t1;
        hh = t1 + t2;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] += s[i];
}

// The 64-bit big-endian word at offset pos (a multiple of 8) of the padded stream msg || 0x80 || 0 ... || bit length,
// for a message that is preceded by 64 hashed bytes; lenpos = the offset of the length's low word.
KYB_DEV uint64_t ed_hram_msg_word(const uint8_t* __restrict__ msg, size_t len, size_t pos, size_t lenpos) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const size_t p = pos + k;
        const uint32_t byte = p < len ? msg[p] : (p == len ? 0x80u : 0u);
        v = (v << 8) | byte;
    }
    if (pos == lenpos) v |= (uint64_t)(len + 64) * 8;
    return v;
}
KYB_DEV uint64_t ed_be64(uint32_t lo, uint32_t hi) {  // eight stream bytes held as two little-endian words
    return ((uint64_t)__builtin_bswap32(lo) << 32) | __builtin_bswap32(hi);
}

// h = SHA-512(R || A || msg) mod l as eight little-endian words (eddsa.go:207-219)
KYB_DEV void ed_hram(uint32_t (&hw)[8], const uint32_t rw[8], const uint32_t aw[8], const uint8_t* __restrict__ msg,
                     size_t len, const sf::Mod& m) {
    uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    const size_t padded = (64 + len + 17 + 127) / 128 * 128;  // bytes hashed, padding and length included
    const size_t lenpos = padded - 64 - 8;
    uint64_t w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[i] = ed_be64(rw[2 * i], rw[2 * i + 1]);
        w[4 + i] = ed_be64(aw[2 * i], aw[2 * i + 1]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) w[8 + i] = ed_hram_msg_word(msg, len, 8 * i, lenpos);
    sha512_compress_regs(h, w);
#pragma unroll 1
    for (size_t pos = 64; pos + 64 < padded; pos += 128) {
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = ed_hram_msg_word(msg, len, pos + 8 * i, lenpos);
        sha512_compress_regs(h, w);
    }
    // the digest's bytes are h[0..7] big-endian; the scalar is those 64 bytes little-endian
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t le = __builtin_bswap64(h[i]);
        x[2 * i] = (uint32_t)le;
        x[2 * i + 1] = (uint32_t)(le >> 32);
    }
    sc_reduce512(hw, x, m);
}

// The byte-level checks of VerifyWithChecks in the reference's order (eddsa.go:158-206), first failure wins:
// S < l, R canonical, R not of small order, A canonical, A decodes, A not of small order.  R's own decoding is left to
// the equation (see the head of this file).  a_ok: -A (or A) decoded.
KYB_DEV int ed_verify_checks(const uint32_t rw[8], const uint32_t sw[8], const uint32_t aw[8], bool a_ok, const sf::Mod& m) {
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = sw[i];
    int st = ED_ST_OK;
    if (ed_point_has_small_order(aw)) st = ED_ST_SIG_SMALL_ORDER;
    if (!a_ok) st = ED_ST_BAD_POINT;
    if (!ed_point_is_canonical(aw)) st = ED_ST_SIG_NONCANONICAL;
    if (ed_point_has_small_order(rw)) st = ED_ST_SIG_SMALL_ORDER;
    if (!ed_point_is_canonical(rw)) st = ED_ST_SIG_NONCANONICAL;
    if (sf::geq(s, 0, m.q)) st = ED_ST_SIG_NONCANONICAL;
    return st;
}

// One signature: returns the status of the checks and, in T, S B - h A (the identity when a check failed, so that a
// parked triple is always invertible).  The verdict is encode(T) == R on bytes, taken by the caller.
// wide: the standard base's comb (EdWide).  tab: room for one 8-entry window table.
template <class Tab>
KYB_DEV int ed_verify_lane(ge_p3& T, const uint32_t rw[8], const uint32_t sw[8], const uint32_t aw[8],
                           const uint8_t* __restrict__ msg, size_t len, const int32_t* __restrict__ wide,
                           const sf::Mod& m, Tab& tab) {
    uint32_t hw[8];
    ed_hram(hw, rw, aw, msg, len, m);  // first: the hash's working set and the point's never meet in the registers
    uint32_t nw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) nw[i] = aw[i];
    nw[7] ^= 0x80000000u;  // the other sign of x: decodes to -A
    ge_p3 nA;
    const bool a_ok = ge_p3_fromwords(nA, nw);
    const int st = ed_verify_checks(rw, sw, aw, a_ok, m);
    int8_t e[65];
    recode16(e, hw, false);  // h < l: no digit is dropped
    ge_scalarmult_w4(T, e, nA, false, tab, 63);
    recode16(e, sw, false);  // S < l where the verdict counts
    ge_precomp t;
    ge_p1p1 r;
#pragma unroll 1
    for (int k = 0; k < EdWide::POS_CT; k++) {
        int d = 0;
#pragma unroll
        for (int i = ED_COMB_G - 1; i >= 0; i--)
            if (ED_COMB_G * k + i < 64) d = 16 * d + (int)e[ED_COMB_G * k + i];
        select_precomp_tab<EdWide::ENT>(t, wide, k, d);
        ge_madd(r, T, t);
        ge_p1p1_to_p3(T, r);
    }
    if (st != ED_ST_OK) ge_p3_0(T);
    return st;
}

// Signed radix-16 digits e[0..63] + 8 as nibbles, read from the top: indexing e[] by a loop counter compiles to a
// select over all 65 digits in every window (ge_scalarmult_w4 keeps its digits the same way).
struct EdDigitQueue {
    uint32_t pk[8];
    KYB_DEV void init(const int8_t e[65]) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            pk[j] = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) pk[j] |= (uint32_t)((e[8 * j + q] + 8) & 15) << (4 * q);
        }
    }
    KYB_DEV void shl4() {
#pragma unroll
        for (int j = 7; j > 0; j--) pk[j] = (pk[j] << 4) | (pk[j - 1] >> 28);
        pk[0] <<= 4;
    }
    KYB_DEV int pop() {
        const int d = (int)(pk[7] >> 28) - 8;
        shl4();
        return d;
    }
};

// h = sum_i 16^i (ea[i] P + eb[i] Q), Straus-Shamir: two window tables, one chain of doublings, two additions per
// window.  Digits are recode16's, so the value is that of ge_scalarmult_w4 on (ea, P) plus that on (eb, Q) for every
// scalar and both values of `full` (KYB_F_VARTIME: the chain starts at the highest digit any lane of the wave needs for
// either scalar -- vt_top -- and a window whose digits are zero in every lane skips its additions).
// tp, tq: the window tables of P and Q (ge_window_table), built by the caller one after the other.
template <class Tab>
KYB_DEV void ge_double_scalarmult_w4(ge_p3& h, const int8_t ea[65], const int8_t eb[65], bool full, Tab& tp, Tab& tq,
                                     int vt_top) {
    ge_p1p1 t;
    ge_p3 u;
    ge_p2 r;
    ge_cached c;
    int top = 63;
    if (full) top = vt_top;  // uniform across the wave
    ge_p3_0(u);
    select_cached(c, tp, ea[top]);
    ge_add(t, u, c);
    ge_p1p1_to_p3(u, t);
    select_cached(c, tq, eb[top]);
    ge_add(t, u, c);
    EdDigitQueue qa, qb;
    qa.init(ea);
    qb.init(eb);
#pragma unroll 1
    for (int i = top; i < 64; i++) {  // digit top - 1 to the top nibble
        qa.shl4();
        qb.shl4();
    }
#pragma unroll 1
    for (int i = top - 1; i >= 0; i--) {
        const int da = qa.pop(), db = qb.pop();
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            ge_p1p1_to_p2(r, t);
            ge_dbl(t, r.X, r.Y, r.Z);
        }
#if defined(__HIP_DEVICE_COMPILE__)
        if (full && __ballot((da | db) != 0) == 0) continue;  // no lane adds anything in this window
#endif
        ge_p1p1_to_p3(u, t);
        select_cached(c, tp, da);
        ge_add(t, u, c);
        ge_p1p1_to_p3(u, t);
        select_cached(c, tq, db);
        ge_add(t, u, c);
    }
    ge_p1p1_to_p3(h, t);
}

// One a P + b Q: false when P or Q does not decode (h is then the identity).  tp, tq: room for two window tables.
template <class Tab>
KYB_DEV bool ed_mul2_lane(ge_p3& h, const uint32_t aw[8], const uint32_t pw[8], const uint32_t bw[8], const uint32_t qw[8],
                          bool full, Tab& tp, Tab& tq) {
    ge_p3 A;  // one point at a time: decoded, its table written, forgotten
    bool ok = ge_p3_fromwords(A, pw);
    ge_window_table(tp, A);
    ok &= ge_p3_fromwords(A, qw);
    ge_window_table(tq, A);
    int8_t ea[65], eb[65];
    recode16(ea, aw, full);
    recode16(eb, bw, full);
    int vt_top = 63;
    if (full) {
        const int ta = wave_top_digit(aw), tb = wave_top_digit(bw);
        vt_top = ta > tb ? ta : tb;
    }
    ge_double_scalarmult_w4(h, ea, eb, full, tp, tq, vt_top);
    if (!ok) ge_p3_0(h);
    return ok;
}

}  // namespace kyb
