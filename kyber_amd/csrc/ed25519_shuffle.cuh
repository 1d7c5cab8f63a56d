// Neff verifiable shuffles on Ed25519: the two lane programs the batched verifier and prover lacked.
//
// Replaces, in the reference:
//   proof hashVerifier.PubRand / hashProver.PubRand   hash.go:68-75, 111-142  -> ed_xof_draw, one candidate draw per lane
//   xof/blake2xb Read at any byte position            blake.go:47-49          -> ed_xof_read32 (a draw may straddle two nodes)
//   util/random Bits / Int, scalar.Pick               rand.go:19-46, scalar.go:180-184 -> ed_pick_draw (blake2xb.cuh)
//   shuffle thver over Xhat = X + U, Yhat = Y + W      simple.go:178-183, 225-242 -> ed_theta_lane
//   scalar.Neg                                        scalar.go:119-128       -> ed_scalar_neg (the reduced residue of -b)
//
// A sequence of n Picks from ONE stream is sequential in the reference: every rejected draw moves all later ones.  Here
// every candidate draw of a fixed window is tested on its own -- draw j is the 32 stream bytes at pos + 32 j, whatever
// happened to the draws before it -- and the accepted ones are compacted in order by the kernels of ed25519_shuffle.hip.
// The window of ed_xof_window(n) = 2n + 16 ceil(sqrt n) + 256 draws holds, at an acceptance of l / 2^253 (just above
// one half), n + 8 sqrt n + 128 accepted draws on average with a deviation of 0.71 sqrt n: the n-th accepted draw lies
// outside it with a probability below that of an eleven-sigma event.
// Compiles with g++ too (tests/shuffle_harness.cpp runs these programs on the CPU against the Python XOF and the oracle).
#pragma once
#include "ed25519_dleq.cuh"

namespace kyb {

// W(n): candidate draws examined for n picks; ceil(sqrt n) in integers
KYB_HD uint64_t ed_xof_isqrt_ceil(uint64_t n) {
    uint64_t lo = 0, hi = (uint64_t)1 << 32;  // lo^2 < n <= hi^2 for n >= 1
    if (n == 0) return 0;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (mid * mid >= n) hi = mid; else lo = mid;
    }
    return hi;
}
KYB_HD uint64_t ed_xof_window(uint64_t n) { return 2 * n + 16 * ed_xof_isqrt_ceil(n) + 256; }

// Output node `node` of the stream whose root hash is m[0..7] (m[8..15] zero): one compression
KYB_HD void ed_xof_node(uint64_t (&h)[8], const uint64_t (&m)[16], uint32_t node) {
    blake2xb_node_iv(h, node);
    blake2b_compress_regs(h, m, 64, true);
}

// o = the 32 stream bytes at byte position p, as four little-endian words in stream order.  One compression when the
// bytes lie in one node (p mod 64 <= 32), two when they straddle.  p / 64 (+ 1 when straddling) is below 2^32: the
// entry points check the window before any lane runs.
KYB_HD void ed_xof_read32(uint64_t (&o)[4], const uint64_t (&m)[16], uint64_t p) {
    const uint32_t node = (uint32_t)(p >> 6), off = (uint32_t)(p & 63);
    uint64_t h[8], w[5];  // w[i] = word q + i of the 16-word pair (this node, the next); a word never computed is 0
    ed_xof_node(h, m, node);
    const uint32_t q = off >> 3, r = (off & 7) * 8;  // first word, bit shift inside it
    if (off > 32) {
        uint64_t g[8];
        ed_xof_node(g, m, node + 1);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            uint64_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                v = (q + i == (uint32_t)k) ? h[k] : v;
                v = (q + i == (uint32_t)(8 + k)) ? g[k] : v;
            }
            w[i] = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            uint64_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) v = (q + i == (uint32_t)k) ? h[k] : v;
            w[i] = v;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = r ? (w[i] >> r) | (w[i + 1] << (64 - r)) : w[i];
}

// Candidate draw j of the window that starts at byte `pos`: c = its value (253 bits), true iff Pick accepts it (< l)
KYB_HD bool ed_xof_draw(uint32_t (&c)[8], const uint64_t (&m)[16], uint64_t pos, uint64_t j) {
    uint64_t o[4];
    ed_xof_read32(o, m, pos + 32 * j);
    return ed_pick_draw(c, o[0], o[1], o[2], o[3]);
}

// the root hash's 64 bytes (eight little-endian words) as the message block every output node compresses
KYB_HD void ed_xof_root_block(uint64_t (&m)[16], const uint64_t* root) {
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = root[i];
#pragma unroll
    for (int i = 8; i < 16; i++) m[i] = 0;
}

// r = -b mod l, fully reduced (0 for b = 0 mod l), for any 32-byte b: what scSub(0, b) leaves (scalar.go:119-128)
KYB_HD void ed_scalar_neg(uint32_t (&r)[8], const uint32_t b[8], const sf::Mod& m) {
    uint32_t x[8], t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = b[i];
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    sf::mont_mul(t, x, m.r2, m);  // b 2^256 mod l
    sf::mont_mul(x, t, one, m);   // b mod l
    uint32_t nz = 0, borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        nz |= x[i];
        const uint64_t d = (uint64_t)m.q[i] - x[i] - borrow;
        r[i] = (uint32_t)d;
        borrow = (uint32_t)(d >> 63);
    }
    if (nz == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) r[i] = 0;
    }
}

// tab = the window table of P + S (S: the batch's shared addend, nullptr for none).  False when P or S does not decode.
template <class Tab>
KYB_DEV bool ed_theta_base(Tab& tab, const uint32_t pw[8], const uint32_t* __restrict__ shared) {
    ge_p3 A;
    bool ok = ge_p3_fromwords(A, pw);
    if (shared) {
        uint32_t sw[8];
        load_words8(sw, shared);
        ge_p3 S;
        ok &= ge_p3_fromwords(S, sw);
        ge_cached c;
        ge_p3_to_cached(c, S);
        ge_p1p1 t;
        ge_add(t, A, c);
        ge_p1p1_to_p3(A, t);
    }
    ge_window_table(tab, A);
    return ok;
}

// One element of the simple k-shuffle's check: h = a (A + U) + Neg(b) (B + W) as one Straus-Shamir chain with
// kyb_ed25519_mul2's value under `full` (a as its 32 wire bytes; Neg(b) below l, so no digit of it is ever dropped).
// Returns ED_ST_BAD_POINT, with h the identity, when A, B, U or W does not decode.  The verdict is
// status == 0 && encode(h) == canon(T) on bytes, taken by the caller's encode pass.
template <class Tab>
KYB_DEV int ed_theta_lane(ge_p3& h, const uint32_t aw[8], const uint32_t Aw[8], const uint32_t* __restrict__ U,
                          const uint32_t bw[8], const uint32_t Bw[8], const uint32_t* __restrict__ W, bool full,
                          const sf::Mod& m, Tab& tp, Tab& tq) {
    bool ok = ed_theta_base(tp, Aw, U);
    ok &= ed_theta_base(tq, Bw, W);
    uint32_t nb[8];
    ed_scalar_neg(nb, bw, m);
    int8_t ea[65], eb[65];
    recode16(ea, aw, full);
    recode16(eb, nb, full);
    int vt_top = 63;
    if (full) {
        const int ta = wave_top_digit(aw), tb = wave_top_digit(nb);
        vt_top = ta > tb ? ta : tb;
    }
    ge_double_scalarmult_w4(h, ea, eb, full, tp, tq, vt_top);
    if (!ok) ge_p3_0(h);
    return ok ? ED_ST_OK : ED_ST_BAD_POINT;
}

}  // namespace kyb
