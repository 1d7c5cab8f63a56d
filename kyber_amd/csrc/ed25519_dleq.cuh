// Ed25519 discrete-log-equality proofs, one proof per lane: the Fiat-Shamir challenge and both verification equations.
//
// Replaces, in the reference:
//   proof/dleq Proof.Verify            dleq.go:160-172   -> ed_dleq_lane (a = r G + c xG, b = r H + c xH, two Straus chains)
//   proof/dleq NewDLEQProof challenge  dleq.go:57-79     -> ed_dleq_challenge (SHA-256 over four encodings, then Pick)
//   share/pvss VerifyDecShare          pvss.go:248-276   -> ed_dleq_challenge + ed_dleq_lane in one program
//   share/pvss VerifyEncShare          pvss.go:154-163   -> ed_dleq_lane with the expected challenge compared on bytes
//   point.MarshalTo of a decoded point point.go:54-63 after ge.go:110-150 -> ed_canon_point_bytes
// Neither vG nor vH is decompressed.  They are hashed, and compared with encode(a) and encode(b), through the bytes
// MarshalTo would write for them: y reduced below p, and the sign bit cleared where x = 0 (y = 1 or p - 1; FromBytes
// accepts "-0" and ToBytes writes sign 0).  That is exact for every encoding that decodes.  One that does not decode
// has a y with no x on the curve, so its canonical bytes equal no point's encoding: an undecodable vG or vH gives
// verdict 0, as in the reference, where UnmarshalBinary fails before Verify is reached.
// Compiles with g++ too (tests/dleq_harness.cpp runs these programs on the CPU against the oracle).
#pragma once
#include "blake2xb.cuh"
#include "ed25519_verify.cuh"
#include "sha256.cuh"

namespace kyb {

// per-element status values of kyb_ed25519_dleq_verify / _challenge (include/kyber_hip.h; ed25519_dleq.hip
// static_asserts the match)
constexpr int ED_ST_DLEQ_CHALLENGE = 7, ED_ST_PICK_EXHAUSTED = 8;

// o = the bytes MarshalTo writes for the point that w decodes to, without decoding it
KYB_HD void ed_canon_point_bytes(uint32_t (&o)[8], const uint32_t w[8]) {
    uint32_t sign = w[7] & 0x80000000u;
    const uint32_t top = w[7] & 0x7fffffffu;
    uint32_t ones = 0xffffffffu, mid = 0;  // words 1..6 all ones / any bit set
#pragma unroll
    for (int i = 1; i < 7; i++) {
        ones &= w[i];
        mid |= w[i];
        o[i] = w[i];
    }
    o[0] = w[0];
    o[7] = top;
    const bool hi = (ones == 0xffffffffu) & (top == 0x7fffffffu);
    if (hi & (w[0] >= 0xffffffedu)) {  // y >= p = 2^255 - 19: y - p is below 19
        o[0] = w[0] - 0xffffffedu;
#pragma unroll
        for (int i = 1; i < 8; i++) o[i] = 0;
    }
    const bool y_one = (o[0] == 1u) & ((hi & (w[0] >= 0xffffffedu)) | ((mid == 0) & (top == 0)));
    const bool y_m1 = hi & (w[0] == 0xffffffecu);
    if (y_one | y_m1) sign = 0;  // x = 0
    o[7] |= sign;
}

// c = Pick(XOF(SHA-256(xG || xH || vG || vH))) over the canonical bytes of the four encodings: the order NewDLEQProof
// (dleq.go:57-79) and VerifyDecShare (pvss.go:250-266) hash in.  128 bytes: two blocks of data and one of padding.
// Returns ed_scalar_pick's draw count (0: exhausted).
KYB_HD int ed_dleq_challenge(uint32_t (&c)[8], const uint32_t xg[8], const uint32_t xh[8], const uint32_t vg[8],
                             const uint32_t vh[8]) {
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint32_t blk[16], t[8];
    ed_canon_point_bytes(t, xg);
#pragma unroll
    for (int i = 0; i < 8; i++) blk[i] = __builtin_bswap32(t[i]);
    ed_canon_point_bytes(t, xh);
#pragma unroll
    for (int i = 0; i < 8; i++) blk[8 + i] = __builtin_bswap32(t[i]);
    sha256_block_inl(h, blk);
    ed_canon_point_bytes(t, vg);
#pragma unroll
    for (int i = 0; i < 8; i++) blk[i] = __builtin_bswap32(t[i]);
    ed_canon_point_bytes(t, vh);
#pragma unroll
    for (int i = 0; i < 8; i++) blk[8 + i] = __builtin_bswap32(t[i]);
    sha256_block_inl(h, blk);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = 0;
    blk[0] = 0x80000000u;
    blk[15] = 128 * 8;
    sha256_block_inl(h, blk);
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = __builtin_bswap32(h[i]);  // the digest's bytes as little-endian words
    return ed_scalar_pick(c, t);
}

KYB_HD bool ed_words8_equal(const uint32_t a[8], const uint32_t b[8]) {
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= a[i] ^ b[i];
    return diff == 0;
}

// The challenge checks that come before the equations, on raw bytes (scalar.Equal compares bytes, and
// UnmarshalBinary copies them unreduced: scalar.go:37-45, 226-232):
//   expect != nullptr: c must equal the batch's one expected challenge (pvss.go:154-157);
//   fs:                c must equal the challenge derived from (xG, xH, vG, vH) (pvss.go:250-270).
KYB_DEV int ed_dleq_challenge_status(const uint32_t cw[8], const uint32_t* __restrict__ expect, bool fs, const uint32_t xg[8],
                                     const uint32_t xh[8], const uint32_t vg[8], const uint32_t vh[8]) {
    int st = ED_ST_OK;
    if (expect) {
        uint32_t e[8];
        load_words8(e, expect);
        if (!ed_words8_equal(e, cw)) st = ED_ST_DLEQ_CHALLENGE;
    }
    if (fs) {
        uint32_t d[8];
        const int draws = ed_dleq_challenge(d, xg, xh, vg, vh);
        if (!ed_words8_equal(d, cw)) st = ED_ST_DLEQ_CHALLENGE;
        if (draws == 0) st = ED_ST_PICK_EXHAUSTED;
    }
    return st;
}

// One side of the proof: h = r P + c Q from the digits of r and c (recoded once by the caller, used by both sides).
// False when P or Q does not decode.  tp, tq: room for two window tables, rewritten by each side.
template <class Tab>
KYB_DEV bool ed_dleq_side(ge_p3& h, const int8_t er[65], const int8_t ec[65], const uint32_t pw[8], const uint32_t qw[8],
                          bool full, int vt_top, Tab& tp, Tab& tq) {
    ge_p3 A;  // one point at a time: decoded, its table written, forgotten
    bool ok = ge_p3_fromwords(A, pw);
    ge_window_table(tp, A);
    ok &= ge_p3_fromwords(A, qw);
    ge_window_table(tq, A);
    ge_double_scalarmult_w4(h, er, ec, full, tp, tq, vt_top);
    return ok;
}

// Both sides of dleq.go:161-172 for one proof.  `st` is the status of the challenge checks (taken first by the caller,
// so that the hash's working set and a point's never meet in the registers); the reference's order is the precedence:
// a challenge mismatch, then ED_ST_BAD_POINT if G, H, xG or xH does not decode.  park(side, h) receives a (side 0) as
// soon as it is known, then b (side 1); a side with an undecodable point parks the identity, so that a parked triple
// is always invertible.  The verdict is status == 0 && encode(a) == canon(vG) && encode(b) == canon(vH) on bytes,
// taken by the caller's encode pass: Point.Equal on re-encodings (point.go:81-96).
// load(side, pw, qw) fetches (G, xG) for side 0 and (H, xH) for side 1: the sides are told apart by address, never by
// selecting between register arrays (which would put them in scratch).
template <class Tab, class Load, class Park>
KYB_DEV int ed_dleq_lane(int st, const uint32_t cw[8], const uint32_t rw[8], bool full, Tab& tp, Tab& tq, Load load, Park park) {
    int8_t er[65], ec[65];  // recoded once, used by both chains
    recode16(er, rw, full);
    recode16(ec, cw, full);
    int vt_top = 63;
    if (full) {
        const int ta = wave_top_digit(rw), tb = wave_top_digit(cw);
        vt_top = ta > tb ? ta : tb;
    }
    ge_p3 h;
    bool ok = true;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {  // one copy of the chain's code serves both sides
        uint32_t pw[8], qw[8];
        load(side, pw, qw);
        const bool good = ed_dleq_side(h, er, ec, pw, qw, full, vt_top, tp, tq);
        if (!good) ge_p3_0(h);
        ok &= good;
        park(side, h);
    }
    if (st == ED_ST_OK && !ok) st = ED_ST_BAD_POINT;
    return st;
}

}  // namespace kyb
