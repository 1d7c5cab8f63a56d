// sign/dss on Ed25519 (dss.go): the lane programs of ed25519_dss.hip.
//
// Replaces, in the reference:
//   hashSig: h = SHA-512(R || A || msg) mod l                  dss.go:201-211  -> ed_dss_session_lane (ed_hram)
//   sessionID: SHA-256(long commitments || random commitments)  dss.go:235-246  -> ed_dss_session_id
//   PartialSig.Hash over PriShare.Hash                          dss.go:221-226, share/poly.go:35-40
//                                                                               -> ed_dss_partial_hash
//   PartialSig: V = h alpha + beta, schnorr.Sign                dss.go:113-134  -> ed_dss_partial_element over
//                                                                                  ed_schnorr_response and ed_hram96
//   ProcessPartialSig: findPub, schnorr.Verify                  dss.go:141-149  -> ed_dss_verify_lane
//   ProcessPartialSig: the session id, V B == randomPoly.Eval(I) + h longPoly.Eval(I)
//                                                               dss.go:152-169  -> ed_dss_fold_lane, then
//                                                                                  ed_deal_check_lane (ed25519_dkg.cuh)
// The fold: D_k = R_k + h A_k, one ladder per commitment of a SESSION, turns the equation of every partial signature of
// that session into a share check against the polynomial D -- sum_k x^k D_k = randomPoly.Eval(I).V + h longPoly.Eval(I).V
// for EVERY input, because multiplication by the integers h and x^k and addition are homomorphisms of the whole curve
// group, torsion included.  The ladders are the nine-limb ones of kyb_ed25519_mul (ge_scalarmult_w4 on ge29_p3); the
// signature's T = S B - h A joins the ten-limb comb through its canonical words.
// Compiles with g++ too (tests/dss_harness.cpp runs these programs on the CPU against the oracle).
#pragma once
#include "ed25519_vss.cuh"

namespace kyb {

// per-element status values of kyb_ed25519_dss_check (include/kyber_hip.h; ed25519_dss.hip static_asserts the match)
constexpr int ED_ST_DSS_INDEX = 14, ED_ST_DSS_SIG = 15, ED_ST_DSS_SESSION = 16, ED_ST_DSS_PARTIAL = 17;

using DssTab = TabGlobal_t<fe29>;

// sid = SHA-256(lc[0 .. tl) || rc[0 .. tr)) as the eight little-endian words of its 32 bytes; the commitments are read as
// little-endian words where they lie.  Two commitments make a block: tl + tr even ends the data on a block boundary and
// the padding takes a block of its own.
KYB_HD void ed_dss_session_id(uint32_t (&sid)[8], const uint32_t* __restrict__ lc, size_t tl, const uint32_t* __restrict__ rc,
                              size_t tr) {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    const uint64_t lw = 8 * (uint64_t)tl, words = lw + 8 * (uint64_t)tr, bits = words * 32;
    const uint64_t nb = (words * 4 + 9 + 63) / 64;
    uint32_t blk[16];
#pragma unroll 1
    for (uint64_t b = 0; b < nb; b++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t j = 16 * b + i;
            blk[i] = j < lw ? __builtin_bswap32(lc[j]) : (j < words ? __builtin_bswap32(rc[j - lw]) : (j == words ? 0x80000000u : 0u));
        }
        if (b == nb - 1) {
            blk[14] = (uint32_t)(bits >> 32);
            blk[15] = (uint32_t)bits;
        }
        sha256_block_inl(h, blk);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) sid[i] = __builtin_bswap32(h[i]);
}

// m = SHA-256(SHA-256(V || u32le(I)) || sid), the bytes a partial signature's Schnorr signature covers, as eight
// little-endian words.  vw: V's 32 bytes as they travel; sid: the 32 bytes of the session id.
KYB_HD void ed_dss_partial_hash(uint32_t (&mw)[8], const uint32_t vw[8], uint32_t index, const uint32_t sid[8]) {
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t h[8], g[8], blk[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h[i] = g[i] = iv[i];
        blk[i] = __builtin_bswap32(vw[i]);
    }
    blk[8] = __builtin_bswap32(index);
    blk[9] = 0x80000000u;
#pragma unroll
    for (int i = 10; i < 15; i++) blk[i] = 0;
    blk[15] = 36 * 8;
    sha256_block_inl(h, blk);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        blk[i] = h[i];
        blk[8 + i] = __builtin_bswap32(sid[i]);
    }
    sha256_block_inl(g, blk);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = 0;
    blk[0] = 0x80000000u;
    blk[15] = 64 * 8;
    sha256_block_inl(g, blk);
#pragma unroll
    for (int i = 0; i < 8; i++) mw[i] = __builtin_bswap32(g[i]);
}

// One session: h = SHA-512(rc[0] || lc[0] || msg) mod l and the session id, from the commitments' bytes (MarshalTo's)
KYB_DEV void ed_dss_session_lane(uint32_t (&hw)[8], uint32_t (&sid)[8], const uint32_t* __restrict__ lc, size_t tl,
                                 const uint32_t* __restrict__ rc, size_t tr, const uint8_t* __restrict__ msg, size_t len,
                                 const sf::Mod& m) {
    uint32_t r0[8], a0[8];
    load_words8(r0, rc);
    load_words8(a0, lc);
    ed_hram(hw, r0, a0, msg, len, m);
    ed_dss_session_id(sid, lc, tl, rc, tr);
}

// D = R + h A on the nine-limb ladder; a missing term comes as the identity's encoding.  false, with D the identity,
// when R or A does not decode.  h < l: recode16's digits are the integer h.
KYB_DEV bool ed_dss_fold_lane(ge29_p3& D, const uint32_t hw[8], const uint32_t rw[8], const uint32_t aw[8], DssTab& tab) {
    ge29_p3 P;
    bool ok = ge_p3_fromwords(P, aw);
    int8_t e[65];
    recode16(e, hw, false);
    ge_scalarmult_w4<false, true>(D, e, P, false, tab, 63);  // P.Z = 1: decoded just above
    ok &= ge_p3_fromwords(P, rw);
    ge29_cached c;
    ge29_p1p1 t;
    ge_p3_to_cached(c, P);
    ge_add(t, D, c);
    ge_p1p1_to_p3(D, t);
    if (!ok) ge_p3_0(D);
    return ok;
}

// schnorr.VerifyWithChecks(A, m, R || S) for a 32-byte message: kyb_ed25519_verify's program (ed_verify_lane) with the
// one-block hash and the ladder on nine limbs.  Returns the checks' status; T = S B - h A (the identity when a check
// failed), the verdict encode(T) == R being the caller's.
KYB_DEV int ed_dss_verify_lane(ge_p3& T, const uint32_t rw[8], const uint32_t sw[8], const uint32_t aw[8], const uint32_t mw[8],
                               const int32_t* __restrict__ wide, const sf::Mod& m, DssTab& tab) {
    uint32_t hw[8];
    ed_hram96(hw, rw, aw, mw, m);
    uint32_t nw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) nw[i] = aw[i];
    nw[7] ^= 0x80000000u;  // the other sign of x: decodes to -A
    ge29_p3 nA, T9;
    const bool a_ok = ge_p3_fromwords(nA, nw);
    const int st = ed_verify_checks(rw, sw, aw, a_ok, m);
    int8_t e[65];
    recode16(e, hw, false);
    ge_scalarmult_w4<false, true>(T9, e, nA, false, tab, 63);
    {
        // through the canonical words, whose limbs are unsigned and full: one multiplication by one brings each
        // coordinate back into the range the mixed addition's sums may have (as ed_deal_decode does for its sums)
        fe one;
        fe_1(one);
        fe29_to_fe(T.X, T9.X);
        fe29_to_fe(T.Y, T9.Y);
        fe29_to_fe(T.Z, T9.Z);
        fe29_to_fe(T.T, T9.T);
        fe_mul(T.X, T.X, one);
        fe_mul(T.Y, T.Y, one);
        fe_mul(T.Z, T.Z, one);
        fe_mul(T.T, T.T, one);
    }
    recode16(e, sw, false);  // S < l where the verdict counts
    {
        ge_precomp p;
        ge_p1p1 r;
        EdCombDigits<ED_COMB_G> digits(e);
#pragma unroll 1
        for (int k = 0; k < EdWide::POS_CT; k++) {
            const int d = digits.next(k);
            select_precomp_tab<EdWide::ENT>(p, wide, k, d);
            ge_madd(r, T, p);
            ge_p1p1_to_p3(T, r);
        }
    }
    if (st != ED_ST_OK) ge_p3_0(T);
    return st;
}

// The last pass of one partial signature to check.  st: the signature's status with ED_ST_DSS_SIG where only the
// equation failed; sess_bad: a commitment of the session did not decode.  Returns the element's final status; ok = 1
// only with 0.
KYB_DEV int ed_dss_share_element(int st, const uint32_t sidw[8], const uint32_t sess_sid[8], bool sess_bad, const uint32_t vw[8],
                                 const ge_precomp* __restrict__ folded, size_t t, uint32_t idx, const int32_t* __restrict__ wide) {
    if (st != ED_ST_OK) return st;
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= sidw[i] ^ sess_sid[i];
    if (diff) return ED_ST_DSS_SESSION;
    if (sess_bad) return ED_ST_BAD_POINT;
    return ed_deal_check_lane(vw, folded, t, idx, wide) ? ED_ST_OK : ED_ST_DSS_PARTIAL;
}

// PartialSig for one session: V = h alpha + beta mod l and the bytes the signature covers
KYB_HD void ed_dss_partial_value(uint32_t (&V)[8], uint32_t (&mw)[8], const uint32_t hw[8], const uint32_t alpha[8],
                                 const uint32_t beta[8], uint32_t index, const uint32_t sid[8], const sf::Mod& m) {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = hw[i];
    ed_schnorr_response(V, beta, alpha, h, m);
    ed_dss_partial_hash(mw, V, index, sid);
}
// ... and its signature R || S from the encodings of R = k B and A = priv B: kyb_ed25519_schnorr_sign's bytes
KYB_DEV void ed_dss_partial_sign(uint32_t (&sig)[16], const uint32_t rw[8], const uint32_t aw[8], const uint32_t kw[8],
                                 const uint32_t xw[8], const uint32_t mw[8], const sf::Mod& m) {
    uint32_t hw[8], S[8];
    ed_hram96(hw, rw, aw, mw, m);
    ed_schnorr_response(S, kw, xw, hw, m);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        sig[i] = rw[i];
        sig[8 + i] = S[i];
    }
}

}  // namespace kyb
