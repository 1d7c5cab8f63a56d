// share/vss (Pedersen and Rabin) on Ed25519: the lane programs of ed25519_vss.hip.
//
// Replaces, in the reference:
//   sign/schnorr Sign                schnorr.go:56-82             -> ed_schnorr_points_lane (R = k B, A = x B on the comb),
//                                                                   ed_schnorr_response (S = k + h x mod l)
//   Dealer.EncryptedDeal             pedersen/vss.go:222-255, rabin/vss.go:263-297
//                                                                -> ed_vss_seal_lane, ed_vss_seal_element
//   decryptDeal, after its Verify    pedersen/vss.go:443-457      -> ed_vss_open_lane, ed_vss_open_element
//   newAEAD                          dh.go:23-40 (both packages)  -> vss_kdf: the first 32 bytes of HKDF-SHA256 with info
//   Rabin's share check              rabin/vss.go:611-651         -> ed_vss_htab, ed_deal_check2_lane
// A seal parks three points per element -- DHKey = dh B, R = k B, pre = dh pub -- for ONE shared inversion; the pass
// after the encoder signs DHKey (one SHA-512 block: R || A || DHKey is 96 bytes), derives the AEAD key from pre and the
// context and streams the deal under the all-zero nonce with the context as additional data.  A check of Rabin's
// equation runs the ladder for g H from H's window table, built ONCE per polynomial by the decode pass, adds f B from
// the comb into the same accumulator and compares with the evaluation projectively, as ed_deal_check_lane does.
// Compiles with g++ too (tests/vss_harness.cpp runs these programs on the CPU against the oracle).
#pragma once
#include "ed25519_dkg.cuh"
#include "ed25519_verify.cuh"

namespace kyb {

constexpr size_t VSS_OVERHEAD = 16;  // the GCM tag behind a deal's ciphertext
// the context: 32 bytes in share/vss/pedersen (SHA-256, dh.go:43-51), 128 in share/vss/rabin (the suite's XOF,
// rabin/dh.go:42-66); it is read as little-endian words where it lies, never copied into registers
constexpr size_t VSS_CTX_PEDERSEN = 32, VSS_CTX_RABIN = 128;

// Sign's two points, byte for byte kyb_ed25519_mul_base's at flags 0
KYB_DEV void ed_schnorr_points_lane(ge_p3& R, ge_p3& A, const uint32_t kw[8], const uint32_t xw[8], const int32_t* __restrict__ wide) {
    int8_t e[65];
    recode16(e, kw, false);
    ed_comb_mul_base(R, e, wide);
    recode16(e, xw, false);
    ed_comb_mul_base(A, e, wide);
}

// S = k + h x mod l for any 32 bytes of k and x and h < l (schnorr.go:70-72): x R mod l, times h; k R mod l, times 1
KYB_HD void ed_schnorr_response(uint32_t (&S)[8], const uint32_t kw[8], const uint32_t xw[8], const uint32_t (&hw)[8],
                                const sf::Mod& m) {
    uint32_t k[8], x[8], t[8], u[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        k[i] = kw[i];
        x[i] = xw[i];
    }
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    sf::mont_mul(t, x, m.r2, m);
    sf::mont_mul(u, t, hw, m);  // x h mod l
    sf::mont_mul(t, k, m.r2, m);
    sf::mont_mul(k, t, one, m);  // k mod l
    sf::add_mod(S, k, u, m);
}

// The pass after the encoder of one signature: sig = R || S over msg[0 .. len), h reduced as the verify lane reduces it
KYB_DEV void ed_schnorr_sign_element(uint32_t (&sig)[16], const uint32_t rw[8], const uint32_t aw[8], const uint32_t kw[8],
                                     const uint32_t xw[8], const uint8_t* __restrict__ msg, size_t len, const sf::Mod& m) {
    uint32_t hw[8], S[8];
    ed_hram(hw, rw, aw, msg, len, m);
    ed_schnorr_response(S, kw, xw, hw, m);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        sig[i] = rw[i];
        sig[8 + i] = S[i];
    }
}

// h = SHA-512(R || A || M) mod l for a message of 32 bytes given as eight little-endian words: ONE block (96 bytes, the
// 0x80, the length)
KYB_DEV void ed_hram96(uint32_t (&hw)[8], const uint32_t rw[8], const uint32_t aw[8], const uint32_t mw[8], const sf::Mod& m) {
    uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    uint64_t w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[i] = ed_be64(rw[2 * i], rw[2 * i + 1]);
        w[4 + i] = ed_be64(aw[2 * i], aw[2 * i + 1]);
        w[8 + i] = ed_be64(mw[2 * i], mw[2 * i + 1]);
    }
    w[12] = 0x8000000000000000ull;
    w[13] = w[14] = 0;
    w[15] = 96 * 8;
    sha512_compress_regs(h, w);
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t le = __builtin_bswap64(h[i]);
        x[2 * i] = (uint32_t)le;
        x[2 * i + 1] = (uint32_t)(le >> 32);
    }
    sc_reduce512(hw, x, m);
}

// HMAC-SHA256(key, info || 01) for an info of nwords little-endian words read at cw: the expand step's T1 (RFC 5869).
// The message is streamed block by block: word j of it is info's word j byte-swapped, then 01 and the padding's 80.
KYB_HD void hmac_sha256_info(uint32_t (&out)[8], const uint32_t (&key)[8], const uint32_t* cw, int nwords) {
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t h[8], g[8], blk[16];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = iv[i];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = (i < 8 ? key[i] : 0u) ^ 0x36363636u;
    sha256_block_inl(h, blk);
    const int mbytes = 4 * nwords + 1, nb = (mbytes + 9 + 63) / 64;
#pragma unroll 1
    for (int b = 0; b < nb; b++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int j = 16 * b + i;
            blk[i] = j < nwords ? __builtin_bswap32(cw[j]) : (j == nwords ? 0x01800000u : 0u);
        }
        if (b == nb - 1) blk[15] = (uint32_t)(64 + mbytes) * 8;
        sha256_block_inl(h, blk);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) g[i] = iv[i];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = (i < 8 ? key[i] : 0u) ^ 0x5c5c5c5cu;
    sha256_block_inl(g, blk);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = i < 8 ? h[i] : 0u;
    blk[8] = 0x80000000u;
    blk[15] = (64 + 32) * 8;
    sha256_block_inl(g, blk);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = g[i];
}

// newAEAD's key (dh.go:23-40): the first 32 bytes of HKDF-SHA256(secret = pre's 32 bytes, salt = nil, info = ctx), one
// expand step: PRK = HMAC(0^32, pre), key = T1 = HMAC(PRK, ctx || 01).  pre: eight little-endian words; cw: the
// context's cwords little-endian words.
KYB_HD void vss_kdf(uint32_t (&key)[8], const uint32_t pre[8], const uint32_t* cw, int cwords) {
    uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prk[8], msg[9];
#pragma unroll
    for (int i = 0; i < 8; i++) msg[i] = __builtin_bswap32(pre[i]);
    msg[8] = 0;
    hmac_sha256_short(prk, zero, msg, 32);
    hmac_sha256_info(key, prk, cw, cwords);
}

// EncryptedDeal's three points: K = dh B (DHKey), D = dh pub (pre) and, by ed_vss_seal_nonce_point, R = k B.
// ED_DKG_ST_BAD_POINT with every point the identity when pub does not decode.
template <class Tab>
KYB_DEV int ed_vss_seal_lane(ge_p3& K, ge_p3& D, const uint32_t dw[8], const uint32_t pw[8], const int32_t* __restrict__ wide,
                             Tab& tab) {
    return ed_ecies_seal_lane(K, D, dw, pw, wide, tab);
}
KYB_DEV void ed_vss_seal_nonce_point(ge_p3& R, const uint32_t kw[8], int st, const int32_t* __restrict__ wide) {
    int8_t e[65];
    recode16(e, kw, false);
    ed_comb_mul_base(R, e, wide);
    if (st != ED_DKG_ST_OK) ge_p3_0(R);
}

// The pass after the encoder of one sealed element.  enc: the encodings of DHKey, R and pre, eight words each; aw: the
// dealer's public key as the caller gave it; cw: the context's cwords words.  slot[0 .. len + 16) = Seal(key, 0^12, msg, ctx);
// dhkey and sig are the element's other two outputs.  All three are zero when st != 0.
template <class RK>
KYB_DEV void ed_vss_seal_element(uint8_t* slot, uint32_t (&dhkey)[8], uint32_t (&sig)[16], const uint8_t* msg, uint64_t len,
                                 const uint32_t* enc, const uint32_t kw[8], const uint32_t xw[8], const uint32_t aw[8],
                                 const uint32_t* cw, int cwords, int st, const sf::Mod& m, RK& rk, const uint8_t* sbox) {
    if (st != ED_DKG_ST_OK) {
        for (uint64_t k = 0; k < len + VSS_OVERHEAD; k++) slot[k] = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) sig[i] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) dhkey[i] = 0;
        return;
    }
    uint32_t hw[8], S[8];
    ed_hram96(hw, enc + 8, aw, enc, m);
    ed_schnorr_response(S, kw, xw, hw, m);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        dhkey[i] = enc[i];
        sig[i] = enc[8 + i];
        sig[8 + i] = S[i];
    }
    uint32_t key[8];
    vss_kdf(key, enc + 16, cw, cwords);
    aes256_expand(rk, key, sbox);
    const uint32_t nonce[3] = {0, 0, 0};
    gcm_seal_aad(slot, msg, len, nonce, rk, sbox, [cw](int i) { return __builtin_bswap32(cw[i]); }, cwords / 4);
}

// decryptDeal's point D = x DHKey for a cipher of len bytes: ED_ST_ECIES_SHORT when it is shorter than a tag,
// ED_DKG_ST_BAD_POINT when DHKey does not decode; D is the identity with either.
template <class Tab>
KYB_DEV int ed_vss_open_lane(ge_p3& D, const uint32_t xw[8], const uint32_t kw[8], uint64_t len, Tab& tab) {
    uint32_t pw[8] = {0x01, 0, 0, 0, 0, 0, 0, 0};  // a short element runs the ladder on the identity's encoding
    const bool longenough = len >= VSS_OVERHEAD;
    if (longenough) {
#pragma unroll
        for (int i = 0; i < 8; i++) pw[i] = kw[i];
    }
    ge_p3 A;
    const bool ok = ge_p3_fromwords(A, pw);
    int8_t e[65];
    recode16(e, xw, false);
    ge_scalarmult_w4<false, true>(D, e, A, false, tab, 63);
    if (!ok || !longenough) ge_p3_0(D);
    return !longenough ? ED_ST_ECIES_SHORT : (ok ? ED_DKG_ST_OK : ED_DKG_ST_BAD_POINT);
}

// The AEAD pass of one element to open, ct[0 .. len): the plaintext (len - 16 bytes) at slot, zero behind it up to
// slot + len; a status other than 0 leaves slot[0 .. len) all zero.  Returns the element's final status.
template <class RK>
KYB_HD int ed_vss_open_element(uint8_t* slot, const uint8_t* ct, uint64_t len, const uint32_t pre[8], const uint32_t* cw, int cwords,
                               int st, RK& rk, const uint8_t* sbox) {
    uint64_t done = 0;
    if (st == ED_DKG_ST_OK) {
        uint32_t key[8];
        vss_kdf(key, pre, cw, cwords);
        aes256_expand(rk, key, sbox);
        const uint32_t nonce[3] = {0, 0, 0};
        done = len - VSS_OVERHEAD;
        if (!gcm_open_aad(slot, ct, done, nonce, rk, sbox, [cw](int i) { return __builtin_bswap32(cw[i]); }, cwords / 4)) st = ED_ST_ECIES_AUTH;
    }
    for (uint64_t k = done; k < len; k++) slot[k] = 0;
    return st;
}

// ----------------------------------------------------------------------------------------------- Rabin's share check
// H decoded and its window table (j + 1) H, j < 8, written where the checks of its polynomial read it; false when H
// does not decode (the table is then the identity's)
template <class Tab>
KYB_DEV bool ed_vss_htab(Tab& tab, const uint32_t w[8]) {
    ge_p3 H;
    const bool ok = ge_p3_fromwords(H, w);
    ge_window_table<true>(tab, H);
    return ok;
}

// h = sum_i e[i] 16^i H from H's table: ge_scalarmult_w4's chain at flags 0 without the table's construction, so the
// value is kyb_ed25519_mul's for every 32 bytes of scalar
template <class Tab>
KYB_DEV void ed_vss_ladder_from_table(ge_p3& h, const int8_t e[65], const Tab& tab) {
    ge_p1p1 t;
    ge_p3 u;
    ge_p2 r;
    ge_cached c;
    ge_p3_0(u);
    select_cached(c, tab, e[63]);
    ge_add(t, u, c);
    EdDigitQueue q;
    q.init(e);
    q.shl4();  // digit 62 to the top nibble
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        const int d = q.pop();
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            ge_p1p1_to_p2(r, t);
            ge_dbl(t, r.X, r.Y, r.Z);
        }
        ge_p1p1_to_p3(u, t);
        select_cached(c, tab, d);
        ge_add(t, u, c);
    }
    ge_p1p1_to_p3(h, t);
}

// Equal(Add(Mul(f, nil), Mul(g, H)), PubPoly.Eval(idx).V) (rabin/vss.go:611-651): neither scalar is reduced; the
// verdict is projective, with no inversion
template <class Tab>
KYB_DEV bool ed_deal_check2_lane(const uint32_t fw[8], const uint32_t gw[8], const ge_precomp* __restrict__ aff, size_t t,
                                 uint32_t idx, const int32_t* __restrict__ wide, const Tab& htab) {
    ge_p3 l;
    int8_t e[65];
    recode16(e, gw, false);
    ed_vss_ladder_from_table(l, e, htab);
    recode16(e, fw, false);
    {
        ge_precomp p;
        ge_p1p1 r;
        EdCombDigits<ED_COMB_G> digits(e);
#pragma unroll 1
        for (int k = 0; k < EdWide::POS_CT; k++) {
            const int d = digits.next(k);
            select_precomp_tab<EdWide::ENT>(p, wide, k, d);
            ge_madd(r, l, p);
            ge_p1p1_to_p3(l, r);
        }
    }
    ge_p3 v;
    ed_deal_eval(v, aff, t, (uint64_t)idx + 1);
    fe a, b, d;
    fe_mul(a, l.X, v.Z);
    fe_mul(b, v.X, l.Z);
    fe_sub(d, a, b);
    bool same = !fe_isnonzero(d);
    fe_mul(a, l.Y, v.Z);
    fe_mul(b, v.Y, l.Z);
    fe_sub(d, a, b);
    same &= !fe_isnonzero(d);
    return same;
}

}  // namespace kyb
