// share/dkg and encrypt/ecies on Ed25519: the lane programs of ed25519_dkg.hip.
//
// Replaces, in the reference:
//   encrypt/ecies Encrypt          ecies.go:23-69    -> ed_ecies_seal_lane (R = r B on the comb, dh = r pub on the ladder),
//                                                       ecies_kdf, ed_ecies_seal_element
//   encrypt/ecies Decrypt          ecies.go:77-112   -> ed_ecies_open_lane (dh = x R), ed_ecies_open_element
//   hkdf.New(hash, dh, nil, nil)   ecies.go:115-127  -> ecies_kdf: HKDF-SHA256, 44 bytes = AES-256 key || GCM nonce
//   the share check of a deal      dkg.go:488-495, 824-832; share/poly.go:340-348, 405-409
//                                                    -> ed_deal_decode, ed_deal_check_lane
// The points of a seal or an open are parked for the shared-inversion encoder like every other fused call's; the AEAD
// pass (aes256gcm.cuh) reads their bytes.  A deal check computes both sides in one lane and compares them
// projectively -- X1 Z2 = X2 Z1 and Y1 Z2 = Y2 Z1 after a full reduction -- which is Point.Equal on re-encodings
// (point.go:81-96) for points with Z != 0, and every point the complete addition law produces from curve points has
// Z != 0: the verdict needs no inversion and no second pass.
// Compiles with g++ too (tests/dkg_harness.cpp runs these programs on the CPU against the fixtures and the oracle).
#pragma once
#include "ed25519_dev.cuh"
#include "sha256.cuh"
#include "aes256gcm.cuh"

namespace kyb {

// per-element status values of the ECIES calls (include/kyber_hip.h; ed25519_dkg.hip static_asserts the match)
constexpr int ED_DKG_ST_OK = 0, ED_DKG_ST_BAD_POINT = 1, ED_ST_ECIES_SHORT = 9, ED_ST_ECIES_AUTH = 10;
constexpr size_t ECIES_OVERHEAD = 48;  // R (32 bytes) in front, the GCM tag (16) behind

// h = s B with kyb_ed25519_mul_base's value at flags 0 (recode16's constant-structure digits on the wide comb)
KYB_DEV void ed_comb_mul_base(ge_p3& h, const int8_t e[65], const int32_t* __restrict__ wide) {
    ge_p3_0(h);
    ge_precomp t;
    ge_p1p1 r;
    EdCombDigits<ED_COMB_G> digits(e);
#pragma unroll 1
    for (int k = 0; k < EdWide::POS_CT; k++) {
        const int d = digits.next(k);
        select_precomp_tab<EdWide::ENT>(t, wide, k, d);
        ge_madd(r, h, t);
        ge_p1p1_to_p3(h, r);
    }
}

// Encrypt's two points: R = r B and D = r pub, byte for byte kyb_ed25519_mul_base's and kyb_ed25519_mul's at flags 0.
// ED_DKG_ST_BAD_POINT, with both points the identity, when pub does not decode (kyb_ed25519_unmarshal's rule).
template <class Tab>
KYB_DEV int ed_ecies_seal_lane(ge_p3& R, ge_p3& D, const uint32_t rw[8], const uint32_t pw[8], const int32_t* __restrict__ wide,
                               Tab& tab) {
    ge_p3 A;
    const bool ok = ge_p3_fromwords(A, pw);
    int8_t e[65];
    recode16(e, rw, false);
    ge_scalarmult_w4<false, true>(D, e, A, false, tab, 63);  // A.Z = 1: decoded just above
    ed_comb_mul_base(R, e, wide);
    if (!ok) {
        ge_p3_0(R);
        ge_p3_0(D);
    }
    return ok ? ED_DKG_ST_OK : ED_DKG_ST_BAD_POINT;
}

// Decrypt's point D = x R of the element ct[0 .. len): ED_ST_ECIES_SHORT before a byte of it is read when it is shorter
// than R and a tag, ED_DKG_ST_BAD_POINT when R does not decode; D is the identity with either.
template <class Tab>
KYB_DEV int ed_ecies_open_lane(ge_p3& D, const uint32_t xw[8], const uint8_t* __restrict__ ct, uint64_t len, Tab& tab) {
    uint32_t pw[8] = {0x01, 0, 0, 0, 0, 0, 0, 0};  // a short element runs the ladder on the identity's encoding
    const bool longenough = len >= ECIES_OVERHEAD;
    if (longenough) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            pw[i] = (uint32_t)ct[4 * i] | ((uint32_t)ct[4 * i + 1] << 8) | ((uint32_t)ct[4 * i + 2] << 16) | ((uint32_t)ct[4 * i + 3] << 24);
    }
    ge_p3 A;
    const bool ok = ge_p3_fromwords(A, pw);
    int8_t e[65];
    recode16(e, xw, false);
    ge_scalarmult_w4<false, true>(D, e, A, false, tab, 63);
    if (!ok || !longenough) ge_p3_0(D);
    return !longenough ? ED_ST_ECIES_SHORT : (ok ? ED_DKG_ST_OK : ED_DKG_ST_BAD_POINT);
}

// HMAC-SHA256 under a 32-byte key of a message of nbytes <= 35 bytes, all as big-endian words (msg zero past its end)
KYB_HD void hmac_sha256_short(uint32_t (&out)[8], const uint32_t (&key)[8], const uint32_t (&msg)[9], int nbytes) {
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t h[8], blk[16];
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {  // the inner hash over (key ^ ipad) || msg, then the outer over (key ^ opad) || inner
        const uint32_t pad = pass ? 0x5c5c5c5cu : 0x36363636u;
        const int nb = pass ? 32 : nbytes;
#pragma unroll
        for (int i = 0; i < 16; i++) blk[i] = (i < 8 ? key[i] : 0u) ^ pad;
        uint32_t m[9];
#pragma unroll
        for (int i = 0; i < 9; i++) m[i] = pass ? (i < 8 ? h[i] : 0u) : msg[i];
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = iv[i];
        sha256_block_inl(h, blk);
#pragma unroll
        for (int i = 0; i < 16; i++) blk[i] = i < 9 ? m[i] : 0u;
#pragma unroll
        for (int i = 0; i < 9; i++) blk[i] |= i == (nb >> 2) ? 0x80u << (24 - 8 * (nb & 3)) : 0u;
        blk[15] = (uint32_t)(64 + nb) * 8;
        sha256_block_inl(h, blk);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = h[i];
}

// key || nonce = the first 44 bytes of HKDF-SHA256(secret = dh, salt = nil, info = nil) (RFC 5869; ecies.go:115-127): a
// nil salt is 32 zero bytes, PRK = HMAC(0^32, dh), T1 = HMAC(PRK, 01), T2 = HMAC(PRK, T1 || 02); key = T1,
// nonce = T2[:12].  secret: n <= 32 bytes as big-endian words.  okm: T1 || T2 as sixteen big-endian words.
KYB_HD void hkdf_sha256_64(uint32_t (&okm)[16], const uint32_t (&secret)[8], int nbytes) {
    uint32_t key[8] = {0, 0, 0, 0, 0, 0, 0, 0}, msg[9], out[8];
#pragma unroll
    for (int i = 0; i < 8; i++) msg[i] = secret[i];
    msg[8] = 0;
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
        hmac_sha256_short(out, key, msg, nbytes);
        if (j == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                key[i] = out[i];
                msg[i] = 0;
            }
            msg[0] = 0x01000000u;
            nbytes = 1;
        } else if (j == 1) {
#pragma unroll
            for (int i = 0; i < 8; i++) okm[i] = msg[i] = out[i];
            msg[8] = 0x02000000u;
            nbytes = 33;
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) okm[8 + i] = out[i];
        }
    }
}
// dh: a point's 32 encoded bytes as the encoder's eight little-endian words
KYB_HD void ecies_kdf(uint32_t (&key)[8], uint32_t (&nonce)[3], const uint32_t dh[8]) {
    uint32_t okm[16], s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = __builtin_bswap32(dh[i]);
    hkdf_sha256_64(okm, s, 32);
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = okm[i];
#pragma unroll
    for (int i = 0; i < 3; i++) nonce[i] = okm[8 + i];
}

// The AEAD pass of one sealed element: slot[0 .. len + 48) = R || Seal(key, nonce, msg), all zero when st != 0
template <class RK>
KYB_HD void ed_ecies_seal_element(uint8_t* slot, const uint8_t* msg, uint64_t len, const uint32_t Rw[8], const uint32_t dh[8],
                                  int st, RK& rk, const uint8_t* sbox) {
    if (st != ED_DKG_ST_OK) {
        for (uint64_t k = 0; k < len + ECIES_OVERHEAD; k++) slot[k] = 0;
        return;
    }
#pragma unroll
    for (int i = 0; i < 32; i++) slot[i] = (uint8_t)(Rw[i >> 2] >> (8 * (i & 3)));
    uint32_t key[8], nonce[3];
    ecies_kdf(key, nonce, dh);
    aes256_expand(rk, key, sbox);
    gcm_seal(slot + 32, msg, len, nonce, rk, sbox);
}

// The AEAD pass of one element to open, ct[0 .. len): the plaintext (len - 48 bytes) at slot, zero behind it up to
// slot + len.  st: the point pass's status; returns the element's final status.  A status other than 0 leaves
// slot[0 .. len) all zero.
template <class RK>
KYB_HD int ed_ecies_open_element(uint8_t* slot, const uint8_t* ct, uint64_t len, const uint32_t dh[8], int st, RK& rk,
                                 const uint8_t* sbox) {
    uint64_t done = 0;
    if (st == ED_DKG_ST_OK) {
        uint32_t key[8], nonce[3];
        ecies_kdf(key, nonce, dh);
        aes256_expand(rk, key, sbox);
        done = len - ECIES_OVERHEAD;
        if (!gcm_open(slot, ct + 32, done, nonce, rk, sbox)) st = ED_ST_ECIES_AUTH;
    }
    for (uint64_t k = done; k < len; k++) slot[k] = 0;
    return st;
}

// ----------------------------------------------------------------------------------------------------- deal checks
// One commitment decoded to (y + x, y - x, 2dxy), the operand of a mixed addition; false when it does not decode
KYB_DEV bool ed_deal_decode(ge_precomp& a, const uint32_t w[8]) {
    ge_p3 p;
    const bool ok = ge_p3_fromwords(p, w);
    fe one;
    fe_1(one);
    fe_add(a.ypx, p.Y, p.X);
    fe_sub(a.ymx, p.Y, p.X);
    fe_mul(a.ypx, a.ypx, one);  // reduce the sums so the entries stay in the multiplier's input range
    fe_mul(a.ymx, a.ymx, one);
    fe_mul(a.xy2d, p.T, fe_d2());
    return ok;
}

// v = sum_j aff[j] x^j by Horner from the top coefficient (PubPoly.Eval, share/poly.go:340-348, x = 1 + index):
// [x] acc by double-and-add from x's highest set bit (x >= 1; 2^32 has 33 bits), then one mixed addition.  t = 0: the
// identity.
KYB_DEV void ed_deal_eval(ge_p3& acc, const ge_precomp* __restrict__ aff, size_t t, uint64_t x) {
    ge_p3_0(acc);
    ge_p1p1 r;
    if (t) {
        const ge_precomp top = aff[t - 1];
        ge_madd(r, acc, top);
        ge_p1p1_to_p3(acc, r);
    }
    const int hi = 63 - __builtin_clzll(x);
#pragma unroll 1
    for (size_t j = t; j-- > 1;) {
        ge_cached c;
        ge_p3_to_cached(c, acc);
        ge_p3 v = acc;
#pragma unroll 1
        for (int b = hi - 1; b >= 0; b--) {
            ge_dbl(r, v.X, v.Y, v.Z);
            ge_p1p1_to_p3(v, r);
            if ((x >> b) & 1) {
                ge_add(r, v, c);
                ge_p1p1_to_p3(v, r);
            }
        }
        const ge_precomp co = aff[j - 1];
        ge_madd(r, v, co);
        ge_p1p1_to_p3(acc, r);
    }
}

// Equal(Mul(share, nil), PubPoly.Eval(idx).V) (dkg.go:488-495): the left side has kyb_ed25519_mul_base's value for
// every 32 bytes of share (never reduced: scalar.UnmarshalBinary copies them, scalar.go:226-232)
KYB_DEV bool ed_deal_check_lane(const uint32_t sw[8], const ge_precomp* __restrict__ aff, size_t t, uint32_t idx,
                                const int32_t* __restrict__ wide) {
    ge_p3 v, l;
    ed_deal_eval(v, aff, t, (uint64_t)idx + 1);
    int8_t e[65];
    recode16(e, sw, false);
    ed_comb_mul_base(l, e, wide);
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
