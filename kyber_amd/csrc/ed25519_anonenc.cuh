// sign/anon Encrypt / Decrypt on Ed25519 (enc.go): the lane programs of ed25519_anonenc.hip.
//
// Replaces, in the reference:
//   encryptKey: key.Pair.Gen's X = x B, xb = Private.MarshalBinary()   enc.go:31-40     -> ed_anon_seal_head
//   header(): S = x Y_i, XOF(MarshalBinary(S)).XORKeyStream(xb)         enc.go:11-27     -> ed_anon_table / ed_anon_ladder,
//                                                                                         ed_anon_slot
//   decryptKey: the length checks, X, S = priv X, xb, x B = X           enc.go:44-88     -> ed_anon_open_head
//   decryptKey: the regenerated header against the ciphertext's         enc.go:90-99     -> ed_anon_slot + a comparison
//   Encrypt's body: ctx = msg ^ XOF(xb), mac = XOF(ctx)[0:16]           enc.go:127-145   -> ed_anon_seal_body
//   Decrypt's body: the length, the MAC, then the plaintext             enc.go:174-191   -> ed_anon_open_body
//   xof/blake2xb New(seed), Read, XORKeyStream                          blake.go:19-104  -> ed_anon_stream32, ed_anon_xor_stream,
//                                                                                         ed_anon_mac
// Encrypt multiplies by the clamped, UNREDUCED x and carries xb = x mod l in the slots; Decrypt multiplies by the 32 bytes
// it recovered, unreduced.  Both have kyb_ed25519_mul's value at flags 0 (recode16's constant-structure digits), so a ring
// member with a torsion component makes Decrypt reject what Encrypt made, as the reference's does.
//
// The hash: suite.XOF(seed) keys BLAKE2b with the first <= 64 seed bytes (a zero-padded block of its own) and writes the
// rest; an empty seed is a keyless root over no data.  BLAKE2b compresses a block only when more input follows, so a
// last block that is exactly full is the final one (ed25519_ring.cuh).  Messages, ciphertexts and plaintexts lie at
// arbitrary byte offsets: every access to them is byte-wise.
// Compiles with g++ too (tests/anon_enc_harness.cpp runs these programs on the CPU against the oracle).
#pragma once
#include "ed25519_dkg.cuh"
#include "ed25519_ring.cuh"

namespace kyb {

// per-element status values of the anon calls (include/kyber_hip.h; ed25519_anonenc.hip static_asserts the match)
constexpr int ED_ST_ANON_SHORT = 11, ED_ST_ANON_INVALID = 12, ED_ST_ANON_MAC = 13;
constexpr size_t ED_ANON_MAX_RING = 4096;  // KYB_ANON_MAX_RING of include/kyber_hip.h
constexpr size_t ANON_MAC = 16;            // macSize, enc.go:117
// a ciphertext is this much longer than its message: X, ring slots, the MAC
KYB_HD size_t anon_overhead(size_t ring) { return 32 + 32 * ring + ANON_MAC; }

using Tab29 = TabGlobal_t<fe29>;

KYB_HD void ed_anon_load32(uint32_t (&w)[8], const uint8_t* __restrict__ p) {
#pragma unroll
    for (int i = 0; i < 8; i++)
        w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
}
KYB_HD void ed_anon_store32(uint8_t* __restrict__ p, const uint32_t (&w)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) p[4 * i + k] = (uint8_t)(w[i] >> (8 * k));
}
KYB_HD void ed_anon_zero(uint8_t* __restrict__ p, uint64_t n) {
#pragma unroll 1
    for (uint64_t b = 0; b < n; b++) p[b] = 0;
}

// ------------------------------------------------------------------------------------------------------- the points
// tab = the nine-limb window table of the point w encodes; false when w does not decode (the table is then of no point)
KYB_DEV bool ed_anon_table(int4* tab, const uint32_t w[8]) {
    ge29_p3 A;
    const bool ok = ge_p3_fromwords(A, w);
    Tab29 t{tab};
    ge_window_table<true>(t, A);  // A.Z = 1: decoded just above
    return ok;
}

// h = sum_i e[i] 16^i A over A's window table, built by someone else: ge_scalarmult_w4's constant-structure walk (top
// digit 63, no window skipped) without its table build.  The digits are read from the top nibble of a pack that moves
// up, as there.
template <class P3, class Tab>
KYB_DEV void ed_anon_ladder(P3& h, const int8_t e[65], const Tab& tab) {
    typedef ge_t<decltype(h.X)> G;
    typename G::p1p1 t;
    P3 u;
    typename G::p2 r;
    typename G::cached c;
    ge_p3_0(u);
    select_cached(c, tab, e[63]);
    ge_add(t, u, c);
    uint32_t pk[8];
    ed_pack_digits(pk, e);
    auto shl4 = [&pk]() {
#pragma unroll
        for (int j = 7; j > 0; j--) pk[j] = (pk[j] << 4) | (pk[j - 1] >> 28);
        pk[0] <<= 4;
    };
    shl4();  // digit 62 to the top nibble
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        const int d = (int)(pk[7] >> 28) - 8;  // e[i]
        shl4();
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        ge_p1p1_to_p2(r, t);
        ge_dbl(t, r.X, r.Y, r.Z);
        ge_p1p1_to_p3(u, t);
        select_cached(c, tab, d);
        ge_add(t, u, c);
    }
    ge_p1p1_to_p3(h, t);
}

// S = s Y with kyb_ed25519_mul's value at flags 0, from the shared table of Y
KYB_DEV void ed_anon_product_shared(ge29_p3& S, const uint32_t sw[8], const int4* __restrict__ ytab) {
    int8_t e[65];
    recode16(e, sw, false);
    const Tab29 tab{const_cast<int4*>(ytab)};
    ed_anon_ladder(S, e, tab);
}
// ... from Y's bytes, its table built in the lane's own slab; false, with S the identity, when Y does not decode
KYB_DEV bool ed_anon_product_own(ge29_p3& S, const uint32_t sw[8], const uint32_t yw[8], int4* __restrict__ own) {
    ge29_p3 A;
    const bool ok = ge_p3_fromwords(A, yw);
    int8_t e[65];
    recode16(e, sw, false);
    Tab29 tab{own};
    ge_scalarmult_w4<false, true>(S, e, A, false, tab, 63);  // A.Z = 1: decoded just above
    if (!ok) ge_p3_0(S);
    return ok;
}

// ---------------------------------------------------------------------------------------------------------- the hash
// ks = XOF(seed)[0:32] for a 32-byte seed: the keyed root and output node 0, one compression site for both
KYB_HD void ed_anon_stream32(uint32_t (&ks)[8], const uint32_t seed[8]) {
    uint64_t h[8], m[16];
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = (uint64_t)seed[2 * i] | ((uint64_t)seed[2 * i + 1] << 32);
#pragma unroll
    for (int i = 4; i < 16; i++) m[i] = 0;
    blake2xb_root_iv(h);
    uint64_t t = 128;  // the key block counts in full
#pragma unroll 1
    for (int it = 0; it < 2; it++) {
        blake2b_compress_regs(h, m, t, true);
        if (it == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) m[i] = h[i];  // the root hash is the node's message
            t = 64;
            blake2xb_node_iv(h, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ks[2 * i] = (uint32_t)h[i];
        ks[2 * i + 1] = (uint32_t)(h[i] >> 32);
    }
}

// one header slot (enc.go:19-24): xb ^ XOF(enc)[0:32], enc the 32 bytes MarshalBinary wrote for the shared secret
KYB_HD void ed_anon_slot(uint32_t (&s)[8], const uint32_t enc[8], const uint32_t xb[8]) {
    ed_anon_stream32(s, enc);
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] ^= xb[i];
}

// dst[0 .. len) = src[0 .. len) ^ XOF(xb)[0 .. len): the root once, then one compression per 64 bytes
KYB_HD void ed_anon_xor_stream(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t len, const uint32_t xb[8]) {
    if (len == 0) return;
    uint64_t h[8], m[16];
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = (uint64_t)xb[2 * i] | ((uint64_t)xb[2 * i + 1] << 32);
#pragma unroll
    for (int i = 4; i < 16; i++) m[i] = 0;
    blake2xb_root_iv(h);
    uint64_t t = 128;
    const uint64_t nodes = (len + 63) / 64;
#pragma unroll 1
    for (uint64_t it = 0; it <= nodes; it++) {  // trip 0: the root; trip it: output node it - 1
        blake2b_compress_regs(h, m, t, true);
        if (it == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) m[i] = h[i];
            t = 64;
        } else {
            const uint64_t base = 64 * (it - 1), cnt = len - base;
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if ((uint64_t)(8 * i + k) < cnt) dst[base + 8 * i + k] = src[base + 8 * i + k] ^ (uint8_t)(h[i] >> (8 * k));
        }
        blake2xb_node_iv(h, (uint32_t)it);
    }
}

// m = the `avail` <= 128 bytes at p, zero beyond
KYB_HD void ed_anon_load_block(uint64_t (&m)[16], const uint8_t* __restrict__ p, uint64_t avail) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
        uint64_t v = 0;
#pragma unroll
        for (int k = 7; k >= 0; k--) v = (v << 8) | ((uint64_t)(8 * i + k) < avail ? (uint64_t)p[8 * i + k] : 0ull);
        m[i] = v;
    }
}

// mac = XOF(ctx)[0:16]: the first <= 64 bytes of ctx are the key (a block of its own), the rest is data in 128-byte
// blocks of which the last -- full or not -- is the final one; an empty ctx is a keyless root over one empty block.
// One compression site serves the root's blocks and output node 0.
KYB_HD void ed_anon_mac(uint32_t (&mac)[4], const uint8_t* __restrict__ ctx, uint64_t len) {
    const uint64_t keylen = len < 64 ? len : 64, dlen = len - keylen;
    const uint64_t nblk = 1 + (dlen + 127) / 128;  // the root's compressions
    uint64_t h[8], m[16];
    blake2xb_root_iv_keyed(h, (uint32_t)keylen);
#pragma unroll 1
    for (uint64_t it = 0; it <= nblk; it++) {
        uint64_t t = 64;
        bool last = true;
        if (it == 0) {
            ed_anon_load_block(m, ctx, keylen);
            t = len ? 128 : 0;
            last = dlen == 0;
        } else if (it < nblk) {
            const uint64_t base = 128 * (it - 1), left = dlen - base;
            ed_anon_load_block(m, ctx + 64 + base, left < 128 ? left : 128);
            last = it == nblk - 1;
            t = 128 + (last ? dlen : 128 * it);
        }
        blake2b_compress_regs(h, m, t, last);
        if (it == nblk - 1) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                m[i] = h[i];
                m[8 + i] = 0;
            }
            blake2xb_node_iv(h, 0);
        }
    }
    mac[0] = (uint32_t)h[0];
    mac[1] = (uint32_t)(h[0] >> 32);
    mac[2] = (uint32_t)h[1];
    mac[3] = (uint32_t)(h[1] >> 32);
}

// ---------------------------------------------------------------------------------------------------------- the heads
// xb = x mod l for any 32 bytes x (scalar.MarshalBinary through toInt): the verify unit's reduction with a zero high half
KYB_HD void ed_anon_reduce(uint32_t (&xb)[8], const uint32_t x[8], const sf::Mod& m) {
    uint32_t wide[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        wide[i] = x[i];
        wide[8 + i] = 0;
    }
    sc_reduce512(xb, wide, m);
}

// Encrypt's key pair as the header sees it: X = x B (kyb_ed25519_mul_base's value at flags 0) and xb = x mod l
KYB_DEV void ed_anon_seal_head(ge_p3& X, uint32_t (&xb)[8], const uint32_t xw[8], const int32_t* __restrict__ wide, const sf::Mod& m) {
    int8_t e[65];
    recode16(e, xw, false);
    ed_comb_mul_base(X, e, wide);
    ed_anon_reduce(xb, xw, m);
}

// decryptKey up to x B (enc.go:52-85) for the ciphertext ct[0 .. len): the two length checks around the decoding of X,
// S = priv X on the nine-limb ladder (its table in tab), xb = slot `mine` ^ XOF(MarshalBinary(S))[0:32] and XB = xb B on
// the comb, for the encoder and the comparison with X on canonical bytes.  Returns ED_ST_ANON_SHORT, ED_DKG_ST_BAD_POINT
// or 0; with a status xb is zero, XB the identity, and no byte past what the checks allow is read.
KYB_DEV int ed_anon_open_head(ge_p3& XB, uint32_t (&xb)[8], const uint32_t pw[8], const uint8_t* __restrict__ ct, uint64_t len,
                              size_t ring, size_t mine, const int32_t* __restrict__ wide, Tab29& tab) {
    int st = len < 32 ? ED_ST_ANON_SHORT : 0;
    ge29_p3 A;
#pragma unroll
    for (int i = 0; i < 8; i++) xb[i] = 0;
    if (!st) {
        uint32_t xw[8];
        ed_anon_load32(xw, ct);
        if (!ge_p3_fromwords(A, xw)) st = ED_DKG_ST_BAD_POINT;
    }
    if (!st && len < 32 + 32 * (uint64_t)ring) st = ED_ST_ANON_SHORT;
    if (!st) {
        uint32_t sw[8];
        {
            int8_t e[65];
            recode16(e, pw, false);
            ge29_p3 S;
            ge_scalarmult_w4<false, true>(S, e, A, false, tab, 63);  // A.Z = 1: decoded just above
            ge_p3_towords(sw, S);  // this lane's own inversion: the secret is needed before the ring can run
        }
        uint32_t slot[8];
        ed_anon_load32(slot, ct + 32 + 32 * mine);
        ed_anon_slot(xb, sw, slot);
    }
    int8_t e[65];
    recode16(e, xb, false);
    ed_comb_mul_base(XB, e, wide);  // (xb = 0 with a status: the identity)
    return st;
}

// --------------------------------------------------------------------------------------------------------- the bodies
// Encrypt's body at out: ctx (len bytes) || mac; all zero with a status
KYB_HD void ed_anon_seal_body(uint8_t* __restrict__ out, const uint8_t* __restrict__ msg, uint64_t len, const uint32_t xb[8], int st) {
    if (st) {
        ed_anon_zero(out, len + ANON_MAC);
        return;
    }
    ed_anon_xor_stream(out, msg, len, xb);
    uint32_t mac[4];
    ed_anon_mac(mac, out, len);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) out[len + 4 * i + k] = (uint8_t)(mac[i] >> (8 * k));
}

// Decrypt's body (enc.go:174-191) for the element ct[0 .. len) whose header, hdrlen bytes, passed: the last length
// check, the MAC -- decided before a plaintext byte is written -- then the plaintext at out, zero behind it up to len.
// Returns the element's status; with one, out[0 .. len) is all zero.
KYB_HD int ed_anon_open_body(uint8_t* __restrict__ out, const uint8_t* __restrict__ ct, uint64_t len, uint64_t hdrlen, const uint32_t xb[8],
                             int st) {
    if (!st && len < hdrlen + ANON_MAC) st = ED_ST_ANON_SHORT;
    uint64_t mlen = 0;
    if (!st) {
        mlen = len - hdrlen - ANON_MAC;
        uint32_t mac[4];
        ed_anon_mac(mac, ct + hdrlen, mlen);
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) diff |= (uint32_t)ct[hdrlen + mlen + 4 * i + k] ^ ((mac[i] >> (8 * k)) & 0xffu);
        if (diff) st = ED_ST_ANON_MAC;
    }
    if (st) {
        ed_anon_zero(out, len);
        return st;
    }
    ed_anon_xor_stream(out, ct + hdrlen, mlen, xb);
    ed_anon_zero(out + mlen, len - mlen);
    return 0;
}

}  // namespace kyb
