// Ed25519 proof predicates (proof/proof.go), one element per lane: the linear combination a Rep predicate commits to
// and checks, and the one challenge of a hash-based proof.
//
// Replaces, in the reference:
//   proof repPred.commit          proof.go:203-237   -> ed_lincomb_lane (V = w P + v_1 B_1 + ... + v_k B_k)
//   proof repPred.verify          proof.go:298-322   -> ed_lincomb_lane (c P + r_1 B_1 + ... ), compared with V on bytes
//   proof hashVerifier.PubRand    hash.go:111-142    -> ed_fs_challenge_lane (Reseed, Write(proof bytes), Scalar.Pick)
//   xof/blake2xb New, Reseed      blake.go:19-41, 55-74
// The combination is ONE Straus-Shamir chain over up to eight window tables: one chain of doublings, one addition per
// term and window (ge_double_scalarmult_w4 of ed25519_verify.cuh is the two-term case).  The tables of a lane's own
// points live in the lane's slab (TabGlobal); the tables of the points a batch shares are built once per call and only
// read.  Eight digit queues (64 registers) do not fit beside the point state, so every scalar's digits are parked in
// memory as the 32 bytes of s + 0x0888...8: nibble i < 63 of that sum is recode16's digit e[i] plus 8, and the sum's
// bits from 252 up are e[63] before recode16 settles the top (ed_effective_scalar states the same identity).
//
// Every term has kyb_ed25519_mul's value under the flag: the digits are recode16's, so an unreduced scalar and a scalar
// >= 2^255 behave as there.  A nil term -- Mul(s, nil), the standard base -- has geScalarMultBase's value whatever
// the flag (point.go:243; ed25519_ring.cuh keeps the same rule): a top digit above 8 is dropped.  Under KYB_F_VARTIME
// the chain reads digit 63 from a nibble, which holds [-8, 7]; a nil term's top digit of exactly 8 is parked as
// -8 at position 63 and 1 at position 64, the same integer.
// Compiles with g++ too (tests/proof_harness.cpp runs these lane programs on the CPU against the oracle).
#pragma once
#include "ed25519_ring.cuh"

namespace kyb {

constexpr int ED_LINCOMB_MAX_OWN = 4, ED_LINCOMB_MAX_SHARED = 4;

// p = a + 0x0888...8 (63 nibbles of 8); returns the sum's bits from 252 up, in [0, 16]: recode16's e[63] before the top
// digit is carried or dropped
KYB_DEV int ed_lincomb_bias(uint32_t (&p)[8], const uint32_t a[8]) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t s = (uint64_t)a[j] + (j < 7 ? 0x88888888u : 0x08888888u) + c;
        p[j] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
    return (int)((c << 4) | (p[7] >> 28));
}

// tab = the window table of a point the batch shares: the standard base's for a nil term (w is then not read), else of
// the point w encodes; false when w does not decode (the table is then of no point)
KYB_DEV bool ed_lincomb_shared_table(int4* tab, const uint32_t* __restrict__ w, bool nil) {
    ge_p3 A;
    bool good = true;
    if (nil) {
        A.X = fe_bx(); A.Y = fe_by(); fe_1(A.Z); A.T = fe_bt();
    } else {
        uint32_t v[8];
        load_words8(v, w);
        good = ge_p3_fromwords(A, v);
    }
    TabGlobal t{tab};
    ge_window_table(t, A);
    return good;
}

// One lane's memory.  Word w of scalar j's parked digits is digits[(8 j + w) * dstride]: a block's lanes interleave
// their columns, so a wave's load of one word is 64 consecutive words.
struct EdLincombMem {
    int4* own_tab;       // the lane's ko window tables: table j at own_tab + 80 j
    const int4* sh_tab;  // the call's ks shared tables: table j at sh_tab + 80 j (nobody writes them during the chain)
    uint32_t* digits;
    size_t dstride;
};

// h = sum_{j < ko} s_j own_j + sum_{j < ks} s_{ko + j} shared_j; false when an own point does not decode (h is then
// the identity).  scalars: (ko + ks) x 8 words, own terms first; own: ko x 8 words.  Bit j of nil_mask: shared term j is
// Mul(s, nil).  Every lane of a wave takes the same path through the windows (the variable-time chain's wave reductions
// want every lane).
KYB_DEV bool ed_lincomb_lane(ge_p3& h, int ko, int ks, uint32_t nil_mask, const uint32_t* __restrict__ scalars,
                             const uint32_t* __restrict__ own, bool full, const EdLincombMem& mem) {
    const int K = ko + ks;
    bool ok = true;
#pragma unroll 1
    for (int j = 0; j < ko; j++) {  // one point at a time: decoded, its table written, forgotten
        uint32_t w[8];
        load_words8(w, own + 8 * j);
        ok &= ed_ring_table(mem.own_tab + 80 * j, w);
    }
    int top = 63;
    if (full) {
        top = 0;
#pragma unroll 1
        for (int j = 0; j < K; j++) {
            uint32_t sw[8];
            load_words8(sw, scalars + 8 * j);
            const int t = wave_top_digit(sw);
            top = t > top ? t : top;
        }
    }
    ge_p1p1 t;
    ge_p3 u;
    ge_p2 r;
    ge_cached c;
    ge_p3_0(u);
    ge_cached_0(c);
    ge_add(t, u, c);  // the identity, in the form the chain keeps between additions
    // the terms are told apart by address, never by selecting between register arrays
    auto table = [&](int j) { return TabGlobal{const_cast<int4*>(j < ko ? mem.own_tab + 80 * j : mem.sh_tab + 80 * (j - ko))}; };
    // Park every scalar's digits and add the one digit that does not fit a nibble: e[63] in [0, 8] on the
    // constant-structure path, e[64] in {0, 1} under KYB_F_VARTIME (nobody has it unless top is 64).
#pragma unroll 1
    for (int j = 0; j < K; j++) {
        uint32_t sw[8], p[8];
        load_words8(sw, scalars + 8 * j);
        int e63 = ed_lincomb_bias(p, sw), e64 = 0;
        const bool nil = j >= ko && ((nil_mask >> (j - ko)) & 1u);
        if (!full || nil) {
            if (e63 > 8) e63 = 0;
            if (full && e63 == 8) {
                e63 = -8;
                e64 = 1;
            }
        } else {
            e64 = (e63 + 8) >> 4;
            e63 -= e64 << 4;
        }
        p[7] = (p[7] & 0x0fffffffu) | ((uint32_t)((e63 + 8) & 15) << 28);  // read under KYB_F_VARTIME only
#pragma unroll
        for (int w = 0; w < 8; w++) mem.digits[(size_t)(8 * j + w) * mem.dstride] = p[w];
        if (!full || top == 64) {
            ge_p1p1_to_p3(u, t);
            select_cached(c, table(j), full ? e64 : e63);
            ge_add(t, u, c);
        }
    }
#pragma unroll 1
    for (int i = full ? (top < 63 ? top : 63) : 62; i >= 0; i--) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            ge_p1p1_to_p2(r, t);
            ge_dbl(t, r.X, r.Y, r.Z);
        }
#pragma unroll 1
        for (int j = 0; j < K; j++) {
            const int d = (int)((mem.digits[(size_t)(8 * j + (i >> 3)) * mem.dstride] >> (4 * (i & 7))) & 15u) - 8;
#if defined(__HIP_DEVICE_COMPILE__)
            if (full && __ballot(d != 0) == 0) continue;  // no lane adds anything for this term in this window
#endif
            ge_p1p1_to_p3(u, t);
            select_cached(c, table(j), d);
            ge_add(t, u, c);
        }
    }
    ge_p1p1_to_p3(h, t);
    if (!ok) ge_p3_0(h);
    return ok;
}

// ------------------------------------------------------------------------------------------- the hash-based challenge
// Eight stream bytes from position pos of a byte string of len bytes, little-endian, zero past the end.  The string
// has any alignment.
KYB_DEV uint64_t ed_fs_word(const uint8_t* __restrict__ p, size_t len, size_t pos) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 7; k >= 0; k--) v = (v << 8) | (pos + k < len ? (uint64_t)p[pos + k] : 0u);
    return v;
}

// The root hash of blake2b.NewXOF(OutputLengthUnknown, key) after Write(pre), Write(tail): key of keylen bytes (0..64,
// its words zero beyond), pre nullptr or 64 bytes as words, tail of tail_len bytes.  The key is a zero-padded block of
// its own; a stream of no bytes at all is one empty final block.
KYB_DEV void ed_fs_root(uint64_t (&h)[8], const uint64_t key[8], uint32_t keylen, const uint64_t* pre,
                        const uint8_t* __restrict__ tail, size_t tail_len) {
    blake2xb_root_iv_keyed(h, keylen);
    const size_t kb = keylen ? 128 : 0, pb = pre ? 64 : 0, total = kb + pb + tail_len;
    const size_t nblk = total ? (total + 127) / 128 : 1;
    uint64_t m[16];
#pragma unroll 1
    for (size_t b = 0; b < nblk; b++) {
        if (kb && b == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                m[i] = key[i];
                m[8 + i] = 0;
            }
        } else {
            const size_t at = 128 * b - kb;  // position in pre || tail
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const size_t q = at + 8 * i;
                uint64_t v = 0;
                if (q >= pb) v = ed_fs_word(tail, tail_len, q - pb);
                m[i] = v;
            }
            if (pb && at == 0) {
#pragma unroll
                for (int i = 0; i < 8; i++) m[i] = pre[i];
            }
        }
        const bool last = b + 1 == nblk;
        blake2b_compress_regs(h, m, last ? total : 128 * (b + 1), last);
    }
}

// Output node `node` of the stream with root hash `root`
KYB_DEV void ed_fs_node(uint64_t (&o)[8], const uint64_t root[8], uint32_t node) {
    uint64_t m[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        m[i] = root[i];
        m[8 + i] = 0;
    }
    blake2xb_node_iv(o, node);
    blake2b_compress_regs(o, m, 64, true);
}

// c = Scalar.Pick(X) for X = blake2xb.New(name) and, when data_len != 0, X.Reseed() and X.Write(data): what
// hashVerifier.PubRand draws after the prover's messages (hash.go:111-142).  Reseed (blake.go:55-74) reads 128 stream
// bytes, keys a new XOF with the first 64 and writes the other 64.  With data_len == 0 nothing was consumed and the pick
// comes from New(name) itself (hash.go:46-65).  Returns ED_ST_OK, or ED_ST_PICK_EXHAUSTED (c zero) when
// ED_PICK_MAX_NODES output nodes held no scalar below l.
KYB_DEV int ed_fs_challenge_lane(uint32_t (&c)[8], const uint8_t* __restrict__ name, size_t name_len,
                                 const uint8_t* __restrict__ data, size_t data_len) {
    uint64_t root[8], key[8];
    const size_t keylen = name_len < 64 ? name_len : 64;
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = ed_fs_word(name, keylen, 8 * i);
    ed_fs_root(root, key, (uint32_t)keylen, nullptr, name + keylen, name_len - keylen);
    if (data_len) {
        uint64_t pre[8];
        ed_fs_node(key, root, 0);
        ed_fs_node(pre, root, 1);
        ed_fs_root(root, key, 64, pre, data, data_len);
    }
    bool done = false;
#pragma unroll 1
    for (int node = 0; node < ED_PICK_MAX_NODES && !done; node++) {
        uint64_t o[8];
        ed_fs_node(o, root, (uint32_t)node);
        done = ed_pick_draw(c, o[0], o[1], o[2], o[3]);
        if (!done) done = ed_pick_draw(c, o[4], o[5], o[6], o[7]);
    }
    if (!done) {
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = 0;
        return ED_ST_PICK_EXHAUSTED;
    }
    return ED_ST_OK;
}

}  // namespace kyb
