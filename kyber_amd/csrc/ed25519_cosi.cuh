// Ed25519 collective signatures (sign/cosi), one element per lane: the aggregate key of a participation mask as a sum of
// table entries, and the verification of a cosignature under that key.
//
// Replaces, in the reference:
//   cosi Mask.SetMask / AggregatePublic   cosi.go:300-317   -> ed_cosi_aggregate_lane (A = sum of the enabled keys)
//   cosi Mask.CountEnabled                cosi.go:361-372   -> ed_cosi_mask_count
//   cosi Verify                           cosi.go:214-232   -> ed_cosi_check_lane (T = (r mod l) B - k A, k from SHA-512)
// A chain of cosigned blocks is n signatures over ONE roster of m keys.  The roster is decoded once per call
// (ed_cosi_roster_lane) and cut into groups of g keys, g = 4 or 8; group b's table holds the 2^g sums of its subsets in
// cached form (Y+X, Y-X, Z, 2dT), entry 0 the identity.  The tables are built in g rounds: the entry of a subset whose
// highest key is k is the entry without that key plus the key (ed_cosi_table_round), one addition per entry and no
// inversion.  A lane then adds one entry per group, picked by the mask's byte or nibble; with more than half of the keys
// enabled it walks the complemented mask and finishes with T_all - acc, T_all being the sum of every group's full
// entry.  The addition formulas are complete, so entry 0 needs no branch.
// Addresses follow the mask, which is public data in every caller.
// Compiles with g++ too (tests/cosi_harness.cpp runs these lane programs on the CPU against the oracle).  The wave
// collective (__ballot) sits behind __HIP_DEVICE_COMPILE__ and changes only what is skipped, never a value.
#pragma once
#include "ed25519_dleq.cuh"

namespace kyb {

constexpr size_t ED_COSI_MAX_ROSTER = 8192;  // KYB_COSI_MAX_ROSTER of include/kyber_hip.h
constexpr int ED_COSI_KEY_WORDS = 40;        // a decoded roster key: (X, Y, Z = 1, T), ten limbs each
constexpr int ED_COSI_ENTRY_INT4 = 10;       // a table entry: the 160 B of a cached point, TabGlobal's layout

// The point additions of a call of n elements over m keys at table width g.  A group of k keys costs 2^k - k - 1 in the
// build (entry 0 and the k single keys are copies, every other subset one addition; k = g but for a partial last
// group), T_all one per group, and a lane at most one per group: n * groups for the call.
KYB_HD size_t ed_cosi_additions(size_t n, size_t m, int g) {
    const size_t full = m / (size_t)g, rem = m % (size_t)g, nb = full + (rem ? 1 : 0);
    return full * (((size_t)1 << g) - (size_t)g - 1) + (rem ? ((size_t)1 << rem) - rem - 1 : 0) + nb + n * nb;
}
// The table width of a call: 8 where that is strictly cheaper by the count above, else 4.  For m a multiple of 8 that is
//   (m / 8) (248 + n) < (m / 4) (12 + n),   from n = 225 on;
// m <= 4 makes the same one table either way and stays at 4.
KYB_HD int ed_cosi_group_width(size_t n, size_t m) { return ed_cosi_additions(n, m, 8) < ed_cosi_additions(n, m, 4) ? 8 : 4; }
KYB_HD size_t ed_cosi_groups(size_t m, int g) { return (m + (size_t)g - 1) / (size_t)g; }
// keys of group b: g, or fewer in the last group
KYB_HD int ed_cosi_group_keys(size_t m, int g, size_t b) {
    const size_t left = m - b * (size_t)g;
    return left < (size_t)g ? (int)left : g;
}

KYB_DEV void ed_cosi_store_p3(int32_t* __restrict__ o, const ge_p3& p) {
#pragma unroll
    for (int l = 0; l < 10; l++) {
        o[l] = p.X.v[l];
        o[10 + l] = p.Y.v[l];
        o[20 + l] = p.Z.v[l];
        o[30 + l] = p.T.v[l];
    }
}
KYB_DEV void ed_cosi_load_p3(ge_p3& p, const int32_t* o) {
    load_fe(p.X, o);
    load_fe(p.Y, o + 10);
    load_fe(p.Z, o + 20);
    load_fe(p.T, o + 30);
}

// Roster key j, decoded once per call by the reference's rules (y >= p reduced, "-0" accepted, small order allowed):
// key = its (X, Y, 1, T); false when the encoding has no x (the words are then of no point)
KYB_DEV bool ed_cosi_roster_lane(int32_t* __restrict__ key, const uint32_t* __restrict__ w) {
    uint32_t v[8];
    load_words8(v, w);
    ge_p3 A;
    const bool ok = ge_p3_fromwords(A, v);
    ed_cosi_store_p3(key, A);
    return ok;
}

// Round k of group b's table, for the subset s whose highest key is k (s >> k == 1): entry[s] = entry[s without k] +
// key k.  Entry 0 is written before round 0; round k reads entries of rounds below k only.  A key at or above m (the
// last group may be partial) adds nothing: its entries are copies, and no lane reads them.
KYB_DEV void ed_cosi_table_round(int4* tables, const int32_t* roster, size_t m, int g, size_t b, int s, int k) {
    TabGlobal t{tables + (b << g) * ED_COSI_ENTRY_INT4};
    const size_t j = b * (size_t)g + (size_t)k;
    const int parent = s ^ (1 << k);
    ge_cached c;
    if (j >= m) {
        t.get(c, parent);
        t.put(s, c);
        return;
    }
    ge_p3 P;
    ed_cosi_load_p3(P, roster + j * ED_COSI_KEY_WORDS);
    if (parent == 0) {
        ge_p3_to_cached(c, P);
    } else {
        ge_p1p1 r;
        ge_p3 u;
        t.get(c, parent);
        ge_add(r, P, c);
        ge_p1p1_to_p3(u, r);
        ge_p3_to_cached(c, u);
    }
    t.put(s, c);
}
KYB_DEV void ed_cosi_table_identity(int4* tables, int g, size_t b) {
    TabGlobal t{tables + (b << g) * ED_COSI_ENTRY_INT4};
    ge_cached c;
    ge_cached_0(c);
    t.put(0, c);
}

// T_all = the sum of every group's full entry, as a tree: a lane sums the groups first, first + stride, ... and the
// partial sums are then combined pairwise (ed25519_cosi_total_kernel: a block's lanes through LDS).
KYB_DEV void ed_cosi_total_partial(ge_p3& acc, const int4* tables, size_t m, int g, size_t first, size_t stride) {
    ge_p3_0(acc);
    const size_t nb = ed_cosi_groups(m, g);
#pragma unroll 1
    for (size_t b = first; b < nb; b += stride) {
        const TabGlobal t{const_cast<int4*>(tables) + (b << g) * ED_COSI_ENTRY_INT4};
        ge_cached c;
        ge_p1p1 r;
        t.get(c, (1 << ed_cosi_group_keys(m, g, b)) - 1);
        ge_add(r, acc, c);
        ge_p1p1_to_p3(acc, r);
    }
}
KYB_DEV void ed_cosi_total_combine(ge_p3& a, const ge_p3& b) {
    ge_cached c;
    ge_p1p1 r;
    ge_p3_to_cached(c, b);
    ge_add(r, a, c);
    ge_p1p1_to_p3(a, r);
}

// CountEnabled: the enabled keys of a mask of (m + 7) >> 3 bytes, read byte by byte; bits at or above m do not count
KYB_DEV uint32_t ed_cosi_mask_count(const uint8_t* __restrict__ mask, size_t m) {
    const size_t L = (m + 7) >> 3;
    uint32_t cnt = 0;
#pragma unroll 1
    for (size_t i = 0; i < L; i++) {
        uint32_t byte = mask[i];
        if (i == L - 1 && (m & 7)) byte &= (1u << (m & 7)) - 1u;
        cnt += (uint32_t)__builtin_popcount(byte);
    }
    return cnt;
}

// acc = the sum of the roster keys the mask enables; returns their number.  tall: T_all as one cached entry.  With
// 2 count > m the lane walks the complemented mask and returns T_all - acc: a full mask adds no table entry at all.
// The digit of a partial last group has its bits at or above m cleared in both polarities.
KYB_DEV uint32_t ed_cosi_aggregate_lane(ge_p3& acc, const uint8_t* __restrict__ mask, size_t m, int g,
                                        const int4* __restrict__ tables, const int4* __restrict__ tall) {
    const uint32_t count = ed_cosi_mask_count(mask, m);
    const bool flip = 2 * (size_t)count > m;
    const size_t nb = ed_cosi_groups(m, g);
    ge_p1p1 r;
    ge_cached c;
    ge_p3_0(acc);
#pragma unroll 1
    for (size_t b = 0; b < nb; b++) {
        uint32_t byte = mask[(b * (size_t)g) >> 3];
        if (flip) byte ^= 0xffu;
        uint32_t d = g == 8 ? byte : (byte >> (4 * (b & 1))) & 15u;
        d &= (1u << ed_cosi_group_keys(m, g, b)) - 1u;
#if defined(__HIP_DEVICE_COMPILE__)
        if (__ballot(d != 0) == 0) continue;  // no lane of the wave adds anything from this group
#endif
        const TabGlobal t{const_cast<int4*>(tables) + (b << g) * ED_COSI_ENTRY_INT4};
        t.get(c, (int)d);
        ge_add(r, acc, c);
        ge_p1p1_to_p3(acc, r);
    }
    if (flip) {
        ge_p3 neg;
        fe_neg(neg.X, acc.X);
        neg.Y = acc.Y;
        neg.Z = acc.Z;
        fe_neg(neg.T, acc.T);
        const TabGlobal t{const_cast<int4*>(tall)};
        t.get(c, 0);
        ge_add(r, neg, c);
        ge_p1p1_to_p3(acc, r);
    }
    return count;
}

// One cosignature (V || r) under the aggregate key A: T = (r mod l) B - k A with k = SHA-512(V as given || A's canonical
// bytes || msg) mod l (cosi.go:214-232).  r is reduced, not rejected; nothing is checked for canonicity or small order:
// the reference checks neither here.  -A comes from the parked (X, Y, Z) of the aggregation -- the encoder only reads
// it -- as (-X Z, Y Z, Z^2, -X Y): four multiplications instead of a second square root.  The verdict is
// encode(T) == canon(V) on bytes, taken by the caller.  wide: the standard base's comb; tab: room for one window table.
template <class Tab>
KYB_DEV void ed_cosi_check_lane(ge_p3& T, const uint32_t vw[8], const uint32_t rw[8], const uint32_t aw[8],
                                const int32_t* __restrict__ triple, const uint8_t* __restrict__ msg, size_t len,
                                const int32_t* __restrict__ wide, const sf::Mod& m, Tab& tab) {
    uint32_t kw[8], sw[8];
    ed_hram(kw, vw, aw, msg, len, m);  // first, as in ed_verify_lane: the hash's working set leaves before the point's comes
    {
        uint32_t x[16];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            x[i] = rw[i];
            x[8 + i] = 0;
        }
        sc_reduce512(sw, x, m);
    }
    ge_p3 nA;
    {
        fe X, Y, Z;
        load_fe(X, triple);
        load_fe(Y, triple + 10);
        load_fe(Z, triple + 20);
        fe_mul(nA.X, X, Z);
        fe_neg(nA.X, nA.X);
        fe_mul(nA.Y, Y, Z);
        fe_sq(nA.Z, Z);
        fe_mul(nA.T, X, Y);
        fe_neg(nA.T, nA.T);
    }
    int8_t e[65];
    recode16(e, kw, false);  // k < l: no digit is dropped
    ge_scalarmult_w4(T, e, nA, false, tab, 63);
    recode16(e, sw, false);  // r mod l
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
}

}  // namespace kyb
