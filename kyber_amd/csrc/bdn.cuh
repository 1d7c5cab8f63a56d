// sign/bdn on the pairing suites, one element per lane: NewMask's coefficients and terms over a roster, and the sum of
// the terms a participation mask enables.  Written once over a group policy G (the G1 / G2 structs at the end of
// bls12381.cuh and bn_suite.inc).
//
// Replaces, in the reference:
//   hashPointToR              bdn.go:29-63     -> bdn_roster_lane (MarshalBinary's bytes), blake2xs_root, bdn_coef_lane
//   NewMask publicTerms       mask.go:57-61    -> bdn_term_lane ((c + 1) P in one ladder)
//   AggregatePublicKeys       bdn.go:166-181   -> bdn_point_lane, bdn_table_round, bdn_total_partial, bdn_slice_lane,
//                                                 bdn_combine, bdn_finish_lane
// The aggregation is ed25519_cosi.cuh's scheme on a generic group: the m points are cut into groups of g = 4 or 8, group
// b's table holds the 2^g sums of its subsets as Jacobian points, entry 0 the identity, built in g rounds of one addition
// per entry; a lane adds one entry per group, picked by the mask's nibble or byte, and a mask with more than half of its
// bits set is walked through its complement and finished as T_all - acc.  The additions are curve.cuh's jac_add, which
// handles either operand at infinity, P = Q and P = -Q: a roster may hold equal points, opposite points and the
// identity.  New against the Ed25519 unit are the SLICES: with few masks one lane per mask is a chain of `groups`
// additions on an idle device, so a lane takes (mask, slice of the groups) and a tree pass sums a mask's S partial sums.
// Addresses follow the mask, which is public data in every caller.
// Compiles with g++ too (tests/bdn_harness.cpp runs these lane programs on the CPU against the oracle).
#pragma once
#include "blake2xs.cuh"
#include "curve.cuh"

namespace kyb {

constexpr size_t BDN_MAX_ROSTER = 8192;  // KYB_COSI_MAX_ROSTER of include/kyber_hip.h
// Lanes that fill the device once: one wave on every SIMD of 256 compute units
constexpr size_t BDN_FILL = 256 * 4 * 64;
constexpr size_t BDN_PIECE = 65536;  // masks per launch: the partial sums of one piece are what the workspace holds
constexpr int BDN_TREE = 64;         // lanes of the tree that sums partial sums (one wave)

// ---- the plan: ed_cosi_additions' count decides the width, BDN_FILL the slices
KYB_HD size_t bdn_additions(size_t n, size_t m, int g) {
    const size_t full = m / (size_t)g, rem = m % (size_t)g, nb = full + (rem ? 1 : 0);
    return full * (((size_t)1 << g) - (size_t)g - 1) + (rem ? ((size_t)1 << rem) - rem - 1 : 0) + nb + n * nb;
}
KYB_HD int bdn_group_width(size_t n, size_t m) { return bdn_additions(n, m, 8) < bdn_additions(n, m, 4) ? 8 : 4; }
KYB_HD size_t bdn_groups(size_t m, int g) { return (m + (size_t)g - 1) / (size_t)g; }
KYB_HD int bdn_group_keys(size_t m, int g, size_t b) {
    const size_t left = m - b * (size_t)g;
    return left < (size_t)g ? (int)left : g;
}
// S = min(groups, ceil(BDN_FILL / n)): 1 from n = BDN_FILL on
KYB_HD size_t bdn_slices(size_t n, size_t m, int g) {
    const size_t nb = bdn_groups(m, g), want = (BDN_FILL + n - 1) / n;
    return nb < want ? nb : want;
}
// groups of one slice: slice s takes [s * per, (s + 1) * per), cut at nb; the last slices may be empty
KYB_HD size_t bdn_slice_groups(size_t nb, size_t S) { return (nb + S - 1) / S; }

// ---- NewMask
// Key j by the suite's UnmarshalBinary rules: canon = MarshalBinary's bytes of the decoded point (zero where rejected),
// the bytes the hash takes; returns the status.
template <class G>
KYB_HD int bdn_roster_lane(uint8_t* __restrict__ canon, const uint8_t* __restrict__ in, uint32_t flags) {
    return G::unmarshal_wire(canon, in, flags);
}
// c = coefficient j as four little-endian words: stream bytes 16 j .. 16 j + 15, half of output node j >> 1
KYB_HD void bdn_coef_lane(uint32_t (&c)[4], const uint32_t (&h0)[8], size_t j) {
    uint32_t o[8];
    blake2xs_node(o, h0, (uint32_t)(j >> 1));
    const bool hi = (j & 1) != 0;
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = hi ? o[4 + i] : o[i];
}
KYB_HD void bdn_coef_bytes(uint8_t* __restrict__ out, const uint32_t (&c)[4]) {
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = (uint8_t)(c[i >> 2] >> (8 * (i & 3)));
}
// k = c + 1 <= 2^128 as the 32 big-endian bytes the ladders take
KYB_HD void bdn_scalar_be(uint8_t (&k)[32], const uint32_t (&c)[4]) {
    uint32_t w[5];
    uint64_t carry = 1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        carry += c[i];
        w[i] = (uint32_t)carry;
        carry >>= 32;
    }
    w[4] = (uint32_t)carry;
#pragma unroll
    for (int i = 0; i < 32; i++) k[i] = 0;
#pragma unroll
    for (int i = 0; i < 20; i++) k[31 - i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}
// term = (c + 1) P from P's canonical bytes, by the group's standing ladder: the value of Mul(c, P) then Add(., P), the
// identity for the identity.  The roster lane ran UnmarshalBinary's checks, so where those prove membership the ladder
// takes the point as vouched for.  tab: this lane's table slab (G::TAB_WORDS words; nullptr where the group has none).
template <class G>
KYB_HD int bdn_term_lane(uint8_t* __restrict__ term, const uint8_t* __restrict__ canon, const uint32_t (&c)[4], uint32_t flags,
                         uint32_t* __restrict__ tab) {
    uint8_t k[32];
    bdn_scalar_be(k, c);
    return G::mul_wire(term, k, canon, G::decode_proves_subgroup() ? (flags | FLAG_TRUSTED0) : flags, tab);
}

// ---- the masked sums
// Point j decoded into the workspace; the status of UnmarshalBinary (the identity is parked where it is not 0)
template <class G>
KYB_HD int bdn_point_lane(Jac<typename G::F>& p, const uint8_t* __restrict__ in, uint32_t flags) {
    Aff<typename G::F> a;
    const int st = G::decode(a, in, flags);
    if (st != 0) jac_set_inf(p);
    else jac_from_aff(p, a);
    return st;
}
// Round k of group b's table, for the subset s whose highest point is k (s >> k == 1): entry[s] = entry[s without k] +
// point k.  Entry 0 is written before round 0; round k reads entries of rounds below k only.  A point at or above m (the
// last group may be partial) adds nothing: its entries are copies, and no lane reads them.
template <class F>
KYB_HD void bdn_table_round(Jac<F>* tables, const Jac<F>* pts, size_t m, int g, size_t b, int s, int k) {
    Jac<F>* t = tables + (b << g);
    const size_t j = b * (size_t)g + (size_t)k;
    const int parent = s ^ (1 << k);
    if (j >= m) {
        t[s] = t[parent];
        return;
    }
    if (parent == 0) {
        t[s] = pts[j];
        return;
    }
    Jac<F> a = t[parent], p = pts[j], r;
    jac_add(r, a, p);
    t[s] = r;
}
template <class F>
KYB_HD void bdn_table_identity(Jac<F>* tables, int g, size_t b) {
    Jac<F> o;
    jac_set_inf(o);
    tables[b << g] = o;
}
// T_all = the sum of every group's full entry: a lane sums the groups first, first + stride, ...; bdn_combine joins them
template <class F>
KYB_HD void bdn_total_partial(Jac<F>& acc, const Jac<F>* tables, size_t m, int g, size_t first, size_t stride) {
    jac_set_inf(acc);
    const size_t nb = bdn_groups(m, g);
#pragma unroll 1
    for (size_t b = first; b < nb; b += stride) {
        Jac<F> e = tables[(b << g) + (((size_t)1 << bdn_group_keys(m, g, b)) - 1)], r;
        jac_add(r, acc, e);
        acc = r;
    }
}
template <class F>
KYB_HD void bdn_combine(Jac<F>& a, const Jac<F>& b) {
    Jac<F> r;
    jac_add(r, a, b);
    a = r;
}
// The enabled points of a mask of (m + 7) >> 3 bytes, read byte by byte; bits at or above m do not count
KYB_HD uint32_t bdn_mask_count(const uint8_t* __restrict__ mask, size_t m) {
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
KYB_HD bool bdn_mask_flips(uint32_t count, size_t m) { return 2 * (size_t)count > m; }
// acc = the sum over groups [lo, hi) of the entry the mask (complemented if flip) picks.  The digit of a partial last
// group has its bits at or above m cleared in both polarities; digit 0 adds nothing and is skipped.
template <class F>
KYB_HD void bdn_slice_lane(Jac<F>& acc, const uint8_t* __restrict__ mask, size_t m, int g, bool flip, const Jac<F>* tables, size_t lo,
                           size_t hi) {
    jac_set_inf(acc);
#pragma unroll 1
    for (size_t b = lo; b < hi; b++) {
        uint32_t byte = mask[(b * (size_t)g) >> 3];
        if (flip) byte ^= 0xffu;
        uint32_t d = g == 8 ? byte : (byte >> (4 * (b & 1))) & 15u;
        d &= (1u << bdn_group_keys(m, g, b)) - 1u;
        if (d == 0) continue;
        Jac<F> e = tables[(b << g) + d], r;
        jac_add(r, acc, e);
        acc = r;
    }
}
// out = MarshalBinary of the mask's sum: acc, or T_all - acc for a mask walked through its complement
template <class G>
KYB_HD void bdn_finish_lane(uint8_t* __restrict__ out, const Jac<typename G::F>& acc, bool flip, const Jac<typename G::F>& tall) {
    Jac<typename G::F> r = acc;
    if (flip) {
        Jac<typename G::F> neg;
        jac_neg(neg, acc);
        jac_add(r, tall, neg);
    }
    Aff<typename G::F> a;
    jac_to_aff(a, r);
    G::encode(out, a, 0);
}

}  // namespace kyb
