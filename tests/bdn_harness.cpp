// kyber_amd/csrc/blake2xs.cuh and bdn.cuh compiled for the CPU over the three pairing suites (test infrastructure, never
// linked into libkyberhip.so): tests/test_bdn_host.py runs the roster, coefficient and term lanes and the masked sums at
// an explicit table width and slice count through these entry points against the oracle's table.  Memory is laid out
// as the kernels lay it out: the canonical roster, the decoded points, the subset tables built round by round, T_all and
// a mask's partial sums by the tree of 64 lanes.  Every buffer is a heap allocation of exactly the size the layout
// states, so that the sanitizer build (-DBDN_HARNESS_MAIN, tests/test_bdn_harness_sanitizers.py) sees a byte read or
// written past one.
#include "../kyber_amd/csrc/bls12381.cuh"
#include "../kyber_amd/csrc/bn254.cuh"
#include "../kyber_amd/csrc/bn256.cuh"
#include "../kyber_amd/csrc/bdn.cuh"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace kyb;

// the wave's tree of bdn_launch.cuh's bdn_tree_reduce, lane after lane
template <class F>
static void tree_reduce(Jac<F>* tree, unsigned live) {
    for (unsigned half = BDN_TREE / 2; half >= 1; half >>= 1)
        for (unsigned t = 0; t < half; t++)
            if (t + half < live) bdn_combine(tree[t], tree[t + half]);
}

template <class G>
static void terms(size_t m, const uint8_t* roster, uint8_t* coefs, uint8_t* out, uint8_t* status, uint32_t flags) {
    std::vector<uint8_t> canon(m * G::POINT);
    bool any = false;
    for (size_t j = 0; j < m; j++) {
        const int st = bdn_roster_lane<G>(canon.data() + G::POINT * j, roster + G::POINT * j, flags);
        if (status) status[j] = (uint8_t)st;
        any |= st != 0;
    }
    if (any) {
        if (coefs) memset(coefs, 0, 16 * m);
        memset(out, 0, G::POINT * m);
        return;
    }
    uint32_t h0[8];
    blake2xs_root(h0, canon.data(), m * G::POINT);
    std::vector<uint32_t> tab(G::TAB_WORDS ? G::TAB_WORDS : 1);
    for (size_t j = 0; j < m; j++) {
        uint32_t c[4];
        bdn_coef_lane(c, h0, j);
        if (coefs) bdn_coef_bytes(coefs + 16 * j, c);
        bdn_term_lane<G>(out + G::POINT * j, canon.data() + G::POINT * j, c, flags, tab.data());
    }
}

template <class G>
static void aggregate(size_t n, size_t m, int g, size_t S, const uint8_t* points, const uint8_t* masks, size_t stride, uint8_t* out,
                      uint32_t* count, uint8_t* status, uint32_t flags) {
    using J = Jac<typename G::F>;
    const size_t nb = bdn_groups(m, g), per = bdn_slice_groups(nb, S);
    std::vector<J> pts(m), tables(nb << g), tree(BDN_TREE), partial(S);
    uint32_t bad = 0;
    for (size_t j = 0; j < m; j++) {
        const int st = bdn_point_lane<G>(pts[j], points + G::POINT * j, flags);
        if (st && !bad) bad = (uint32_t)st;
    }
    for (size_t b = 0; b < nb; b++) {
        bdn_table_identity(tables.data(), g, b);
        for (int k = 0; k < g; k++)  // the rounds the block's barrier separates
            for (int s = 1 << k; s < 2 << k; s++) bdn_table_round(tables.data(), pts.data(), m, g, b, s, k);
    }
    for (size_t t = 0; t < (size_t)BDN_TREE; t++) bdn_total_partial(tree[t], tables.data(), m, g, t, BDN_TREE);
    tree_reduce(tree.data(), BDN_TREE);
    const J tall = tree[0];
    for (size_t i = 0; i < n; i++) {
        const uint8_t* mask = masks + i * stride;
        const uint32_t cnt = bdn_mask_count(mask, m);
        const bool flip = bdn_mask_flips(cnt, m);
        for (size_t s = 0; s < S; s++) {
            const size_t lo = s * per < nb ? s * per : nb, hi = lo + per < nb ? lo + per : nb;
            bdn_slice_lane(partial[s], mask, m, g, flip, tables.data(), lo, hi);
        }
        if (S > 1) {  // bdn_fold_kernel
            const unsigned live = S < (size_t)BDN_TREE ? (unsigned)S : (unsigned)BDN_TREE;
            for (unsigned t = 0; t < live; t++)
                for (size_t s = (size_t)t + BDN_TREE; s < S; s += BDN_TREE) bdn_combine(partial[t], partial[s]);
            tree_reduce(partial.data(), live);
        }
        if (count) count[i] = cnt;
        if (status) status[i] = (uint8_t)bad;
        if (bad) memset(out + G::POINT * i, 0, G::POINT);
        else bdn_finish_lane<G>(out + G::POINT * i, partial[0], flip, tall);
    }
}

extern "C" {
// which: 0 / 1 = BLS12-381 G1 / G2, 2 / 3 = bn256, 4 / 5 = bn254
int bdh_point_len(int which) {
    const size_t len[6] = {bls::G1::POINT, bls::G2::POINT, bn::G1::POINT, bn::G2::POINT, bn4::G1::POINT, bn4::G2::POINT};
    return which >= 0 && which < 6 ? (int)len[which] : -1;
}
void bdh_plan(size_t n, size_t m, int* plan) {
    plan[0] = bdn_group_width(n, m);
    plan[1] = (int)bdn_slices(n, m, plan[0]);
}
size_t bdh_additions(size_t n, size_t m, int g) { return bdn_additions(n, m, g); }
// ncoef coefficients of 16 bytes over `len` message bytes
void bdh_blake2xs(const uint8_t* data, size_t len, size_t ncoef, uint8_t* out) {
    uint32_t h0[8];
    blake2xs_root(h0, data, len);
    for (size_t j = 0; j < ncoef; j++) {
        uint32_t c[4];
        bdn_coef_lane(c, h0, j);
        bdn_coef_bytes(out + 16 * j, c);
    }
}
// kyb_<suite>_bdn_terms_<g>'s value.  coefs, status: each may be NULL.
void bdh_terms(int which, size_t m, const uint8_t* roster, uint8_t* coefs, uint8_t* out, uint8_t* status, uint32_t flags) {
    switch (which) {
        case 0: return terms<bls::G1>(m, roster, coefs, out, status, flags);
        case 1: return terms<bls::G2>(m, roster, coefs, out, status, flags);
        case 2: return terms<bn::G1>(m, roster, coefs, out, status, flags);
        case 3: return terms<bn::G2>(m, roster, coefs, out, status, flags);
        case 4: return terms<bn4::G1>(m, roster, coefs, out, status, flags);
        default: return terms<bn4::G2>(m, roster, coefs, out, status, flags);
    }
}
// kyb_<suite>_mask_aggregate_<g>'s value at table width g and S slices.  count, status: each may be NULL.
void bdh_aggregate(int which, size_t n, size_t m, int g, size_t S, const uint8_t* points, const uint8_t* masks, size_t stride, uint8_t* out,
                   uint32_t* count, uint8_t* status, uint32_t flags) {
    switch (which) {
        case 0: return aggregate<bls::G1>(n, m, g, S, points, masks, stride, out, count, status, flags);
        case 1: return aggregate<bls::G2>(n, m, g, S, points, masks, stride, out, count, status, flags);
        case 2: return aggregate<bn::G1>(n, m, g, S, points, masks, stride, out, count, status, flags);
        case 3: return aggregate<bn::G2>(n, m, g, S, points, masks, stride, out, count, status, flags);
        case 4: return aggregate<bn4::G1>(n, m, g, S, points, masks, stride, out, count, status, flags);
        default: return aggregate<bn4::G2>(n, m, g, S, points, masks, stride, out, count, status, flags);
    }
}
}

#ifdef BDN_HARNESS_MAIN
// Rosters at every group edge of both widths, every slice count from 1 to the number of groups, masks of both polarities
// with stray bits, at the exact stride and at an odd one, hashes at the block edges, all over exactly sized buffers.  The
// roster is the generator's encoding with the identity's and a rejected key's among its copies: equal points, the identity
// and the status path.  Values are checked by tests/test_bdn_host.py: this program is for the sanitizers.
static uint8_t* filled(size_t bytes, uint32_t& seed) {
    uint8_t* p = new uint8_t[bytes ? bytes : 1];
    for (size_t i = 0; i < bytes; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
template <class G>
static void run(int which, uint32_t& seed) {
    Aff<typename G::F> gen;
    G::generator(gen);
    uint8_t base[G::POINT], zero[G::POINT];
    G::encode(base, gen, 0);
    gen.inf = true;
    G::encode(zero, gen, 0);
    const size_t ms[] = {1, 3, 4, 5, 8, 9, 17}, n = 5;
    for (size_t m : ms)
        for (int bad = 0; bad < 2; bad++) {
            uint8_t* roster = new uint8_t[G::POINT * m];
            for (size_t j = 0; j < m; j++) memcpy(roster + G::POINT * j, j % 3 == 2 ? zero : base, G::POINT);
            if (bad) memset(roster + G::POINT * (m - 1), 0xff, G::POINT);
            uint8_t *coefs = new uint8_t[16 * m], *tm = new uint8_t[G::POINT * m], *st = new uint8_t[m > n ? m : n];
            bdh_terms(which, m, roster, coefs, tm, st, 0);
            bdh_terms(which, m, roster, nullptr, tm, nullptr, 0x100);
            for (int g = 4; g <= 8; g += 4)
                for (size_t slack = 0; slack <= 3; slack += 3) {
                    const size_t L = (m + 7) >> 3, stride = L + slack, nb = bdn_groups(m, g);
                    uint8_t* masks = filled((n - 1) * stride + L, seed);  // the last mask ends the buffer
                    memset(masks, 0xff, L);                                // full, stray bits included
                    memset(masks + stride, 0, L);                          // empty
                    uint8_t* out = new uint8_t[G::POINT * n];
                    uint32_t* cnt = new uint32_t[n];
                    for (size_t S = 1; S <= nb; S++) {
                        bdh_aggregate(which, n, m, g, S, bad ? roster : tm, masks, stride, out, cnt, st, 0);
                        bdh_aggregate(which, n, m, g, S, bad ? roster : tm, masks, stride, out, nullptr, nullptr, 0x100);
                    }
                    delete[] masks; delete[] out; delete[] cnt;
                }
            delete[] roster; delete[] coefs; delete[] tm; delete[] st;
        }
}
int main() {
    uint32_t seed = 11;
    const size_t lens[] = {0, 63, 64, 65, 128, 200};
    for (size_t len : lens) {
        uint8_t* msg = filled(len, seed);
        uint8_t* out = new uint8_t[16 * 5];
        bdh_blake2xs(msg, len, 5, out);
        delete[] msg; delete[] out;
    }
    run<bls::G1>(0, seed);
    run<bls::G2>(1, seed);
    run<bn::G1>(2, seed);
    run<bn::G2>(3, seed);
    run<bn4::G1>(4, seed);
    run<bn4::G2>(5, seed);
    puts("ok");
    return 0;
}
#endif
