// kyber_amd/csrc/ed25519_dss.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_dss_host.py runs the two calls -- the partial-signature check and PartialSig for a batch of sessions --
// through these entry points against the oracle (tests/_dss_oracle.py) on the labelled cases of tests/_dss_cases.py.
// The entry points take the arguments of the C ABI's host calls and walk memory as the kernels do: a session pass (the
// hashes), a fold pass over (session, coefficient) lanes with a lane's window table in a nine-limb slab, the folded
// commitments through their encodings into mixed-addition operands, then the three passes of a partial signature.  With
// -DDSS_HARNESS_MAIN the file is a stand-alone program over the same entry points, for a sanitizer build
// (tests/test_dss_harness_sanitizers.py).
#include "../kyber_amd/csrc/ed25519_dss.cuh"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace kyb;

static void words(uint32_t w[8], const uint8_t* p) { memcpy(w, p, 32); }  // little-endian host

static const sf::Mod& order() {
    static const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    return m;
}

// the rows of the standard base's wide comb that a scalar reads, built on demand with the device's row code
static int32_t* g_wide = nullptr;
static std::vector<bool> g_have;
static void need_comb_rows(const uint32_t sw[8]) {
    if (!g_wide) {
        g_wide = (int32_t*)calloc(ED_WIDE_WORDS, sizeof(int32_t));
        g_have.assign(EdWide::ROWS, false);
    }
    ge_p3 B;
    B.X = fe_bx(); B.Y = fe_by(); fe_1(B.Z); B.T = fe_bt();
    int8_t e[65];
    recode16(e, sw, false);
    for (int k = 0; k < EdWide::POS_CT; k++) {
        int d = 0;
        for (int i = ED_COMB_G - 1; i >= 0; i--)
            if (ED_COMB_G * k + i < 64) d = 16 * d + (int)e[ED_COMB_G * k + i];
        if (d == 0) continue;
        const int t = k * EdWide::ENT + (d < 0 ? -d : d) - 1;
        if (g_have[t]) continue;
        ed_comb_row<ED_COMB_G>(g_wide + (size_t)t * ED_TAB_STRIDE, t, B);
        g_have[t] = true;
    }
}

// exactly sized copies of the word arrays the kernels read in place: a word read past one is the sanitizer's to report
static std::vector<uint32_t> word_copy(const uint8_t* p, size_t bytes) {
    std::vector<uint32_t> w(bytes / 4);
    memcpy(w.data(), p, bytes);
    return w;
}

static int args_bad(size_t n, size_t tl, size_t tr, size_t ns, std::initializer_list<const void*> ptrs) {
    if (!n) return 0;
    for (const void* p : ptrs)
        if (!p) return 1;
    return tl == 0 || tr == 0 || ns == 0;
}

extern "C" {

void dsh_session_id(size_t tl, const uint8_t* lc, size_t tr, const uint8_t* rc, uint8_t* out) {
    const std::vector<uint32_t> l = word_copy(lc, 32 * tl), r = word_copy(rc, 32 * tr);
    uint32_t sid[8];
    ed_dss_session_id(sid, l.data(), tl, r.data(), tr);
    memcpy(out, sid, 32);
}
void dsh_partial_hash(const uint8_t* v, uint32_t index, const uint8_t* sid, uint8_t* out) {
    uint32_t vw[8], sw[8], mw[8];
    words(vw, v);
    words(sw, sid);
    ed_dss_partial_hash(mw, vw, index, sw);
    memcpy(out, mw, 32);
}
// h_b of every session, 32 bytes each (the scalar, little-endian)
void dsh_hash_sig(size_t ns, size_t tl, const uint8_t* lc, size_t tr, const uint8_t* rc, const uint8_t* msgs, const uint64_t* off,
                  uint8_t* out) {
    const std::vector<uint32_t> l = word_copy(lc, 32 * tl), r = word_copy(rc, 32 * tr * ns);
    for (size_t b = 0; b < ns; b++) {
        uint32_t hw[8], sid[8];
        ed_dss_session_lane(hw, sid, l.data(), tl, r.data() + b * tr * 8, tr, msgs + off[b], (size_t)element_len(off, b), order());
        memcpy(out + 32 * b, hw, 32);
    }
}

// kyb_ed25519_dss_check's value and return code; a partial that names no session of the call gives ok = 0, status 0 (the
// _dev rule).  folded (may be NULL): ns x max(tl, tr) x 32 bytes, the encodings of the folded commitments.
int dsh_dss_check(size_t n, size_t np, const uint8_t* participants, size_t tl, const uint8_t* long_commits, size_t ns, size_t tr,
                  const uint8_t* rand_commits, const uint8_t* msgs, const uint64_t* off, const uint32_t* sess, const uint32_t* idx,
                  const uint8_t* V, const uint8_t* sid, const uint8_t* sigs, uint8_t* ok, uint8_t* status, uint8_t* sess_status,
                  uint8_t* folded) {
    if (args_bad(n, tl, tr, ns, {participants, long_commits, rand_commits, off, sess, idx, V, sid, sigs, ok})) return -1;
    if (n == 0) return 0;
    for (size_t b = 0; b < ns; b++)
        if (off[b + 1] < off[b]) return -1;
    const size_t T = tl > tr ? tl : tr;
    const std::vector<uint32_t> lc = word_copy(long_commits, 32 * tl), rc = word_copy(rand_commits, 32 * tr * ns);
    std::vector<uint32_t> hs(8 * ns), sids(8 * ns);
    std::vector<uint8_t> bad(ns, 0);
    std::vector<ge_precomp> aff(ns * T);
    std::vector<int4> slab(80);
    if (sess_status) memset(sess_status, 0, ns);
    for (size_t b = 0; b < ns; b++) {  // the session pass
        uint32_t hw[8], sw[8];
        ed_dss_session_lane(hw, sw, lc.data(), tl, rc.data() + b * tr * 8, tr, msgs + off[b], (size_t)element_len(off, b), order());
        memcpy(hs.data() + 8 * b, hw, 32);
        memcpy(sids.data() + 8 * b, sw, 32);
    }
    for (size_t i = 0; i < ns * T; i++) {  // the fold pass and its encoder
        const size_t b = i / T, k = i % T;
        uint32_t rw[8] = {1, 0, 0, 0, 0, 0, 0, 0}, aw[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        if (k < tr) memcpy(rw, rc.data() + (b * tr + k) * 8, 32);
        if (k < tl) memcpy(aw, lc.data() + k * 8, 32);
        DssTab tab{slab.data()};
        ge29_p3 D;
        if (!ed_dss_fold_lane(D, hs.data() + 8 * b, rw, aw, tab)) {
            bad[b] = 1;
            if (sess_status) sess_status[b] = ED_ST_BAD_POINT;
        }
        int32_t proj[30];
        store_proj(proj, 0, D);  // parked as ten limbs, read back as the encoder reads it
        ge_p3 P;
        load_fe(P.X, proj);
        load_fe(P.Y, proj + 10);
        load_fe(P.Z, proj + 20);
        uint32_t w[8];
        ge_p3_towords(w, P);
        if (folded) memcpy(folded + 32 * i, w, 32);
        ed_deal_decode(aff[i], w);
    }
    for (size_t i = 0; i < n; i++) {  // the three passes of a partial signature
        if (sess[i] >= ns) {
            ok[i] = 0;
            if (status) status[i] = 0;
            continue;
        }
        int st;
        if (idx[i] >= np) {
            st = ED_ST_DSS_INDEX;
        } else {
            uint32_t vw[8], sw[8], mw[8], aw[8], rw[8], Sw[8];
            words(vw, V + 32 * i);
            words(sw, sid + 32 * i);
            ed_dss_partial_hash(mw, vw, idx[i], sw);
            words(aw, participants + 32 * (size_t)idx[i]);
            words(rw, sigs + 64 * i);
            words(Sw, sigs + 64 * i + 32);
            need_comb_rows(Sw);
            DssTab tab{slab.data()};
            ge_p3 Tp;
            st = ed_dss_verify_lane(Tp, rw, Sw, aw, mw, g_wide, order(), tab);
            uint32_t w[8];
            ge_p3_towords(w, Tp);
            if (st == ED_ST_OK && memcmp(w, rw, 32) != 0) st = ED_ST_DSS_SIG;
            if (st == ED_ST_OK) {
                const size_t b = sess[i];
                need_comb_rows(vw);
                st = ed_dss_share_element(st, sw, sids.data() + 8 * b, bad[b] != 0, vw, aff.data() + b * T, T, idx[i], g_wide);
            }
        }
        ok[i] = st == ED_ST_OK ? 1 : 0;
        if (status) status[i] = (uint8_t)st;
    }
    return 0;
}

// kyb_ed25519_dss_partial's value and return code
int dsh_dss_partial(size_t ns, const uint8_t* priv, uint32_t index, const uint8_t* alpha, const uint8_t* beta, const uint8_t* k, size_t tl,
                    const uint8_t* long_commits, size_t tr, const uint8_t* rand_commits, const uint8_t* msgs, const uint64_t* off, uint8_t* V,
                    uint8_t* sid, uint8_t* sigs) {
    if (args_bad(ns, tl, tr, 1, {priv, alpha, beta, k, long_commits, rand_commits, off, V, sid, sigs})) return -1;
    if (ns == 0) return 0;
    for (size_t b = 0; b < ns; b++)
        if (off[b + 1] < off[b]) return -1;
    const std::vector<uint32_t> lc = word_copy(long_commits, 32 * tl), rc = word_copy(rand_commits, 32 * tr * ns);
    uint32_t xw[8], alw[8], Aw[8];
    words(xw, priv);
    words(alw, alpha);
    {
        need_comb_rows(xw);
        int8_t e[65];
        recode16(e, xw, false);
        ge_p3 A;
        ed_comb_mul_base(A, e, g_wide);
        ge_p3_towords(Aw, A);
    }
    for (size_t b = 0; b < ns; b++) {
        uint32_t hw[8], sw[8], bw[8], kw[8], vw[8], mw[8], rw[8], sig[16];
        ed_dss_session_lane(hw, sw, lc.data(), tl, rc.data() + b * tr * 8, tr, msgs + off[b], (size_t)element_len(off, b), order());
        words(bw, beta + 32 * b);
        words(kw, k + 32 * b);
        ed_dss_partial_value(vw, mw, hw, alw, bw, index, sw, order());
        need_comb_rows(kw);
        int8_t e[65];
        recode16(e, kw, false);
        ge_p3 R;
        ed_comb_mul_base(R, e, g_wide);
        ge_p3_towords(rw, R);
        ed_dss_partial_sign(sig, rw, Aw, kw, xw, mw, order());
        memcpy(V + 32 * b, vw, 32);
        memcpy(sid + 32 * b, sw, 32);
        memcpy(sigs + 64 * b, sig, 64);
    }
    return 0;
}
}

#ifdef DSS_HARNESS_MAIN
// Both entries over exactly sized heap buffers: an odd byte offset stands in front of the first message and the last
// message ends its buffer.  Values are checked by tests/test_dss_host.py; this program is for the sanitizers, and checks
// only that what it signed passes its own check and that planted rejects are rejected.
static uint8_t* filled(size_t bytes, uint32_t& seed) {
    uint8_t* p = new uint8_t[bytes ? bytes : 1];
    for (size_t i = 0; i < bytes; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
static void base_mul(uint8_t* out, const uint8_t* scalar) {
    uint32_t sw[8], w[8];
    words(sw, scalar);
    need_comb_rows(sw);
    int8_t e[65];
    recode16(e, sw, false);
    ge_p3 P;
    ed_comb_mul_base(P, e, g_wide);
    ge_p3_towords(w, P);
    memcpy(out, w, 32);
}
int main() {
    static const size_t LENGTHS[] = {0, 47, 48, 63, 64, 111, 112};
    const size_t ns = sizeof(LENGTHS) / sizeof(LENGTHS[0]), np = 3;
    uint32_t seed = 29;
    int bad = 0;
    for (size_t shape = 0; shape < 4; shape++) {  // (tl, tr): equal, longer long-term, longer random, one each
        const size_t tl = shape == 1 ? 3 : (shape == 3 ? 1 : 2), tr = shape == 2 ? 3 : (shape == 3 ? 1 : 2);
        uint64_t off[ns + 1];
        off[0] = 3;  // an odd byte offset in front of the first message, which is empty
        for (size_t i = 0; i < ns; i++) off[i + 1] = off[i] + LENGTHS[i];
        uint8_t* msgs = filled((size_t)off[ns], seed);
        uint8_t *privs = filled(32 * np, seed), *alpha = filled(32, seed), *beta = filled(32 * ns, seed), *k = filled(32 * ns, seed);
        for (size_t i = 0; i < np; i++) privs[32 * i + 31] &= 0x0f;  // below l: S = k + h x is then what verifies
        for (size_t i = 0; i < ns; i++) k[32 * i + 31] &= 0x7f;      // below 2^255: k B is then (k mod l) B
        uint8_t* seeds = filled(32 * (tl + ns * tr), seed);
        uint8_t *parts = new uint8_t[32 * np], *lc = new uint8_t[32 * tl], *rc = new uint8_t[32 * ns * tr];
        for (size_t i = 0; i < np; i++) base_mul(parts + 32 * i, privs + 32 * i);
        for (size_t i = 0; i < tl; i++) base_mul(lc + 32 * i, seeds + 32 * i);
        for (size_t i = 0; i < ns * tr; i++) base_mul(rc + 32 * i, seeds + 32 * (tl + i));
        uint8_t *V = new uint8_t[32 * ns], *sid = new uint8_t[32 * ns], *sigs = new uint8_t[64 * ns];
        bad |= dsh_dss_partial(ns, privs + 32, 1, alpha, beta, k, tl, lc, tr, rc, msgs, off, V, sid, sigs);
        uint32_t *sess = new uint32_t[ns + 2], *idx = new uint32_t[ns + 2];
        uint8_t *ok = new uint8_t[ns + 2], *st = new uint8_t[ns + 2], *sst = new uint8_t[ns];
        uint8_t *V2 = new uint8_t[32 * (ns + 2)], *sid2 = new uint8_t[32 * (ns + 2)], *sigs2 = new uint8_t[64 * (ns + 2)];
        memcpy(V2, V, 32 * ns); memcpy(sid2, sid, 32 * ns); memcpy(sigs2, sigs, 64 * ns);
        memcpy(V2 + 32 * ns, V, 64); memcpy(sid2 + 32 * ns, sid, 64); memcpy(sigs2 + 64 * ns, sigs, 128);
        for (size_t i = 0; i < ns; i++) { sess[i] = (uint32_t)i; idx[i] = 1; }
        sess[ns] = 0; idx[ns] = (uint32_t)np;           // an index outside the roster
        sess[ns + 1] = (uint32_t)ns; idx[ns + 1] = 1;   // a session outside the call
        bad |= dsh_dss_check(ns + 2, np, parts, tl, lc, ns, tr, rc, msgs, off, sess, idx, V2, sid2, sigs2, ok, st, sst, nullptr);
        bad |= dsh_dss_check(ns + 2, np, parts, tl, lc, ns, tr, rc, msgs, off, sess, idx, V2, sid2, sigs2, ok, nullptr, nullptr, nullptr);
        // the signatures hold and the session ids match; V is no share of these commitments (they are unrelated points)
        for (size_t i = 0; i < ns; i++) bad |= st[i] != ED_ST_DSS_PARTIAL;
        bad |= st[ns] != ED_ST_DSS_INDEX || ok[ns + 1] != 0;
        delete[] msgs; delete[] privs; delete[] alpha; delete[] beta; delete[] k; delete[] seeds; delete[] parts; delete[] lc; delete[] rc;
        delete[] V; delete[] sid; delete[] sigs; delete[] sess; delete[] idx; delete[] ok; delete[] st; delete[] sst;
        delete[] V2; delete[] sid2; delete[] sigs2;
    }
    free(g_wide);
    puts(bad ? "FAILED" : "ok");
    return bad;
}
#endif
