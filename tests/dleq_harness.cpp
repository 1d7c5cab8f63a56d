// kyber_amd/csrc/blake2xb.cuh and ed25519_dleq.cuh compiled for the CPU (test infrastructure, never linked into
// libkyberhip.so): tests/test_dleq_host.py runs the compression, the bounded pick, the canonical-bytes rule, the
// challenge and the two-sided verify program through these entry points against hashlib, the Python XOF and the
// big-integer oracle.  Window tables live in a TabGlobal slab and the points are parked and encoded as in the kernels.
#include "../kyber_amd/csrc/ed25519_dleq.cuh"

#include <string.h>

#include <vector>

using namespace kyb;

static void words(uint32_t w[8], const uint8_t* p) { memcpy(w, p, 32); }  // little-endian host

extern "C" {
// out = BLAKE2b-512(key, msg): RFC 7693's sequential mode, every block through blake2b_compress_regs
void dlq_blake2b(const uint8_t* key, size_t keylen, const uint8_t* msg, size_t len, uint8_t* out) {
    std::vector<uint8_t> data;
    if (keylen) {
        data.assign(128, 0);
        memcpy(data.data(), key, keylen);
    }
    data.insert(data.end(), msg, msg + len);
    const size_t total = data.size();
    const size_t blocks = total ? (total + 127) / 128 : 1;
    data.resize(blocks * 128, 0);
    uint64_t h[8] = KYB_BLAKE2B_IV;
    h[0] ^= 0x01010000ull | ((uint64_t)keylen << 8) | 64;
    for (size_t b = 0; b < blocks; b++) {
        uint64_t m[16];
        memcpy(m, data.data() + 128 * b, 128);
        const bool last = b + 1 == blocks;
        blake2b_compress_regs(h, m, last ? total : 128 * (b + 1), last);
    }
    memcpy(out, h, 64);
}
// c = Pick(blake2xb.New(seed)) for a 32-byte seed; returns the draws taken (0: exhausted)
int dlq_pick(const uint8_t* seed, uint8_t* c) {
    uint32_t cb[8], cw[8];
    words(cb, seed);
    const int draws = ed_scalar_pick(cw, cb);
    memcpy(c, cw, 32);
    return draws;
}
void dlq_canon(const uint8_t* enc, uint8_t* out) {
    uint32_t w[8], o[8];
    words(w, enc);
    ed_canon_point_bytes(o, w);
    memcpy(out, o, 32);
}
int dlq_challenge(const uint8_t* xG, const uint8_t* xH, const uint8_t* vG, const uint8_t* vH, uint8_t* c) {
    uint32_t a[8], b[8], u[8], v[8], cw[8];
    words(a, xG);
    words(b, xH);
    words(u, vG);
    words(v, vH);
    const int draws = ed_dleq_challenge(cw, a, b, u, v);
    memcpy(c, cw, 32);
    return draws;
}
// the verify kernel's lane program + the encode pass's verdict, element by element.  gs, hs: 32 or 0 (a shared base);
// expect: NULL or one scalar; fs, full: KYB_F_DLEQ_FS, KYB_F_VARTIME
void dlq_verify(size_t n, const uint8_t* G, size_t gs, const uint8_t* H, size_t hs, const uint8_t* xG, const uint8_t* xH,
                const uint8_t* C, const uint8_t* R, const uint8_t* VG, const uint8_t* VH, const uint8_t* expect, int fs,
                int full, uint8_t* ok, uint8_t* status) {
    std::vector<int4> slab(160);
    std::vector<uint32_t> ex(8);
    if (expect) memcpy(ex.data(), expect, 32);
    for (size_t i = 0; i < n; i++) {
        uint32_t cw[8], rw[8], a[8], b[8], u[8], v[8];
        words(cw, C + 32 * i);
        words(rw, R + 32 * i);
        words(a, xG + 32 * i);
        words(b, xH + 32 * i);
        words(u, VG + 32 * i);
        words(v, VH + 32 * i);
        int st = ed_dleq_challenge_status(cw, expect ? ex.data() : nullptr, fs != 0, a, b, u, v);
        TabGlobal tp{slab.data()}, tq{slab.data() + 80};
        ge_p3 side[2];
        st = ed_dleq_lane(
            st, cw, rw, full != 0, tp, tq,
            [&](int s, uint32_t(&pw)[8], uint32_t(&qw)[8]) {
                words(pw, s ? H + hs * i : G + gs * i);
                words(qw, (s ? xH : xG) + 32 * i);
            },
            [&](int s, const ge_p3& h) { side[s] = h; });
        uint32_t ea[8], eb[8], cu[8], cv[8];
        ge_p3_towords(ea, side[0]);
        ge_p3_towords(eb, side[1]);
        ed_canon_point_bytes(cu, u);
        ed_canon_point_bytes(cv, v);
        status[i] = (uint8_t)st;
        ok[i] = st == ED_ST_OK && ed_words8_equal(ea, cu) && ed_words8_equal(eb, cv);
    }
}
}
