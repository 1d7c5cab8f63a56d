// kyber_amd/csrc/ed25519_ring.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_ring_host.py runs the ring chain and the challenge through these entry points against the sign/anon
// oracle.  Window tables, the parked point and the hash midstate live in host memory laid out as the kernels lay them
// out in the slab; the shared tables are built the way ed25519_ring_tables_kernel builds them.
#include "../kyber_amd/csrc/ed25519_ring.cuh"

#include <string.h>

#include <vector>

using namespace kyb;

extern "C" {
// kyb_ed25519_ring_chain's arguments, element by element.  Buffers of 32-byte items must be 16-byte aligned.
void rng_chain(size_t n, size_t ring, const uint8_t* keys, size_t key_stride, const uint8_t* msgs, const uint64_t* off,
               const uint8_t* scope, size_t scope_len, const uint8_t* link_base, const uint8_t* sigs, size_t sig_stride,
               const uint32_t* start, size_t steps, int full, uint8_t* c_zero, uint8_t* c_out, uint8_t* ok, uint8_t* status) {
    const bool shared = key_stride == 0;
    const size_t ntab = ED_RING_TAB_KEYS + (shared ? ring : 0);
    std::vector<int4> tabs(80 * ntab);
    std::vector<uint8_t> bad(ntab, 0);
    for (size_t k = 0; k < ntab; k++) {
        if (k == (size_t)ED_RING_TAB_LINK && !link_base) continue;
        ge_p3 A;
        if (k == (size_t)ED_RING_TAB_G) {
            A.X = fe_bx(); A.Y = fe_by(); fe_1(A.Z); A.T = fe_bt();
        } else {
            uint32_t w[8];
            memcpy(w, k == (size_t)ED_RING_TAB_LINK ? link_base : keys + 32 * (k - ED_RING_TAB_KEYS), 32);
            bad[k] = ge_p3_fromwords(A, w) ? 0 : 1;
        }
        TabGlobal t{tabs.data() + 80 * k};
        ge_window_table(t, A);
    }
    const EdRingShared sh{tabs.data(), bad.data()};
    std::vector<int4> lane_tabs(160);
    std::vector<uint64_t> lane_mem(75);  // 600 bytes: the parked point, then the midstate at byte 128
    for (size_t i = 0; i < n; i++) {
        EdRingSig s;
        s.ring = ring;
        s.keys = shared ? nullptr : (const uint32_t*)(keys + key_stride * i);
        s.sig = (const uint32_t*)(sigs + sig_stride * i);
        s.msg = msgs + off[i];
        s.len = (size_t)(off[i + 1] - off[i]);
        s.scope = scope;
        s.scope_len = scope_len;
        int32_t* park = (int32_t*)lane_mem.data();
        const EdRingLaneMem mem{lane_tabs.data(), lane_tabs.data() + 80, park, (EdRingMid*)((uint8_t*)park + 128)};
        uint32_t c[8];
        const int st = ed_ring_lane(c, s, start ? start[i] % ring : 0, steps, full != 0, sh, mem);
        uint32_t c0[8];
        memcpy(c0, s.sig, 32);
        ok[i] = st == ED_ST_OK && ed_words8_equal(c, c0);
        status[i] = (uint8_t)st;
        if (st) {
            memset(c_out + 32 * i, 0, 32);
            memset(c_zero + 32 * i, 0, 32);
        } else {
            memcpy(c_out + 32 * i, c, 32);
            memcpy(c_zero + 32 * i, mem.mid->czero, 32);
        }
    }
}
// kyb_ed25519_ring_challenge's arguments, element by element
void rng_challenge(size_t n, const uint8_t* msgs, const uint64_t* off, const uint8_t* scope, size_t scope_len,
                   const uint8_t* tags, const uint8_t* PG, const uint8_t* PH, uint8_t* c, uint8_t* status) {
    std::vector<uint64_t> lane_mem(75);
    for (size_t i = 0; i < n; i++) {
        uint32_t tw[8] = {0}, pg[8], ph[8] = {0}, cw[8];
        memcpy(pg, PG + 32 * i, 32);
        if (scope) {
            memcpy(tw, tags + 32 * i, 32);
            memcpy(ph, PH + 32 * i, 32);
        }
        uint8_t* mem = (uint8_t*)lane_mem.data();
        status[i] = (uint8_t)ed_ring_challenge_lane(cw, msgs + off[i], (size_t)(off[i + 1] - off[i]), scope, scope_len, tw, pg, ph,
                                                    (EdRingMid*)(mem + 128), (uint32_t*)mem);
        memcpy(c + 32 * i, cw, 32);
    }
}
}
