// kyber_amd/csrc/ed25519_proof.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_proof_host.py runs the linear-combination lane program and the challenge lane through these entry points
// against the big-integer oracle and the Python XOF.  Memory is laid out as the kernels lay it out: the shared tables
// built once per call, a lane's own tables in a TabGlobal slab, the parked digits interleaved over the lanes of a block
// (here PRF_BLOCK lanes), and the point encoded and compared as in the encode pass.  Every buffer is a heap allocation
// of exactly the size the layout states, so that the sanitizer build (-DPROOF_HARNESS_MAIN,
// tests/test_proof_harness_sanitizers.py) sees a byte read or written past one.
#include "../kyber_amd/csrc/ed25519_proof.cuh"

#include <stdio.h>
#include <string.h>

#include <vector>

using namespace kyb;

constexpr size_t PRF_BLOCK = 3;  // lanes of a "block": the stride of the parked digits

extern "C" {
// kyb_ed25519_lincomb's value, element by element.  expect, out, ok: each may be NULL (ok needs expect).
void prf_lincomb(size_t n, size_t ko, size_t ks, const uint8_t* scalars, const uint8_t* own, const uint8_t* shared,
                 uint32_t nil_mask, const uint8_t* expect, int full, uint8_t* out, uint8_t* ok, uint8_t* status) {
    const size_t K = ko + ks, blocks = (n + PRF_BLOCK - 1) / PRF_BLOCK;
    std::vector<int4> sh_tab(80 * ks), own_tab(80 * ko);
    std::vector<uint32_t> digits(blocks * PRF_BLOCK * 8 * K), sw(8 * K), ow(8 * ko), shw(8 * ks);
    if (ks) memcpy(shw.data(), shared, 32 * ks);
    bool sh_ok = true;
    for (size_t j = 0; j < ks; j++) sh_ok &= ed_lincomb_shared_table(sh_tab.data() + 80 * j, shw.data() + 8 * j, (nil_mask >> j) & 1u);
    for (size_t i = 0; i < n; i++) {
        memcpy(sw.data(), scalars + 32 * K * i, 32 * K);
        if (ko) memcpy(ow.data(), own + 32 * ko * i, 32 * ko);
        const EdLincombMem mem{own_tab.data(), sh_tab.data(), digits.data() + (i / PRF_BLOCK) * PRF_BLOCK * 8 * K + i % PRF_BLOCK,
                               PRF_BLOCK};
        ge_p3 h;
        bool good = ed_lincomb_lane(h, (int)ko, (int)ks, nil_mask, sw.data(), ow.data(), full != 0, mem);
        good &= sh_ok;
        if (!good) ge_p3_0(h);
        uint32_t enc[8];
        ge_p3_towords(enc, h);
        if (!good) memset(enc, 0, 32);
        if (out) memcpy(out + 32 * i, enc, 32);
        if (ok) {
            uint32_t tw[8], ct[8];
            memcpy(tw, expect + 32 * i, 32);
            ed_canon_point_bytes(ct, tw);
            ok[i] = good && ed_words8_equal(enc, ct);
        }
        if (status) status[i] = good ? ED_ST_OK : ED_ST_BAD_POINT;
    }
}

// kyb_ed25519_fs_challenge's value, element by element.  off: NULL (one name of name_len bytes) or n + 1 offsets.
void prf_fs_challenge(size_t n, const uint8_t* names, const uint64_t* off, size_t name_len, const uint8_t* data, size_t data_len,
                      uint8_t* c, uint8_t* status) {
    for (size_t i = 0; i < n; i++) {
        const uint8_t* name = off ? names + off[i] : names;
        const size_t len = off ? (size_t)(off[i + 1] - off[i]) : name_len;
        uint32_t cw[8];
        status[i] = (uint8_t)ed_fs_challenge_lane(cw, name, len, data + i * data_len, data_len);
        memcpy(c + 32 * i, cw, 32);
    }
}
}

#ifdef PROOF_HARNESS_MAIN
// Every (ko, ks) shape and both flag values over exactly sized buffers, with nil terms, an undecodable own point and a
// scalar of all ones; the challenge at every name and data length of the tests.  Values are checked by
// tests/test_proof_host.py: this program is for the sanitizers.
static uint8_t* filled(size_t bytes, uint32_t& seed) {
    uint8_t* p = new uint8_t[bytes ? bytes : 1];
    for (size_t i = 0; i < bytes; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
int main() {
    uint32_t seed = 7;
    const size_t n = 4;
    for (size_t ko = 0; ko <= 4; ko++)
        for (size_t ks = 0; ks <= 4; ks++) {
            if (ko + ks == 0) continue;
            for (int full = 0; full < 2; full++) {
                uint8_t* s = filled(n * (ko + ks) * 32, seed);
                uint8_t* own = filled(n * ko * 32, seed);
                uint8_t* sh = filled(ks * 32, seed);
                uint8_t* ex = filled(n * 32, seed);
                memset(s, 0xff, 32);
                uint8_t *out = new uint8_t[n * 32], *ok = new uint8_t[n], *st = new uint8_t[n];
                prf_lincomb(n, ko, ks, s, ko ? own : nullptr, ks ? sh : nullptr, ks ? 1u << (ks - 1) : 0u, ex, full, out, ok, st);
                prf_lincomb(n, ko, ks, s, ko ? own : nullptr, ks ? sh : nullptr, 0, nullptr, full, out, nullptr, st);
                delete[] s; delete[] own; delete[] sh; delete[] ex; delete[] out; delete[] ok; delete[] st;
            }
        }
    const size_t name_lens[] = {0, 1, 63, 64, 65, 128, 129}, data_lens[] = {0, 32, 96, 2048};
    for (size_t nl : name_lens)
        for (size_t dl : data_lens) {
            uint8_t* names = filled(nl, seed);
            uint8_t* data = filled(2 * dl, seed);
            uint8_t c[64], st[2];
            prf_fs_challenge(2, names, nullptr, nl, data, dl, c, st);
            const uint64_t off[3] = {0, nl / 2, nl};
            prf_fs_challenge(2, names, off, 0, data, dl, c, st);
            delete[] names; delete[] data;
        }
    puts("ok");
    return 0;
}
#endif
