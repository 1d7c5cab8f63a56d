// kyber_amd/csrc/ed25519_shuffle.cuh compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_shuffle_host.py runs the stream's output nodes, the candidate draws, the window and the theta lane program
// through these entry points against the Python XOF and the big-integer oracle; tests/test_gpu_shuffle.py uses
// shf_stream as its fast stream generator.  Window tables live in a TabGlobal slab and the point is encoded and compared
// as in the kernels.
#include "../kyber_amd/csrc/ed25519_shuffle.cuh"

#include <string.h>

#include <vector>

using namespace kyb;

static void words(uint32_t w[8], const uint8_t* p) { memcpy(w, p, 32); }  // little-endian host
static void root_block(uint64_t (&m)[16], const uint8_t* root) {
    uint64_t r[8];
    memcpy(r, root, 64);
    ed_xof_root_block(m, r);
}

extern "C" {
// out = output node `node` of the stream with this root hash (64 bytes)
void shf_node(const uint8_t* root, uint32_t node, uint8_t* out) {
    uint64_t m[16], h[8];
    root_block(m, root);
    ed_xof_node(h, m, node);
    memcpy(out, h, 64);
}
// out = len stream bytes from byte position pos, node by node
void shf_stream(const uint8_t* root, uint64_t pos, size_t len, uint8_t* out) {
    uint64_t m[16], h[8];
    root_block(m, root);
    size_t done = 0;
    while (done < len) {
        const uint64_t p = pos + done;
        const size_t off = (size_t)(p & 63), take = len - done < 64 - off ? len - done : 64 - off;
        ed_xof_node(h, m, (uint32_t)(p >> 6));
        memcpy(out + done, (const uint8_t*)h + off, take);
        done += take;
    }
}
// candidate draws first .. first + count of the window at pos: value[j] (32 bytes little-endian) and accept[j], each
// through ed_xof_draw as a lane computes it
void shf_draws(const uint8_t* root, uint64_t pos, uint64_t first, size_t count, uint8_t* value, uint8_t* accept) {
    uint64_t m[16];
    root_block(m, root);
    for (size_t j = 0; j < count; j++) {
        uint32_t c[8];
        accept[j] = ed_xof_draw(c, m, pos, first + j);
        memcpy(value + 32 * j, c, 32);
    }
}
uint64_t shf_window(uint64_t n) { return ed_xof_window(n); }
void shf_neg(const uint8_t* b, uint8_t* out) {
    const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    uint32_t w[8], r[8];
    words(w, b);
    ed_scalar_neg(r, w, m);
    memcpy(out, r, 32);
}
// the theta kernel's lane program + the encode pass's verdict, element by element.  U, W: NULL or one point
void shf_theta(size_t n, const uint8_t* a, const uint8_t* A, const uint8_t* U, const uint8_t* b, const uint8_t* B,
               const uint8_t* W, const uint8_t* T, int full, uint8_t* ok, uint8_t* status) {
    const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    std::vector<int4> slab(160);
    uint32_t uw[8], ww[8];
    if (U) words(uw, U);
    if (W) words(ww, W);
    for (size_t i = 0; i < n; i++) {
        uint32_t aw[8], Aw[8], bw[8], Bw[8], tw[8], ct[8], enc[8];
        words(aw, a + 32 * i);
        words(Aw, A + 32 * i);
        words(bw, b + 32 * i);
        words(Bw, B + 32 * i);
        words(tw, T + 32 * i);
        TabGlobal tp{slab.data()}, tq{slab.data() + 80};
        ge_p3 h;
        const int st = ed_theta_lane(h, aw, Aw, U ? uw : nullptr, bw, Bw, W ? ww : nullptr, full != 0, m, tp, tq);
        ge_p3_towords(enc, h);
        ed_canon_point_bytes(ct, tw);
        status[i] = (uint8_t)st;
        ok[i] = st == ED_ST_OK && ed_words8_equal(enc, ct);
    }
}
}
