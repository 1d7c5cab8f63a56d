// sign/anon Encrypt / Decrypt on Ed25519 (enc.go): kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_anonenc.cuh's; this unit is their kernels' own, so that the other Ed25519 units keep their kernels and their
// register allocation.
//
// Replaces, in the reference:
//   Encrypt   enc.go:123-148 over encryptKey and header(), enc.go:11-40
//             -> [ed25519_anon_tables_kernel], ed25519_anon_seal_head_kernel, ed25519_anon_points_kernel<SHARED>,
//                ed25519_anon_encode_kernel, ed25519_anon_slot_kernel<false>, ed25519_anon_body_kernel<false>
//   Decrypt   enc.go:165-192 over decryptKey and header(), enc.go:44-102
//             -> [ed25519_anon_tables_kernel], ed25519_anon_open_head_kernel, ed25519_anon_points_kernel<SHARED>,
//                ed25519_anon_encode_kernel, ed25519_anon_slot_kernel<true>, ed25519_anon_body_kernel<true>
// An element of ring keys is ring + 1 consecutive lanes of a piece: lane 0, its head, owns X (x B in a seal, xb B in an
// open) and the master secret xb; lane 1 + k owns the product with ring member k.  A lane's memory in the slab: a window
// table (80 int4), one parked (X, Y, Z) and 16 words -- the point's encoding in words 0 .. 7, a head's xb in words
// 8 .. 15; an element's status byte is the slab's.  Pieces are whole elements (ed_anon_piece).  With one set for the batch
// the ring's window tables are decoded and built once per call in the (WS_ED_ANON, stream) workspace; with a set per
// element each product lane builds its own in the slab.  Every call runs on the current device: none shards over a
// device set.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_anonenc.cuh"
#include "ed25519_launch.h"

namespace kyb {

static_assert(ED_DKG_ST_OK == KYB_ST_OK && ED_DKG_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_ANON_SHORT == KYB_ST_ANON_SHORT &&
                  ED_ST_ANON_INVALID == KYB_ST_ANON_INVALID && ED_ST_ANON_MAC == KYB_ST_ANON_MAC && ED_ANON_MAX_RING == KYB_ANON_MAX_RING && ED_ANON_MAX_RING == ED_ANON_SLAB_MAX_RING,
              "status values and the ring's bound of include/kyber_hip.h");

constexpr size_t ANON_LANE_WORDS = 16;  // a lane's words in the slab's digit field: the encoding, then a head's xb
constexpr unsigned ED_HASH_BLOCK = 64;

// One lane per member of the set a call shares: its window table at tabs + 80 k; *bad set where one does not decode
__global__ __launch_bounds__(64, 3) void ed25519_anon_tables_kernel(size_t ring, const uint32_t* __restrict__ keys, int4* __restrict__ tabs,
                                                                     uint8_t* __restrict__ bad) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ring) return;
    uint32_t w[8];
    load_words8(w, keys + k * 8);
    if (!ed_anon_table(tabs + k * ED_TAB_INT4, w)) *bad = 1;  // (every lane that stores here stores the same value)
}

// One lane per message: X = x B parked in the element's head lane, xb = x mod l beside it; the element's status starts
// as the shared set's verdict
__global__ __launch_bounds__(128, 3) void ed25519_anon_seal_head_kernel(size_t n, size_t ring, const uint32_t* __restrict__ x,
                                                                         const int32_t* __restrict__ wide, sf::Mod m,
                                                                         const uint8_t* __restrict__ shared_bad, int32_t* __restrict__ proj,
                                                                         uint32_t* __restrict__ words, uint8_t* __restrict__ st) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t xw[8], xb[8];
    load_words8(xw, x + e * 8);
    ge_p3 X;
    ed_anon_seal_head(X, xb, xw, wide, m);
    const size_t j = e * (ring + 1);
    store_proj(proj, j, X);
    store_words8(words + j * ANON_LANE_WORDS + 8, xb);
    st[e] = (shared_bad && *shared_bad) ? KYB_ST_BAD_POINT : KYB_ST_OK;
}

// One lane per ciphertext: the checks in front of the ring, xb recovered with the receiver's key, xb B parked in the
// element's head lane.  priv_stride: 8 words, or 0 for one receiver.  mine is taken modulo ring.
__global__ __launch_bounds__(128, 3) void ed25519_anon_open_head_kernel(size_t n, size_t ring, const uint32_t* __restrict__ mine,
                                                                         const uint32_t* __restrict__ privs, size_t priv_stride,
                                                                         const uint8_t* __restrict__ cts, const uint64_t* __restrict__ off,
                                                                         const int32_t* __restrict__ wide, int4* __restrict__ gtab,
                                                                         int32_t* __restrict__ proj, uint32_t* __restrict__ words,
                                                                         uint8_t* __restrict__ st) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t pw[8], xb[8];
    load_words8(pw, privs + e * priv_stride);
    const size_t j = e * (ring + 1);
    Tab29 tab{gtab + j * ED_TAB_INT4};
    ge_p3 XB;
    const int s = ed_anon_open_head(XB, xb, pw, cts + off[e], element_len(off, e), ring, (size_t)mine[e] % ring, wide, tab);
    store_proj(proj, j, XB);
    store_words8(words + j * ANON_LANE_WORDS + 8, xb);
    st[e] = (uint8_t)s;
}

// One lane per (element, ring member), flat over the piece's lanes; the heads' lanes leave at once.  The scalar of
// element e is scal[e * scal_stride ..]: the caller's x in a seal, the head's parked xb in an open.  An element that
// already has a status parks the identity and runs no ladder.  SHARED: the member's table is the call's (tabs + 80 k),
// and a member that does not decode was found when the tables were built (shared_bad); otherwise the lane decodes its
// member from keys[e * key_stride ..], builds the table in its slab and marks the element where it does not decode.
template <bool SHARED>
__global__ __launch_bounds__(128, 3) void ed25519_anon_points_kernel(size_t lanes, size_t ring, const uint32_t* __restrict__ scal,
                                                                      size_t scal_stride, const uint32_t* __restrict__ keys, size_t key_stride,
                                                                      const int4* __restrict__ tabs, const uint8_t* __restrict__ shared_bad,
                                                                      int4* __restrict__ gtab, int32_t* __restrict__ proj,
                                                                      uint8_t* __restrict__ st) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= lanes) return;
    const size_t e = j / (ring + 1), k = j % (ring + 1);
    if (k == 0) return;
    if (SHARED && *shared_bad && st[e] == KYB_ST_OK) st[e] = KYB_ST_BAD_POINT;  // (an open: after the head's checks)
    ge29_p3 S;
    if (st[e] != KYB_ST_OK) {
        ge_p3_0(S);
        store_proj(proj, j, S);
        return;
    }
    uint32_t sw[8];
    load_words8(sw, scal + e * scal_stride);
    if constexpr (SHARED) {
        ed_anon_product_shared(S, sw, tabs + (k - 1) * ED_TAB_INT4);
    } else {
        uint32_t yw[8];
        load_words8(yw, keys + e * key_stride + (k - 1) * 8);
        if (!ed_anon_product_own(S, sw, yw, gtab + j * ED_TAB_INT4)) st[e] = KYB_ST_BAD_POINT;  // (the same value from every lane)
    }
    store_proj(proj, j, S);
}

// The encodings of a piece's parked points, one inversion per ENC_CHUNK points, into words 0 .. 7 of each lane
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_anon_encode_kernel(size_t points, const int32_t* __restrict__ proj,
                                                                                         uint32_t* __restrict__ words) {
    EncPreScratch pre;
    ed_encode_chunk(points, proj, ed_encode_first(), blockDim.x, pre,
                    [&](size_t i, uint32_t(&w)[8]) { store_words8(words + i * ANON_LANE_WORDS, w); });
}

// One lane per point.  A seal (OPEN = false) writes the header: the head X's bytes, a product's slot xb ^ XOF(S)[0:32];
// all zero where the element has a status.  Ciphertext e of the piece lies at bytes + off[e] + (first + e) * overhead.
// An open compares instead -- X on canonical bytes with xb B, a slot with the ciphertext's -- and marks the element
// KYB_ST_ANON_INVALID on a mismatch; elements that already have a status are left alone.
template <bool OPEN>
__global__ __launch_bounds__(ED_HASH_BLOCK, KYB_TU_WAVES) void ed25519_anon_slot_kernel(size_t lanes, size_t ring, size_t first,
                                                                                        const uint32_t* __restrict__ words,
                                                                                        const uint64_t* __restrict__ off,
                                                                                        uint8_t* __restrict__ bytes, uint8_t* __restrict__ st) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= lanes) return;
    const size_t e = j / (ring + 1), k = j % (ring + 1);
    const int s = st[e];
    if (OPEN && s != KYB_ST_OK) return;
    uint8_t* at = bytes + off[e] + (OPEN ? 0 : (first + e) * anon_overhead(ring)) + 32 * k;
    uint32_t enc[8], w[8];
    load_words8(enc, words + j * ANON_LANE_WORDS);
    if (k == 0) {
        if constexpr (OPEN) {
            uint32_t raw[8];
            ed_anon_load32(raw, at);
            ed_canon_point_bytes(w, raw);
            if (!ed_words8_equal(w, enc)) st[e] = KYB_ST_ANON_INVALID;  // (the same value from every lane that stores)
            return;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = enc[i];
    } else {
        uint32_t xb[8];
        load_words8(xb, words + e * (ring + 1) * ANON_LANE_WORDS + 8);
        ed_anon_slot(w, enc, xb);
        if constexpr (OPEN) {
            uint32_t have[8];
            ed_anon_load32(have, at);
            if (!ed_words8_equal(w, have)) st[e] = KYB_ST_ANON_INVALID;
            return;
        }
    }
    if (s != KYB_ST_OK) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0;
    }
    ed_anon_store32(at, w);
}

// One lane per element: the message under XOF(xb) and its MAC.  A seal reads msgs[off[e] ..) and writes behind the
// header of ciphertext e; an open reads ciphertext e = in[off[e] .. off[e + 1]) and writes out + off[e].
template <bool OPEN>
__global__ __launch_bounds__(ED_HASH_BLOCK, KYB_TU_WAVES) void ed25519_anon_body_kernel(size_t n, size_t ring, size_t first,
                                                                                        const uint32_t* __restrict__ words,
                                                                                        const uint8_t* __restrict__ in,
                                                                                        const uint64_t* __restrict__ off, const uint8_t* __restrict__ st,
                                                                                        uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t xb[8];
    load_words8(xb, words + e * (ring + 1) * ANON_LANE_WORDS + 8);
    int s = st[e];
    const uint64_t len = element_len(off, e);
    if constexpr (OPEN)
        s = ed_anon_open_body(out + off[e], in + off[e], len, 32 + 32 * (uint64_t)ring, xb, s);
    else
        ed_anon_seal_body(out + off[e] + (first + e) * anon_overhead(ring) + 32 + 32 * ring, in + off[e], len, xb, s);
    if (status) status[e] = (uint8_t)s;
}

struct AnonSealArgs {
    size_t ring;
    const void* keys;
    size_t key_stride;
    const void *x, *msgs, *off;
    void *out, *status;
};
struct AnonOpenArgs {
    size_t ring;
    const void* keys;
    size_t key_stride;
    const void *mine, *privs;
    size_t priv_stride;
    const void *cts, *off;
    void *out, *status;
};

// The (WS_ED_ANON, stream) workspace of a call that shares one set:  [ the set's flag, 256 B | ring x 1 280 B of tables ].
// The caller holds enq_mu: the workspace and the kernels that read it are one unit.
struct AnonShared {
    const int4* tabs = nullptr;
    const uint8_t* bad = nullptr;
};
static int anon_shared_tables(DeviceCtx* ctx, size_t ring, const void* keys, hipStream_t st, AnonShared* sh) {
    void* ws;
    if (int rc = ctx_workspace(ctx, WS_ED_ANON, st, 256 + ring * ED_TAB_BYTES, &ws)) return rc;
    KYB_HIP_CHECK(hipMemsetAsync(ws, 0, 256, st));
    sh->bad = (const uint8_t*)ws;
    sh->tabs = (const int4*)((uint8_t*)ws + 256);
    hipLaunchKernelGGL(ed25519_anon_tables_kernel, ed_grid(ring, 64), dim3(64), 0, st, ring, (const uint32_t*)keys,
                       (int4*)sh->tabs, (uint8_t*)ws);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}

// the passes a seal and an open have in common, behind their heads: products, encodings
static void launch_ring(hipStream_t st, size_t cnt, size_t ring, const uint32_t* scal, size_t scal_stride, const uint32_t* keys,
                        size_t key_words, const AnonShared& sh, const EdSlab& w) {
    const size_t lanes = cnt * (ring + 1);
    const dim3 grid = ed_grid(lanes, 128);
    if (sh.tabs)
        hipLaunchKernelGGL(ed25519_anon_points_kernel<true>, grid, dim3(128), 0, st, lanes, ring, scal, scal_stride, keys, key_words, sh.tabs,
                           sh.bad, w.gtab, w.proj, w.status);
    else
        hipLaunchKernelGGL(ed25519_anon_points_kernel<false>, grid, dim3(128), 0, st, lanes, ring, scal, scal_stride, keys, key_words, sh.tabs,
                           sh.bad, w.gtab, w.proj, w.status);
    hipLaunchKernelGGL(ed25519_anon_encode_kernel, ed_encode_grid(lanes), dim3(ED_ENC_BLOCK), 0, st, lanes, (const int32_t*)w.proj, w.digits);
}

static int launch_anon_seal(size_t n, const AnonSealArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    AnonShared sh;
    if (!a.key_stride)
        if ((rc = anon_shared_tables(ctx, a.ring, a.keys, st, &sh))) return rc;
    const size_t ring = a.ring, kw = a.key_stride / 4;
    return ed_for_pieces(n, st, ed_slab_anon(ring, a.key_stride != 0), [&](DeviceCtx* c, size_t lo, size_t cnt, const EdSlab& w) {
        const size_t lanes = cnt * (ring + 1);
        const uint32_t* x = (const uint32_t*)a.x + lo * 8;
        const uint64_t* off = (const uint64_t*)a.off + lo;
        hipLaunchKernelGGL(ed25519_anon_seal_head_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt, ring, x,
                           (const int32_t*)c->ed_wide_tab, ed_order(), sh.bad, w.proj, w.digits, w.status);
        launch_ring(st, cnt, ring, x, 8, (const uint32_t*)a.keys + lo * kw, kw, sh, w);
        hipLaunchKernelGGL(ed25519_anon_slot_kernel<false>, ed_grid(lanes, ED_HASH_BLOCK), dim3(ED_HASH_BLOCK), 0,
                           st, lanes, ring, lo, (const uint32_t*)w.digits, off, (uint8_t*)a.out, w.status);
        hipLaunchKernelGGL(ed25519_anon_body_kernel<false>, ed_grid(cnt, ED_HASH_BLOCK), dim3(ED_HASH_BLOCK), 0, st,
                           cnt, ring, lo, (const uint32_t*)w.digits, (const uint8_t*)a.msgs, off, (const uint8_t*)w.status, (uint8_t*)a.out,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
    }, ed_anon_piece(ring));
}

static int launch_anon_open(size_t n, const AnonOpenArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    AnonShared sh;
    if (!a.key_stride)
        if ((rc = anon_shared_tables(ctx, a.ring, a.keys, st, &sh))) return rc;
    const size_t ring = a.ring, kw = a.key_stride / 4, ps = a.priv_stride / 4;
    return ed_for_pieces(n, st, ed_slab_anon(ring, true), [&](DeviceCtx* c, size_t lo, size_t cnt, const EdSlab& w) {
        const size_t lanes = cnt * (ring + 1);
        const uint64_t* off = (const uint64_t*)a.off + lo;
        hipLaunchKernelGGL(ed25519_anon_open_head_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt, ring,
                           (const uint32_t*)a.mine + lo, (const uint32_t*)a.privs + lo * ps, ps, (const uint8_t*)a.cts, off,
                           (const int32_t*)c->ed_wide_tab, w.gtab, w.proj, w.digits, w.status);
        launch_ring(st, cnt, ring, (const uint32_t*)w.digits + 8, (ring + 1) * ANON_LANE_WORDS, (const uint32_t*)a.keys + lo * kw, kw, sh, w);
        hipLaunchKernelGGL(ed25519_anon_slot_kernel<true>, ed_grid(lanes, ED_HASH_BLOCK), dim3(ED_HASH_BLOCK), 0,
                           st, lanes, ring, lo, (const uint32_t*)w.digits, off, (uint8_t*)a.cts, w.status);
        hipLaunchKernelGGL(ed25519_anon_body_kernel<true>, ed_grid(cnt, ED_HASH_BLOCK), dim3(ED_HASH_BLOCK), 0, st,
                           cnt, ring, lo, (const uint32_t*)w.digits, (const uint8_t*)a.cts, off, (const uint8_t*)w.status, (uint8_t*)a.out,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
    }, ed_anon_piece(ring));
}

static bool ring_bad(size_t ring, size_t key_stride) {
    return ring == 0 || ring > ED_ANON_MAX_RING || (key_stride != 0 && key_stride != 32 * ring);
}
static bool seal_args_bad(size_t n, const AnonSealArgs& a) {
    return ring_bad(a.ring, a.key_stride) || (n && (!a.keys || !a.x || !a.off || !a.out));
}
static bool open_args_bad(size_t n, const AnonOpenArgs& a) {
    return ring_bad(a.ring, a.key_stride) || stride_bad(a.priv_stride) ||
           (n && (!a.keys || !a.mine || !a.privs || !a.off || !a.out));
}

}  // namespace kyb

using namespace kyb;

extern "C" {

// sign/anon Encrypt (enc.go:123-148) for a batch
int kyb_ed25519_anon_seal_dev(size_t n, size_t ring, const void* d_keys, size_t key_stride, const void* d_x, const void* d_msgs,
                              const void* d_msg_off, void* d_out, void* d_status, void* stream) {
    const AnonSealArgs a{ring, d_keys, key_stride, d_x, d_msgs, d_msg_off, d_out, d_status};
    if (int rc; ed_entry_done(&rc, n, seal_args_bad(n, a), "kyb_ed25519_anon_seal_dev: bad argument")) return rc;
    return launch_anon_seal(n, a, (hipStream_t)stream);
}

int kyb_ed25519_anon_seal(size_t n, size_t ring, const uint8_t* keys, size_t key_stride, const uint8_t* x, const uint8_t* msgs,
                          const uint64_t* msg_off, uint8_t* out, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n,
                              seal_args_bad(n, AnonSealArgs{ring, keys, key_stride, x, msgs, msg_off, out, status}) ||
                                  (n && EdHostSpans::offsets_bad(n, msgs, msg_off)),
                              "kyb_ed25519_anon_seal: bad argument (pointers; a ring of 1 .. KYB_ANON_MAX_RING keys at a stride of 0 or 32 ring; "
                              "offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, msg_off);
    return staged_call(ctx,
                       {{keys, key_stride ? n * key_stride : 32 * ring}, {x, n * 32}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sp.at(out), sp.total + anon_overhead(ring) * n}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_anon_seal(n, AnonSealArgs{ring, in[0], key_stride, in[1], in[2], in[3], o[0], o[1]}, st);
                       });
}

// sign/anon Decrypt (enc.go:165-192) for a batch
int kyb_ed25519_anon_open_dev(size_t n, size_t ring, const void* d_keys, size_t key_stride, const void* d_mine, const void* d_privs,
                              size_t priv_stride, const void* d_ctx, const void* d_ctx_off, void* d_out, void* d_status, void* stream) {
    const AnonOpenArgs a{ring, d_keys, key_stride, d_mine, d_privs, priv_stride, d_ctx, d_ctx_off, d_out, d_status};
    if (int rc; ed_entry_done(&rc, n, open_args_bad(n, a), "kyb_ed25519_anon_open_dev: bad argument")) return rc;
    return launch_anon_open(n, a, (hipStream_t)stream);
}

int kyb_ed25519_anon_open(size_t n, size_t ring, const uint8_t* keys, size_t key_stride, const uint32_t* mine, const uint8_t* privs,
                          size_t priv_stride, const uint8_t* ctx_bytes, const uint64_t* ctx_off, uint8_t* out, uint8_t* status) {
    bool bad = open_args_bad(n, AnonOpenArgs{ring, keys, key_stride, mine, privs, priv_stride, ctx_bytes, ctx_off, out, status}) ||
               (n && EdHostSpans::offsets_bad(n, ctx_bytes, ctx_off));
    for (size_t i = 0; !bad && i < n; i++) bad = mine[i] >= ring;
    if (int rc; ed_entry_done(&rc, n, bad,
                              "kyb_ed25519_anon_open: bad argument (pointers; a ring of 1 .. KYB_ANON_MAX_RING keys at a stride of 0 or 32 ring; "
                              "mine inside the ring; a key stride of 0 or 32; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, ctx_bytes, ctx_off);
    return staged_call(ctx,
                       {{keys, key_stride ? n * key_stride : 32 * ring}, {mine, n * sizeof(uint32_t)}, {privs, priv_stride ? n * 32 : 32},
                        {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sp.at(out), sp.total}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_anon_open(n, AnonOpenArgs{ring, in[0], key_stride, in[1], in[2], priv_stride, in[3], in[4], o[0], o[1]},
                                                   st);
                       });
}
}
