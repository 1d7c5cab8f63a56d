// Ed25519 ring signatures (sign/anon): kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_ring.cuh's; this unit is their kernels' own, so that ed25519.o, ed25519_verify.o and ed25519_dleq.o keep
// their kernels and their register allocation.
//
// Replaces, in the reference:
//   sign/anon Verify, the ring loop   sig.go:231-238   -> ed25519_ring_chain_kernel (start = 0, steps = ring)
//   sign/anon Sign, the ring loop     sig.go:159-166   -> the same, from mine + 1 for ring - 1 steps
//   sign/anon signH1 over signH1pre   sig.go:23-43     -> ed25519_ring_challenge_kernel
// Window tables never live in scratch.  What a call shares -- the standard base's table, linkBase's, and the ring
// members' when the batch shares one ring -- is built once per call by ed25519_ring_tables_kernel, one lane per table,
// into the (WS_ED_RING, stream) workspace, and only read by the chain.  Per lane, in the (WS_ED, stream) slab
// (ed25519_launch.h, ED_SLAB_RING): the tag's table, built once per signature; the ring member's, rebuilt each step
// when every signature has a ring of its own; PG's parked (X, Y, Z) and the hash midstate.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_launch.h"
#include "ed25519_ring.cuh"

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_PICK_EXHAUSTED == KYB_ST_PICK_EXHAUSTED,
              "status values of include/kyber_hip.h");
static_assert(sizeof(EdRingMid) + ED_RING_MID_OFFSET <= ED_SLAB_RING.parked * ED_PROJ_LIMBS * sizeof(int32_t) &&
                  ED_SLAB_RING_CHALLENGE.parked == ED_SLAB_RING.parked,
              "the midstate inside the lane's parked slots");
constexpr size_t ED_RING_LANE_LIMBS = ED_SLAB_RING.parked * ED_PROJ_LIMBS;  // int32 words of parked memory per lane

// Table k of the call's shared tables, one lane per table: 0 the standard base, 1 linkBase (left alone when the call
// has none), 2 + i ring member i.
__global__ __launch_bounds__(64) void ed25519_ring_tables_kernel(size_t count, const uint32_t* __restrict__ link_base,
                                                                 const uint32_t* __restrict__ keys, int4* __restrict__ tabs,
                                                                 uint8_t* __restrict__ bad) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    if (k == ED_RING_TAB_LINK && !link_base) {
        bad[k] = 0;
        return;
    }
    ge_p3 A;
    bool good = true;
    if (k == ED_RING_TAB_G) {
        A.X = fe_bx(); A.Y = fe_by(); fe_1(A.Z); A.T = fe_bt();
    } else {
        uint32_t w[8];
        load_words8(w, k == ED_RING_TAB_LINK ? link_base : keys + 8 * (k - ED_RING_TAB_KEYS));
        good = ge_p3_fromwords(A, w);
    }
    TabGlobal t{tabs + 80 * k};
    ge_window_table(t, A);
    bad[k] = good ? 0 : 1;
}

// One lane per signature, the whole chain in the lane.  Lanes past n repeat element n - 1 (the variable-time chain's
// wave reductions want every lane) and store nothing.  keys: nullptr when the ring is shared (its tables are sh's),
// else ring x 8 words per signature.  sig_words: words between consecutive signatures.  A start position is taken
// modulo ring.  Outputs are each nullable; c_zero and c_out are zero bytes where the status is not 0.
__global__ __launch_bounds__(128, 3) void ed25519_ring_chain_kernel(
    size_t n, size_t ring, const uint32_t* __restrict__ keys, const uint8_t* __restrict__ msgs,
    const uint64_t* __restrict__ off, const uint8_t* __restrict__ scope, size_t scope_len, const uint32_t* __restrict__ sigs,
    size_t sig_words, const uint32_t* __restrict__ start, size_t steps, uint32_t flags, EdRingShared sh,
    int4* __restrict__ gtab, int32_t* __restrict__ proj, uint32_t* __restrict__ c_zero, uint32_t* __restrict__ c_out,
    uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    const uint64_t lo = off[idx], hi = off[idx + 1];
    EdRingSig s;
    s.ring = ring;
    s.keys = keys ? keys + idx * ring * 8 : nullptr;
    s.sig = sigs + idx * sig_words;
    s.msg = msgs + lo;
    s.len = hi >= lo ? (size_t)(hi - lo) : 0;  // a pair of offsets that decreases is an empty message
    s.scope = scope;
    s.scope_len = scope_len;
    int32_t* park = proj + lane * ED_RING_LANE_LIMBS;
    const EdRingLaneMem mem{gtab + lane * 160, gtab + lane * 160 + 80, park,
                            reinterpret_cast<EdRingMid*>(reinterpret_cast<uint8_t*>(park) + ED_RING_MID_OFFSET)};
    uint32_t c[8];
    const int st = ed_ring_lane(c, s, start ? (size_t)(start[idx] % ring) : 0, steps, (flags & KYB_F_VARTIME) != 0, sh, mem);
    if (lane >= n) return;
    uint32_t c0[8], cz[8];
    load_words8(c0, s.sig);
    const bool same = ed_words8_equal(c, c0);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        cz[i] = st ? 0u : mem.mid->czero[i];
        if (st) c[i] = 0;
    }
    if (c_zero) store_words8(c_zero + idx * 8, cz);
    if (c_out) store_words8(c_out + idx * 8, c);
    if (ok) ok[idx] = (st == ED_ST_OK && same) ? 1 : 0;
    if (status) status[idx] = (uint8_t)st;
}

// c[i] = signH1 of element i, one lane per element.  Nothing here is wave-collective, so lanes past n simply leave.
__global__ __launch_bounds__(128, 3) void ed25519_ring_challenge_kernel(
    size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off, const uint8_t* __restrict__ scope,
    size_t scope_len, const uint32_t* __restrict__ tags, const uint32_t* __restrict__ PG, const uint32_t* __restrict__ PH,
    int32_t* __restrict__ proj, uint32_t* __restrict__ c, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t lo = off[i], hi = off[i + 1];
    uint32_t tw[8], pg[8], ph[8], cw[8];
    load_words8(pg, PG + i * 8);
#pragma unroll
    for (int k = 0; k < 8; k++) tw[k] = ph[k] = 0;
    if (scope) {
        load_words8(tw, tags + i * 8);
        load_words8(ph, PH + i * 8);
    }
    int32_t* mem = proj + i * ED_RING_LANE_LIMBS;
    const int st = ed_ring_challenge_lane(cw, msgs + lo, hi >= lo ? (size_t)(hi - lo) : 0, scope, scope_len, tw, pg, ph,
                                          reinterpret_cast<EdRingMid*>(reinterpret_cast<uint8_t*>(mem) + ED_RING_MID_OFFSET),
                                          reinterpret_cast<uint32_t*>(mem));
    store_words8(c + i * 8, cw);
    if (status) status[i] = (uint8_t)st;
}

struct RingArgs {
    size_t ring;
    const void* keys;
    size_t key_stride;
    const void *msgs, *off, *scope;
    size_t scope_len;
    const void *link_base, *sigs;
    size_t sig_stride;
    const void* start;
    size_t steps;
    void *c_zero, *c_out, *ok, *status;
    uint32_t flags;
};

static bool chain_args_bad(size_t n, const RingArgs& a) {
    if (a.ring == 0) return true;
    if (a.key_stride != 0 && a.key_stride != 32 * a.ring) return true;
    if ((a.scope != nullptr) != (a.link_base != nullptr)) return true;
    if (a.sig_stride != 32 * (a.ring + (a.scope ? 2 : 1))) return true;
    if (a.flags & ~KYB_F_VARTIME) return true;  // KYB_F_UNIFORM: no scanned Straus chain
    return n && (!a.keys || !a.off || !a.sigs);
}

static int launch_chain(size_t n, const RingArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the shared tables and the pieces as one unit
    const bool shared = a.key_stride == 0;
    const size_t ntab = ED_RING_TAB_KEYS + (shared ? a.ring : 0);
    void* base;
    if ((rc = ctx_workspace(ctx, WS_ED_RING, st, ntab * (ED_TAB_BYTES + 1), &base))) return rc;
    const EdRingShared sh{(const int4*)base, (const uint8_t*)base + ntab * ED_TAB_BYTES};
    hipLaunchKernelGGL(ed25519_ring_tables_kernel, ed_grid(ntab, 64), dim3(64), 0, st, ntab,
                       (const uint32_t*)a.link_base, (const uint32_t*)a.keys, (int4*)base, (uint8_t*)base + ntab * ED_TAB_BYTES);
    KYB_HIP_CHECK(hipGetLastError());
    const size_t kw = a.key_stride / 4, sw = a.sig_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_RING, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_ring_chain_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt, a.ring,
                           shared ? (const uint32_t*)nullptr : (const uint32_t*)a.keys + lo * kw, (const uint8_t*)a.msgs,
                           (const uint64_t*)a.off + lo, (const uint8_t*)a.scope, a.scope_len, (const uint32_t*)a.sigs + lo * sw,
                           sw, a.start ? (const uint32_t*)a.start + lo : nullptr, a.steps, a.flags, sh, w.gtab, w.proj,
                           a.c_zero ? (uint32_t*)a.c_zero + lo * 8 : nullptr, a.c_out ? (uint32_t*)a.c_out + lo * 8 : nullptr,
                           a.ok ? (uint8_t*)a.ok + lo : nullptr, a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static int launch_challenge(size_t n, const void* msgs, const void* off, const void* scope, size_t scope_len, const void* tags,
                            const void* PG, const void* PH, void* c, void* status, hipStream_t st) {
    return ed_for_pieces(n, st, ED_SLAB_RING_CHALLENGE, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_ring_challenge_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint8_t*)msgs, (const uint64_t*)off + lo, (const uint8_t*)scope, scope_len,
                           scope ? (const uint32_t*)tags + lo * 8 : nullptr, (const uint32_t*)PG + lo * 8,
                           scope ? (const uint32_t*)PH + lo * 8 : nullptr, w.proj, (uint32_t*)c + lo * 8,
                           status ? (uint8_t*)status + lo : nullptr);
    });
}

// one device's share of a host-buffer chain: offsets rebased to the first message of the share
static int chain_host(size_t n, const RingArgs& a) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, a.msgs, (const uint64_t*)a.off);
    return staged_call(ctx,
                       {{a.keys, a.key_stride ? n * a.key_stride : 32 * a.ring},
                        {sp.base, sp.total},
                        {sp.offsets(), sp.offsets_bytes()},
                        {a.scope, a.scope_len, /*absent=*/!a.scope},
                        {a.link_base, 32, /*absent=*/!a.link_base},
                        {a.sigs, n * a.sig_stride},
                        {a.start, n * sizeof(uint32_t), /*absent=*/!a.start}},
                       {{a.c_zero, n * 32}, {a.c_out, n * 32}, {a.ok, n}, {a.status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           RingArgs d = a;
                           d.keys = in[0];
                           d.msgs = in[1];
                           d.off = in[2];
                           d.scope = in[3];
                           d.link_base = in[4];
                           d.sigs = in[5];
                           d.start = in[6];
                           d.c_zero = o[0];
                           d.c_out = o[1];
                           d.ok = o[2];
                           d.status = o[3];
                           return launch_chain(n, d, st);
                       });
}

static int challenge_host(size_t n, const uint8_t* msgs, const uint64_t* off, const uint8_t* scope, size_t scope_len,
                          const uint8_t* tags, const uint8_t* PG, const uint8_t* PH, uint8_t* c, uint8_t* status) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, off);
    return staged_call(ctx,
                       {{sp.base, sp.total},
                        {sp.offsets(), sp.offsets_bytes()},
                        {scope, scope_len, /*absent=*/!scope},
                        {tags, n * 32, /*absent=*/!scope},
                        {PG, n * 32},
                        {PH, n * 32, /*absent=*/!scope}},
                       {{c, n * 32}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_challenge(n, in[0], in[1], in[2], scope_len, in[3], in[4], in[5], o[0], o[1], st);
                       });
}

static bool challenge_args_bad(size_t n, const void* off, const void* scope, const void* tags, const void* PG, const void* PH,
                               const void* c) {
    if (!scope && (tags || PH)) return true;  // a tag or a PH belongs to a linkable signature
    return n && (!off || !PG || !c || (scope && (!tags || !PH)));
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_ring_chain_dev(size_t n, size_t ring, const void* d_keys, size_t key_stride, const void* d_msgs,
                               const void* d_msg_off, const void* d_scope, size_t scope_len, const void* d_link_base,
                               const void* d_sigs, size_t sig_stride, const void* d_start, size_t steps, void* d_c_zero,
                               void* d_c_out, void* d_ok, void* d_status, uint32_t flags, void* stream) {
    const RingArgs a{ring, d_keys, key_stride, d_msgs, d_msg_off, d_scope, scope_len, d_link_base, d_sigs, sig_stride,
                     d_start, steps, d_c_zero, d_c_out, d_ok, d_status, flags};
    if (int rc; ed_entry_done(&rc, n, chain_args_bad(n, a) || (n && !d_msgs), "kyb_ed25519_ring_chain_dev: bad argument")) return rc;
    return launch_chain(n, a, (hipStream_t)stream);
}

int kyb_ed25519_ring_chain(size_t n, size_t ring, const uint8_t* keys, size_t key_stride, const uint8_t* msgs,
                           const uint64_t* msg_off, const uint8_t* scope, size_t scope_len, const uint8_t* link_base,
                           const uint8_t* sigs, size_t sig_stride, const uint32_t* start, size_t steps, uint8_t* c_zero,
                           uint8_t* c_out, uint8_t* ok, uint8_t* status, uint32_t flags) {
    const RingArgs a{ring, keys, key_stride, msgs, msg_off, scope, scope_len, link_base, sigs, sig_stride,
                     start, steps, c_zero, c_out, ok, status, flags};
    if (int rc; ed_entry_done(&rc, n, chain_args_bad(n, a), "kyb_ed25519_ring_chain: bad argument")) return rc;
    if (EdHostSpans::offsets_bad(n, msgs, msg_off)) {
        set_error("kyb_ed25519_ring_chain: bad argument (message offsets must not decrease, nor name bytes of a NULL msgs)");
        return KYB_E_ARG;
    }
    if (start)
        for (size_t i = 0; i < n; i++)
            if (start[i] >= ring) {
                set_error("kyb_ed25519_ring_chain: bad argument (a start position outside the ring)");
                return KYB_E_ARG;
            }
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {  // the shared ring, scope and linkBase go to every shard
            RingArgs s = a;
            s.keys = keys + key_stride * lo;
            s.off = msg_off + lo;
            s.sigs = sigs + sig_stride * lo;
            s.start = start ? start + lo : nullptr;
            s.c_zero = c_zero ? c_zero + 32 * lo : nullptr;
            s.c_out = c_out ? c_out + 32 * lo : nullptr;
            s.ok = ok ? ok + lo : nullptr;
            s.status = status ? status + lo : nullptr;
            return chain_host(hi - lo, s);
        });
    return chain_host(n, a);
}

int kyb_ed25519_ring_challenge_dev(size_t n, const void* d_msgs, const void* d_msg_off, const void* d_scope, size_t scope_len,
                                   const void* d_tags, const void* d_PG, const void* d_PH, void* d_c, void* d_status,
                                   void* stream) {
    if (int rc; ed_entry_done(&rc, n, challenge_args_bad(n, d_msg_off, d_scope, d_tags, d_PG, d_PH, d_c) || (n && !d_msgs),
                              "kyb_ed25519_ring_challenge_dev: bad argument")) return rc;
    return launch_challenge(n, d_msgs, d_msg_off, d_scope, scope_len, d_tags, d_PG, d_PH, d_c, d_status, (hipStream_t)stream);
}

int kyb_ed25519_ring_challenge(size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* scope, size_t scope_len,
                               const uint8_t* tags, const uint8_t* PG, const uint8_t* PH, uint8_t* c, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n, challenge_args_bad(n, msg_off, scope, tags, PG, PH, c),
                              "kyb_ed25519_ring_challenge: bad argument")) return rc;
    if (EdHostSpans::offsets_bad(n, msgs, msg_off)) {
        set_error("kyb_ed25519_ring_challenge: bad argument (message offsets must not decrease, nor name bytes of a NULL msgs)");
        return KYB_E_ARG;
    }
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return challenge_host(hi - lo, msgs, msg_off + lo, scope, scope_len, tags ? tags + 32 * lo : nullptr, PG + 32 * lo,
                                  PH ? PH + 32 * lo : nullptr, c + 32 * lo, status ? status + lo : nullptr);
        });
    return challenge_host(n, msgs, msg_off, scope, scope_len, tags, PG, PH, c, status);
}
}
