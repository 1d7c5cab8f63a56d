// Ed25519 fused signature verification and double-scalar multiplication: kernels for gfx950 + their C-ABI entry points.
// The lane programs are ed25519_verify.cuh's; this unit is their kernels' own so that the tuned multiplication kernels of
// ed25519.hip keep their register allocation (a unit's out-of-line callees take the
// loosest budget of the kernels that reach them).
//
// Replaces, in the reference:
//   sign/eddsa VerifyWithChecks    eddsa.go:143-229   -> ed25519_verify_kernel + ed25519_verify_encode_kernel
//   sign/schnorr VerifyWithChecks  schnorr.go:84-160  -> the same two kernels
//   proof/dleq Proof.Verify        dleq.go:160-172    -> ed25519_mul2_kernel + ed25519_mul2_encode_kernel, twice
// Both programs keep their window tables in a global slab (TabGlobal: 1 280 B per table, lane-contiguous) and park
// (X, Y, Z) for the shared-inversion encoder at every batch size: one field inversion per ENC_CHUNK elements, and the
// verdict of a signature is taken in the encode pass.  Batches run in pieces of ED_PIECE lanes, so the per-stream slab
// is bounded whatever n is (ed25519_launch.h: the slab's layout, ED_SLAB_VERIFY / ED_SLAB_MUL2, and the piece loop).
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_verify.cuh"
#include "ed25519_launch.h"

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT &&
                  ED_ST_SIG_NONCANONICAL == KYB_ST_SIG_NONCANONICAL && ED_ST_SIG_SMALL_ORDER == KYB_ST_SIG_SMALL_ORDER,
              "status values of include/kyber_hip.h");

// One lane per signature.  Lanes past n repeat element n - 1 (the variable-time ladder's wave reductions want every
// lane) and store nothing.  A pair of offsets that decreases is read as an empty message, never as a length.
__global__ __launch_bounds__(128, 3) void ed25519_verify_kernel(
    size_t n, const uint32_t* __restrict__ pubs, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ sigs, const int32_t* __restrict__ wide, sf::Mod m, int32_t* __restrict__ proj,
    uint8_t* __restrict__ st, int4* __restrict__ gtab) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    uint32_t aw[8], rw[8], sw[8];
    load_words8(aw, pubs + idx * 8);
    load_words8(rw, sigs + idx * 16);
    load_words8(sw, sigs + idx * 16 + 8);
    const uint64_t lo = off[idx], hi = off[idx + 1];
    const size_t len = hi >= lo ? (size_t)(hi - lo) : 0;
    TabGlobal tab{gtab + lane * 80};
    ge_p3 T;
    const int s = ed_verify_lane(T, rw, sw, aw, msgs + lo, len, wide, m, tab);
    if (lane >= n) return;
    store_proj(proj, idx, T);
    st[idx] = (uint8_t)s;
}
// ok[i] = checks passed and encode(T_i) == R_i, one inversion per ENC_CHUNK signatures
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_verify_encode_kernel(
    size_t n, const int32_t* __restrict__ proj, const uint8_t* __restrict__ st, const uint32_t* __restrict__ sigs,
    uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t (&w)[8]) {
        uint32_t r[8];
        load_words8(r, sigs + i * 16);
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) diff |= r[k] ^ w[k];
        const uint8_t s = st[i];
        ok[i] = (s == KYB_ST_OK && diff == 0) ? 1 : 0;
        if (status) status[i] = s;
    });
}

// out = a P + b Q, one lane per element; table slab: 2 x 80 int4 per lane
__global__ __launch_bounds__(128, 3) void ed25519_mul2_kernel(
    size_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ P, const uint32_t* __restrict__ b,
    const uint32_t* __restrict__ Q, uint32_t flags, int32_t* __restrict__ proj, uint8_t* __restrict__ st,
    int4* __restrict__ gtab) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    uint32_t aw[8], pw[8], bw[8], qw[8];
    load_words8(aw, a + idx * 8);
    load_words8(pw, P + idx * 8);
    load_words8(bw, b + idx * 8);
    load_words8(qw, Q + idx * 8);
    TabGlobal tp{gtab + lane * 160}, tq{gtab + lane * 160 + 80};
    ge_p3 h;
    const bool ok = ed_mul2_lane(h, aw, pw, bw, qw, (flags & KYB_F_VARTIME) != 0, tp, tq);
    if (lane >= n) return;
    store_proj(proj, idx, h);
    st[idx] = ok ? KYB_ST_OK : KYB_ST_BAD_POINT;
}
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_mul2_encode_kernel(
    size_t n, const int32_t* __restrict__ proj, const uint8_t* __restrict__ st, uint32_t* __restrict__ out,
    uint8_t* __restrict__ status) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t (&w)[8]) {
        const uint8_t s = st[i];
        if (s) {
#pragma unroll
            for (int k = 0; k < 8; k++) w[k] = 0;
        }
        store_words8(out + i * 8, w);
        if (status) status[i] = s;
    });
}

static int launch_verify(size_t n, const void* d_pubs, const void* d_msgs, const void* d_off, const void* d_sigs,
                         void* d_ok, void* d_status, hipStream_t st) {
    return ed_for_pieces(n, st, ED_SLAB_VERIFY, [&](DeviceCtx* ctx, size_t lo, size_t cnt, const EdSlab& w) {
        const uint32_t* sigs = (const uint32_t*)d_sigs + lo * 16;
        hipLaunchKernelGGL(ed25519_verify_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)d_pubs + lo * 8, (const uint8_t*)d_msgs, (const uint64_t*)d_off + lo, sigs,
                           (const int32_t*)ctx->ed_wide_tab, ed_order(), w.proj, w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_verify_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, (const uint8_t*)w.status, sigs, (uint8_t*)d_ok + lo,
                           d_status ? (uint8_t*)d_status + lo : nullptr);
    });
}

static int launch_mul2(size_t n, const void* d_a, const void* d_P, const void* d_b, const void* d_Q, void* d_out,
                       void* d_status, uint32_t flags, hipStream_t st) {
    return ed_for_pieces(n, st, ED_SLAB_MUL2, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_mul2_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)d_a + lo * 8, (const uint32_t*)d_P + lo * 8, (const uint32_t*)d_b + lo * 8,
                           (const uint32_t*)d_Q + lo * 8, flags, w.proj, w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_mul2_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, (const uint8_t*)w.status, (uint32_t*)d_out + lo * 8,
                           d_status ? (uint8_t*)d_status + lo : nullptr);
    });
}

// one device's share of a host-buffer verification: offsets rebased to the first message of the share
static int verify_host(size_t n, const uint8_t* pubs, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs,
                       uint8_t* ok, uint8_t* status) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, off);
    // (msgs may be null when every message is empty: a present input of zero bytes)
    return staged_call(ctx, {{pubs, n * 32}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}, {sigs, n * 64}},
                       {{ok, n}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_verify(n, in[0], in[1], in[2], in[3], o[0], o[1], st);
                       });
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_verify_dev(size_t n, const void* d_pubkeys, const void* d_msgs, const void* d_msg_off, const void* d_sigs,
                           void* d_ok, void* d_status, uint32_t flags, void* stream) {
    if (int rc; ed_entry_done(&rc, n, (n && (!d_pubkeys || !d_msgs || !d_msg_off || !d_sigs || !d_ok)) || flags,
                              "kyb_ed25519_verify_dev: bad argument")) return rc;
    return launch_verify(n, d_pubkeys, d_msgs, d_msg_off, d_sigs, d_ok, d_status, (hipStream_t)stream);
}

int kyb_ed25519_verify(size_t n, const uint8_t* pubkeys, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* sigs,
                       uint8_t* ok, uint8_t* status, uint32_t flags) {
    if (int rc; ed_entry_done(&rc, n, (n && (!pubkeys || !msg_off || !sigs || !ok)) || flags,
                              "kyb_ed25519_verify: bad argument")) return rc;
    if (EdHostSpans::offsets_bad(n, msgs, msg_off)) {
        set_error("kyb_ed25519_verify: bad argument (message offsets must not decrease, nor name bytes of a NULL msgs)");
        return KYB_E_ARG;
    }
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return verify_host(hi - lo, pubkeys + 32 * lo, msgs, msg_off + lo, sigs + 64 * lo, ok + lo, status ? status + lo : nullptr);
        });
    return verify_host(n, pubkeys, msgs, msg_off, sigs, ok, status);
}

static bool mul2_args_bad(size_t n, const void* a, const void* P, const void* b, const void* Q, const void* out, uint32_t flags) {
    return (n && (!a || !P || !b || !Q || !out)) || (flags & ~KYB_F_VARTIME);  // KYB_F_UNIFORM: no scanned Straus chain
}

int kyb_ed25519_mul2_dev(size_t n, const void* d_a, const void* d_P, const void* d_b, const void* d_Q, void* d_out,
                         void* d_status, uint32_t flags, void* stream) {
    if (int rc; ed_entry_done(&rc, n, mul2_args_bad(n, d_a, d_P, d_b, d_Q, d_out, flags), "kyb_ed25519_mul2_dev: bad argument")) return rc;
    return launch_mul2(n, d_a, d_P, d_b, d_Q, d_out, d_status, flags, (hipStream_t)stream);
}

int kyb_ed25519_mul2(size_t n, const uint8_t* a, const uint8_t* P, const uint8_t* b, const uint8_t* Q, uint8_t* out,
                     uint8_t* status, uint32_t flags) {
    if (int rc; ed_entry_done(&rc, n, mul2_args_bad(n, a, P, b, Q, out, flags), "kyb_ed25519_mul2: bad argument")) return rc;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return kyb_ed25519_mul2(hi - lo, a + 32 * lo, P + 32 * lo, b + 32 * lo, Q + 32 * lo, out + 32 * lo,
                                    status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx, {{a, n * 32}, {P, n * 32}, {b, n * 32}, {Q, n * 32}}, {{out, n * 32}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_mul2(n, in[0], in[1], in[2], in[3], o[0], o[1], flags, st);
                       });
}
}
