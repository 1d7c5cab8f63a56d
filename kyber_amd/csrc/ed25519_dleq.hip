// Ed25519 discrete-log-equality proofs: kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_dleq.cuh's; this unit is their kernels' own, so that ed25519.o and ed25519_verify.o keep their kernels and
// their register allocation (a unit's out-of-line callees take the loosest budget of
// the kernels that reach them).
//
// Replaces, in the reference:
//   proof/dleq Proof.Verify        dleq.go:160-172   -> ed25519_dleq_kernel + ed25519_dleq_encode_kernel
//   share/pvss VerifyEncShare      pvss.go:154-163   -> the same, with expect_c
//   share/pvss VerifyDecShare      pvss.go:248-276   -> the same, with KYB_F_DLEQ_FS
//   proof/dleq NewDLEQProof        dleq.go:57-79     -> ed25519_dleq_challenge_kernel (the challenge; the rest is batch_mul)
// The verify kernel keeps two window tables per lane in the global slab (TabGlobal: 2 x 1 280 B, lane-contiguous; both
// sides of a proof rewrite the same two) and parks (X, Y, Z) of a and of b for the shared-inversion encoder, where the
// verdict is taken.  Batches run in pieces of ED_PIECE lanes, so the per-stream slab is bounded whatever n is
// (ed25519_launch.h: the slab's layout, ED_SLAB_DLEQ, and the piece loop).
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_dleq.cuh"
#include "ed25519_launch.h"

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_DLEQ_CHALLENGE == KYB_ST_DLEQ_CHALLENGE &&
                  ED_ST_PICK_EXHAUSTED == KYB_ST_PICK_EXHAUSTED,
              "status values of include/kyber_hip.h");

// c[i] = Pick(XOF(SHA-256(xG_i || xH_i || vG_i || vH_i))), one lane per element.  The rejection loop of the pick is the
// lane's own; nothing here is wave-collective, so lanes past n simply leave.
__global__ __launch_bounds__(128, 3) void ed25519_dleq_challenge_kernel(
    size_t n, const uint32_t* __restrict__ xG, const uint32_t* __restrict__ xH, const uint32_t* __restrict__ vG,
    const uint32_t* __restrict__ vH, uint32_t* __restrict__ c, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t a[8], b[8], u[8], v[8], cw[8];
    load_words8(a, xG + i * 8);
    load_words8(b, xH + i * 8);
    load_words8(u, vG + i * 8);
    load_words8(v, vH + i * 8);
    const int draws = ed_dleq_challenge(cw, a, b, u, v);
    store_words8(c + i * 8, cw);
    if (status) status[i] = draws ? KYB_ST_OK : KYB_ST_PICK_EXHAUSTED;
}

// One lane per proof.  Lanes past n repeat element n - 1 (the variable-time chain's wave reductions want every lane)
// and store nothing.  gs, hs: words between the bases of consecutive elements, 0 for one base shared by the batch.
// table slab: 2 x 80 int4 per lane; proj: 2 x 30 limbs per element (a, then b).
__global__ __launch_bounds__(128, 3) void ed25519_dleq_kernel(
    size_t n, const uint32_t* __restrict__ G, size_t gs, const uint32_t* __restrict__ H, size_t hs,
    const uint32_t* __restrict__ xG, const uint32_t* __restrict__ xH, const uint32_t* __restrict__ C,
    const uint32_t* __restrict__ R, const uint32_t* __restrict__ VG, const uint32_t* __restrict__ VH,
    const uint32_t* __restrict__ expect, uint32_t flags, int32_t* __restrict__ proj, uint8_t* __restrict__ st,
    int4* __restrict__ gtab) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    uint32_t cw[8], rw[8];
    load_words8(cw, C + idx * 8);
    int s;
    {  // first: the hash's working set and a point's never meet in the registers
        uint32_t a[8], b[8], u[8], v[8];
        const bool fs = (flags & KYB_F_DLEQ_FS) != 0;
        if (fs) {
            load_words8(a, xG + idx * 8);
            load_words8(b, xH + idx * 8);
            load_words8(u, VG + idx * 8);
            load_words8(v, VH + idx * 8);
        }
        s = ed_dleq_challenge_status(cw, expect, fs, a, b, u, v);
    }
    load_words8(rw, R + idx * 8);
    TabGlobal tp{gtab + lane * 160}, tq{gtab + lane * 160 + 80};
    const bool live = lane < n;
    s = ed_dleq_lane(
        s, cw, rw, (flags & KYB_F_VARTIME) != 0, tp, tq,
        [&](int side, uint32_t(&pw)[8], uint32_t(&qw)[8]) {
            load_words8(pw, side ? H + idx * hs : G + idx * gs);
            load_words8(qw, (side ? xH : xG) + idx * 8);
        },
        [&](int side, const ge_p3& h) {
            if (live) store_proj(proj, 2 * idx + side, h);
        });
    if (live) st[idx] = (uint8_t)s;
}

// ok[i] = status 0 and encode(a_i) == canon(VG_i) and encode(b_i) == canon(VH_i), one inversion per ENC_CHUNK parked
// points.  A lane's records are proofs -- a_i and b_i, two consecutive parked points -- and each is walked downwards, so
// the lane meets b_i just before a_i.
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_dleq_encode_kernel(
    size_t n, const int32_t* __restrict__ proj, const uint8_t* __restrict__ st, const uint32_t* __restrict__ VG,
    const uint32_t* __restrict__ VH, uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    static_assert(ENC_CHUNK % 2 == 0, "a and b of one proof share a chunk");
    bool b_same = false;
    EncPreScratch pre;
    ed_encode_chunk<2>(n, proj, ed_encode_first<2>(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        const size_t e = i >> 1;
        uint32_t v[8], cv[8];
        load_words8(v, ((i & 1) ? VH : VG) + e * 8);
        ed_canon_point_bytes(cv, v);
        const bool same = ed_words8_equal(cv, w);
        if (i & 1) {
            b_same = same;
        } else {
            const uint8_t s = st[e];
            ok[e] = (s == KYB_ST_OK && same && b_same) ? 1 : 0;
            if (status) status[e] = s;
        }
    });
}

static int launch_challenge(size_t n, const void* xG, const void* xH, const void* vG, const void* vH, void* c, void* status,
                            hipStream_t st) {
    DeviceCtx* ctx;
    const int rc = get_ctx(&ctx);
    if (rc) return rc;
    for (size_t lo = 0; lo < n; lo += ED_PIECE) {
        const size_t cnt = std::min(ED_PIECE, n - lo);
        hipLaunchKernelGGL(ed25519_dleq_challenge_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)xG + lo * 8, (const uint32_t*)xH + lo * 8, (const uint32_t*)vG + lo * 8,
                           (const uint32_t*)vH + lo * 8, (uint32_t*)c + lo * 8, status ? (uint8_t*)status + lo : nullptr);
        KYB_HIP_CHECK(hipGetLastError());
    }
    return KYB_OK;
}

struct DleqArgs {
    const void *G, *H, *xG, *xH, *C, *R, *VG, *VH, *expect;
    size_t g_stride, h_stride;
    void *ok, *status;
    uint32_t flags;
};

static int launch_verify(size_t n, const DleqArgs& a, hipStream_t st) {
    const size_t gs = a.g_stride / 4, hs = a.h_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_DLEQ, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        const uint32_t *VG = (const uint32_t*)a.VG + lo * 8, *VH = (const uint32_t*)a.VH + lo * 8;
        hipLaunchKernelGGL(ed25519_dleq_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.G + lo * gs, gs, (const uint32_t*)a.H + lo * hs, hs,
                           (const uint32_t*)a.xG + lo * 8, (const uint32_t*)a.xH + lo * 8, (const uint32_t*)a.C + lo * 8,
                           (const uint32_t*)a.R + lo * 8, VG, VH, (const uint32_t*)a.expect, a.flags, w.proj, w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_dleq_encode_kernel, ed_encode_grid(2 * cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, (const uint8_t*)w.status, VG, VH, (uint8_t*)a.ok + lo,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static bool verify_args_bad(size_t n, const DleqArgs& a) {
    if (a.flags & ~(KYB_F_VARTIME | KYB_F_DLEQ_FS)) return true;  // KYB_F_UNIFORM: no scanned Straus chain
    if ((a.g_stride != 0 && a.g_stride != 32) || (a.h_stride != 0 && a.h_stride != 32)) return true;
    if ((a.flags & KYB_F_DLEQ_FS) && a.expect) return true;  // one source for the challenge, not two
    return n && (!a.G || !a.H || !a.xG || !a.xH || !a.C || !a.R || !a.VG || !a.VH || !a.ok);
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_dleq_challenge_dev(size_t n, const void* d_xG, const void* d_xH, const void* d_vG, const void* d_vH, void* d_c,
                                   void* d_status, void* stream) {
    if (int rc; ed_entry_done(&rc, n, n && (!d_xG || !d_xH || !d_vG || !d_vH || !d_c),
                              "kyb_ed25519_dleq_challenge_dev: bad argument")) return rc;
    return launch_challenge(n, d_xG, d_xH, d_vG, d_vH, d_c, d_status, (hipStream_t)stream);
}

int kyb_ed25519_dleq_challenge(size_t n, const uint8_t* xG, const uint8_t* xH, const uint8_t* vG, const uint8_t* vH, uint8_t* c,
                               uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n, n && (!xG || !xH || !vG || !vH || !c), "kyb_ed25519_dleq_challenge: bad argument")) return rc;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return kyb_ed25519_dleq_challenge(hi - lo, xG + 32 * lo, xH + 32 * lo, vG + 32 * lo, vH + 32 * lo, c + 32 * lo,
                                              status ? status + lo : nullptr);
        });
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx, {{xG, n * 32}, {xH, n * 32}, {vG, n * 32}, {vH, n * 32}}, {{c, n * 32}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_challenge(n, in[0], in[1], in[2], in[3], o[0], o[1], st);
                       });
}

int kyb_ed25519_dleq_verify_dev(size_t n, const void* d_G, size_t g_stride, const void* d_H, size_t h_stride, const void* d_xG,
                                const void* d_xH, const void* d_C, const void* d_R, const void* d_VG, const void* d_VH,
                                const void* d_expect_c, void* d_ok, void* d_status, uint32_t flags, void* stream) {
    const DleqArgs a{d_G, d_H, d_xG, d_xH, d_C, d_R, d_VG, d_VH, d_expect_c, g_stride, h_stride, d_ok, d_status, flags};
    if (int rc; ed_entry_done(&rc, n, verify_args_bad(n, a), "kyb_ed25519_dleq_verify_dev: bad argument")) return rc;
    return launch_verify(n, a, (hipStream_t)stream);
}

int kyb_ed25519_dleq_verify(size_t n, const uint8_t* G, size_t g_stride, const uint8_t* H, size_t h_stride, const uint8_t* xG,
                            const uint8_t* xH, const uint8_t* C, const uint8_t* R, const uint8_t* VG, const uint8_t* VH,
                            const uint8_t* expect_c, uint8_t* ok, uint8_t* status, uint32_t flags) {
    const DleqArgs a{G, H, xG, xH, C, R, VG, VH, expect_c, g_stride, h_stride, ok, status, flags};
    if (int rc; ed_entry_done(&rc, n, verify_args_bad(n, a), "kyb_ed25519_dleq_verify: bad argument")) return rc;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {  // a shared base goes to every shard
            return kyb_ed25519_dleq_verify(hi - lo, G + g_stride * lo, g_stride, H + h_stride * lo, h_stride, xG + 32 * lo,
                                           xH + 32 * lo, C + 32 * lo, R + 32 * lo, VG + 32 * lo, VH + 32 * lo, expect_c, ok + lo,
                                           status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx,
                       {{G, g_stride ? n * 32 : 32}, {H, h_stride ? n * 32 : 32}, {xG, n * 32}, {xH, n * 32}, {C, n * 32}, {R, n * 32},
                        {VG, n * 32}, {VH, n * 32}, {expect_c, 32, /*absent=*/!expect_c}},
                       {{ok, n}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_verify(n, DleqArgs{in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8],
                                                            g_stride, h_stride, o[0], o[1], flags}, st);
                       });
}
}
