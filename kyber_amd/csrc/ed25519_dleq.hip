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
// verdict is taken.  Batches run in pieces of ED_PIECE lanes, so the per-stream slab is bounded whatever n is.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_dleq.cuh"

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_DLEQ_CHALLENGE == KYB_ST_DLEQ_CHALLENGE &&
                  ED_ST_PICK_EXHAUSTED == KYB_ST_PICK_EXHAUSTED,
              "status values of include/kyber_hip.h");

// Lanes per piece, as in ed25519_verify.hip: enough waves to fill the device at three per SIMD, and a slab of at most
// 2^18 x (2 560 + 240 + 1) B = 734 MB per stream.
constexpr size_t ED_PIECE = size_t(1) << 18;

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
// points.  A lane's chunk starts at an even index and is walked downwards, so it meets b_i just before a_i.
__global__ __launch_bounds__(64, KYB_TU_WAVES) void ed25519_dleq_encode_kernel(
    size_t n, const int32_t* __restrict__ proj, const uint8_t* __restrict__ st, const uint32_t* __restrict__ VG,
    const uint32_t* __restrict__ VH, uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    static_assert(ENC_CHUNK % 2 == 0, "a and b of one proof share a chunk");
    bool b_same = false;
    ed_encode_chunk(2 * n, proj, (size_t)blockIdx.x * blockDim.x + threadIdx.x, [&](size_t i, uint32_t(&w)[8]) {
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

// the (WS_ED, stream) slab of one piece: [ window tables: cnt x 2 560 B | (X, Y, Z) of a and b: cnt x 240 B | status: cnt ]
static int piece_workspace(DeviceCtx* ctx, hipStream_t st, size_t cnt, int4** gtab, int32_t** proj, uint8_t** status) {
    cnt = (cnt + 127) / 128 * 128;  // the lanes past n of the last block keep their table writes inside the slab
    void* base;
    const int rc = ctx_workspace(ctx, WS_ED, st, cnt * (2560 + 60 * sizeof(int32_t) + 1) + 256, &base);
    if (rc) return rc;
    *gtab = (int4*)base;
    *proj = (int32_t*)((uint8_t*)base + cnt * 2560);
    *status = (uint8_t*)base + cnt * (2560 + 60 * sizeof(int32_t));
    return KYB_OK;
}

static int launch_challenge(size_t n, const void* xG, const void* xH, const void* vG, const void* vH, void* c, void* status,
                            hipStream_t st) {
    DeviceCtx* ctx;
    const int rc = get_ctx(&ctx);
    if (rc) return rc;
    for (size_t lo = 0; lo < n; lo += ED_PIECE) {
        const size_t cnt = std::min(ED_PIECE, n - lo);
        hipLaunchKernelGGL(ed25519_dleq_challenge_kernel, dim3((unsigned)((cnt + 127) / 128)), dim3(128), 0, st, cnt,
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
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // context.h: the slab + its kernels as one unit
    const size_t gs = a.g_stride / 4, hs = a.h_stride / 4;
    for (size_t lo = 0; lo < n; lo += ED_PIECE) {
        const size_t cnt = std::min(ED_PIECE, n - lo);
        int4* gtab;
        int32_t* proj;
        uint8_t* stat;
        if ((rc = piece_workspace(ctx, st, std::min(ED_PIECE, n), &gtab, &proj, &stat))) return rc;
        const uint32_t *VG = (const uint32_t*)a.VG + lo * 8, *VH = (const uint32_t*)a.VH + lo * 8;
        hipLaunchKernelGGL(ed25519_dleq_kernel, dim3((unsigned)((cnt + 127) / 128)), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.G + lo * gs, gs, (const uint32_t*)a.H + lo * hs, hs,
                           (const uint32_t*)a.xG + lo * 8, (const uint32_t*)a.xH + lo * 8, (const uint32_t*)a.C + lo * 8,
                           (const uint32_t*)a.R + lo * 8, VG, VH, (const uint32_t*)a.expect, a.flags, proj, stat, gtab);
        const size_t lanes = (2 * cnt + ENC_CHUNK - 1) / ENC_CHUNK;
        hipLaunchKernelGGL(ed25519_dleq_encode_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, cnt,
                           (const int32_t*)proj, (const uint8_t*)stat, VG, VH, (uint8_t*)a.ok + lo,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
        KYB_HIP_CHECK(hipGetLastError());
    }
    return KYB_OK;
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
    if (n && (!d_xG || !d_xH || !d_vG || !d_vH || !d_c)) {
        set_error("kyb_ed25519_dleq_challenge_dev: bad argument");
        return KYB_E_ARG;
    }
    if (n == 0) return KYB_OK;
    return launch_challenge(n, d_xG, d_xH, d_vG, d_vH, d_c, d_status, (hipStream_t)stream);
}

int kyb_ed25519_dleq_challenge(size_t n, const uint8_t* xG, const uint8_t* xH, const uint8_t* vG, const uint8_t* vH, uint8_t* c,
                               uint8_t* status) {
    if (n && (!xG || !xH || !vG || !vH || !c)) {
        set_error("kyb_ed25519_dleq_challenge: bad argument");
        return KYB_E_ARG;
    }
    if (n == 0) return KYB_OK;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return kyb_ed25519_dleq_challenge(hi - lo, xG + 32 * lo, xH + 32 * lo, vG + 32 * lo, vH + 32 * lo, c + 32 * lo,
                                              status ? status + lo : nullptr);
        });
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    StageScope sc_(ctx);
    StageBuf d_a, d_b, d_u, d_v, d_c, d_st;
    rc = d_a.upload(xG, n * 32);
    if (rc == KYB_OK) rc = d_b.upload(xH, n * 32);
    if (rc == KYB_OK) rc = d_u.upload(vG, n * 32);
    if (rc == KYB_OK) rc = d_v.upload(vH, n * 32);
    if (rc == KYB_OK) rc = d_c.alloc(n * 32);
    if (rc == KYB_OK) rc = d_st.alloc(n);
    if (rc == KYB_OK) rc = launch_challenge(n, d_a.p, d_b.p, d_u.p, d_v.p, d_c.p, d_st.p, sc_.stream());
    if (rc == KYB_OK) rc = d_c.download(c, n * 32);
    if (rc == KYB_OK && status) rc = d_st.download(status, n);
    return rc;
}

int kyb_ed25519_dleq_verify_dev(size_t n, const void* d_G, size_t g_stride, const void* d_H, size_t h_stride, const void* d_xG,
                                const void* d_xH, const void* d_C, const void* d_R, const void* d_VG, const void* d_VH,
                                const void* d_expect_c, void* d_ok, void* d_status, uint32_t flags, void* stream) {
    const DleqArgs a{d_G, d_H, d_xG, d_xH, d_C, d_R, d_VG, d_VH, d_expect_c, g_stride, h_stride, d_ok, d_status, flags};
    if (verify_args_bad(n, a)) {
        set_error("kyb_ed25519_dleq_verify_dev: bad argument");
        return KYB_E_ARG;
    }
    if (n == 0) return KYB_OK;
    return launch_verify(n, a, (hipStream_t)stream);
}

int kyb_ed25519_dleq_verify(size_t n, const uint8_t* G, size_t g_stride, const uint8_t* H, size_t h_stride, const uint8_t* xG,
                            const uint8_t* xH, const uint8_t* C, const uint8_t* R, const uint8_t* VG, const uint8_t* VH,
                            const uint8_t* expect_c, uint8_t* ok, uint8_t* status, uint32_t flags) {
    if (verify_args_bad(n, DleqArgs{G, H, xG, xH, C, R, VG, VH, expect_c, g_stride, h_stride, ok, status, flags})) {
        set_error("kyb_ed25519_dleq_verify: bad argument");
        return KYB_E_ARG;
    }
    if (n == 0) return KYB_OK;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {  // a shared base goes to every shard
            return kyb_ed25519_dleq_verify(hi - lo, G + g_stride * lo, g_stride, H + h_stride * lo, h_stride, xG + 32 * lo,
                                           xH + 32 * lo, C + 32 * lo, R + 32 * lo, VG + 32 * lo, VH + 32 * lo, expect_c, ok + lo,
                                           status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    StageScope sc_(ctx);
    StageBuf d_G, d_H, d_xG, d_xH, d_C, d_R, d_VG, d_VH, d_e, d_ok, d_st;
    rc = d_G.upload(G, g_stride ? n * 32 : 32);
    if (rc == KYB_OK) rc = d_H.upload(H, h_stride ? n * 32 : 32);
    if (rc == KYB_OK) rc = d_xG.upload(xG, n * 32);
    if (rc == KYB_OK) rc = d_xH.upload(xH, n * 32);
    if (rc == KYB_OK) rc = d_C.upload(C, n * 32);
    if (rc == KYB_OK) rc = d_R.upload(R, n * 32);
    if (rc == KYB_OK) rc = d_VG.upload(VG, n * 32);
    if (rc == KYB_OK) rc = d_VH.upload(VH, n * 32);
    if (rc == KYB_OK && expect_c) rc = d_e.upload(expect_c, 32);
    if (rc == KYB_OK) rc = d_ok.alloc(n);
    if (rc == KYB_OK) rc = d_st.alloc(n);
    if (rc == KYB_OK)
        rc = launch_verify(n, DleqArgs{d_G.p, d_H.p, d_xG.p, d_xH.p, d_C.p, d_R.p, d_VG.p, d_VH.p, expect_c ? d_e.p : nullptr,
                                       g_stride, h_stride, d_ok.p, d_st.p, flags},
                           sc_.stream());
    if (rc == KYB_OK) rc = d_ok.download(ok, n);
    if (rc == KYB_OK && status) rc = d_st.download(status, n);
    return rc;
}
}
