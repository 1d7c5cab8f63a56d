// sign/dss on Ed25519: kernels for gfx950 + their C-ABI entry points.  The lane programs are ed25519_dss.cuh's; this unit
// is their kernels' own, so that the other Ed25519 units keep their kernels and their register allocation (DESIGN.md
// section 5 items 41-42).
//
// Replaces, in the reference:
//   hashSig and sessionID     dss.go:201-211, 235-246  -> ed25519_dss_session_kernel
//   ProcessPartialSig         dss.go:141-173           -> ed25519_dss_fold_kernel, ed25519_dss_encode_kernel,
//                                                         ed25519_dss_fold_decode_kernel (per session),
//                                                         ed25519_dss_verify_kernel, ed25519_dss_verify_encode_kernel,
//                                                         ed25519_dss_share_kernel (per partial signature)
//   PartialSig                dss.go:113-134           -> ed25519_dss_partial_points_kernel, ed25519_dss_encode_kernel,
//                                                         ed25519_dss_partial_sign_kernel
// A check is four passes per session and three per partial signature.  The session passes hash, fold the commitments
// D_{b,k} = R_{b,k} + h_b A_k on the nine-limb ladder (window tables in the slab) and leave them, through the
// shared-inversion encoder and the decoder of the deal checks, as mixed-addition operands in the workspace; the partial passes run in
// pieces of ED_PIECE lanes: the signature's T parked, its verdict taken in the encoder, then the session id and the share
// check of ed25519_dkg.cuh against the folded polynomial.  Every call runs on the current device: none shards over a
// device set.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_dss.cuh"
#include "ed25519_launch.h"

#include <vector>

namespace kyb {

static_assert(ED_ST_DSS_INDEX == KYB_ST_DSS_INDEX && ED_ST_DSS_SIG == KYB_ST_DSS_SIG && ED_ST_DSS_SESSION == KYB_ST_DSS_SESSION &&
                  ED_ST_DSS_PARTIAL == KYB_ST_DSS_PARTIAL && ED_ST_BAD_POINT == KYB_ST_BAD_POINT,
              "status values of include/kyber_hip.h");

// ed25519_dss_fold_kernel: a lane's window table and its parked D; ed25519_dss_verify_kernel: the table of -A, T parked,
// the status; ed25519_dss_partial_points_kernel: a parked point.  Lanes past n leave before their tables.
constexpr EdSlabDesc ED_SLAB_DSS_FOLD{1, 1, false, false};
constexpr EdSlabDesc ED_SLAB_DSS_VERIFY{1, 1, true, false};
constexpr EdSlabDesc ED_SLAB_DSS_PARTIAL{0, 1, false, false};
static_assert(ed_slab_bytes(ED_SLAB_DSS_VERIFY, ED_PIECE) == ED_PIECE * (1280 + 120 + 1) + 256, "367 MB per stream");

// One lane per session: hs[b] = h_b, sids[b] = the session id
__global__ __launch_bounds__(64, 3) void ed25519_dss_session_kernel(size_t ns, const uint32_t* __restrict__ lc, size_t tl,
                                                                     const uint32_t* __restrict__ rc, size_t tr,
                                                                     const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                                                     sf::Mod m, uint32_t* __restrict__ hs, uint32_t* __restrict__ sids) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ns) return;
    uint32_t hw[8], sid[8];
    ed_dss_session_lane(hw, sid, lc, tl, rc + b * tr * 8, tr, msgs + off[b], (size_t)element_len(off, b), m);
    store_words8(hs + b * 8, hw);
    store_words8(sids + b * 8, sid);
}

// One lane per folded commitment: lane first + i is (session b, coefficient k) = ((first + i) / T, (first + i) % T) and
// parks D_{b,k} = R_{b,k} + h_b A_k; a term its polynomial does not have is the identity.  A commitment that does not
// decode marks its session (every lane that stores there stores the same value).
__global__ __launch_bounds__(128, 3) void ed25519_dss_fold_kernel(size_t n, size_t first, size_t T, const uint32_t* __restrict__ lc,
                                                                   size_t tl, const uint32_t* __restrict__ rc, size_t tr,
                                                                   const uint32_t* __restrict__ hs, int32_t* __restrict__ proj,
                                                                   uint8_t* __restrict__ bad, uint8_t* __restrict__ sess_status,
                                                                   int4* __restrict__ gtab) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t b = (first + i) / T, k = (first + i) % T;
    uint32_t hw[8], rw[8] = {1, 0, 0, 0, 0, 0, 0, 0}, aw[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    load_words8(hw, hs + b * 8);
    if (k < tr) load_words8(rw, rc + (b * tr + k) * 8);
    if (k < tl) load_words8(aw, lc + k * 8);
    DssTab tab{gtab + i * ED_TAB_INT4};
    ge29_p3 D;
    if (!ed_dss_fold_lane(D, hw, rw, aw, tab)) {
        bad[b] = 1;
        if (sess_status) sess_status[b] = KYB_ST_BAD_POINT;
    }
    store_proj(proj, i, D);
}

// The encodings of a piece's parked points (the folded D's of a check, A and the nonce points of a PartialSig call), one
// inversion per ENC_CHUNK points: enc[i], eight words a point
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_dss_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                        uint32_t* __restrict__ enc) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) { store_words8(enc + i * 8, w); });
}

// One lane per folded commitment: aff[i] = the share check's mixed-addition operand (y + x, y - x, 2dxy) of D_i, through
// the decoder of ed25519_dkg.cuh (an encoding the encoder wrote always decodes)
__global__ __launch_bounds__(64, 3) void ed25519_dss_fold_decode_kernel(size_t n, const uint32_t* __restrict__ enc,
                                                                         ge_precomp* __restrict__ aff) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[8];
    load_words8(w, enc + i * 8);
    ge_precomp a;
    ed_deal_decode(a, w);
    aff[i] = a;
}

// One lane per partial signature: the index, the bytes signed, T = S B - h A parked.  An index outside the roster or a
// session outside the call reads nothing else of the element.
__global__ __launch_bounds__(128, 3) void ed25519_dss_verify_kernel(size_t n, size_t np, size_t ns, const uint32_t* __restrict__ pubs,
                                                                     const uint32_t* __restrict__ sess, const uint32_t* __restrict__ idx,
                                                                     const uint32_t* __restrict__ V, const uint32_t* __restrict__ sid,
                                                                     const uint32_t* __restrict__ sigs, const int32_t* __restrict__ wide,
                                                                     sf::Mod m, int32_t* __restrict__ proj, uint8_t* __restrict__ st,
                                                                     int4* __restrict__ gtab) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t I = idx[i];
    ge_p3 T;
    if (sess[i] >= ns || I >= np) {
        ge_p3_0(T);
        store_proj(proj, i, T);
        st[i] = sess[i] >= ns ? 0xff : KYB_ST_DSS_INDEX;
        return;
    }
    uint32_t vw[8], sw[8], mw[8];
    load_words8(vw, V + i * 8);
    load_words8(sw, sid + i * 8);
    ed_dss_partial_hash(mw, vw, I, sw);
    uint32_t aw[8], rw[8];
    load_words8(aw, pubs + (size_t)I * 8);
    load_words8(rw, sigs + i * 16);
    load_words8(sw, sigs + i * 16 + 8);
    DssTab tab{gtab + i * ED_TAB_INT4};
    const int s = ed_dss_verify_lane(T, rw, sw, aw, mw, wide, m, tab);
    store_proj(proj, i, T);
    st[i] = (uint8_t)s;
}

// The signature's verdict, one inversion per ENC_CHUNK signatures: st[i] becomes KYB_ST_DSS_SIG where the checks passed
// and encode(T_i) != R_i
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_dss_verify_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                               const uint32_t* __restrict__ sigs,
                                                                                               uint8_t* __restrict__ st) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        if (st[i] != KYB_ST_OK) return;
        uint32_t r[8];
        load_words8(r, sigs + i * 16);
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) diff |= r[k] ^ w[k];
        if (diff) st[i] = KYB_ST_DSS_SIG;
    });
}

// One lane per partial signature: the session id, then V B against the folded polynomial of its session
__global__ __launch_bounds__(64, 3) void ed25519_dss_share_kernel(size_t n, size_t T, const uint32_t* __restrict__ sess,
                                                                   const uint32_t* __restrict__ idx, const uint32_t* __restrict__ V,
                                                                   const uint32_t* __restrict__ sid, const uint32_t* __restrict__ sids,
                                                                   const ge_precomp* __restrict__ aff, const uint8_t* __restrict__ bad,
                                                                   const uint8_t* __restrict__ st, const int32_t* __restrict__ wide,
                                                                   uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = st[i];
    if (s == 0xff) {  // a session the call does not hold: nothing read
        ok[i] = 0;
        if (status) status[i] = KYB_ST_OK;
        return;
    }
    if (s == KYB_ST_OK) {
        const size_t b = sess[i];
        uint32_t vw[8], sw[8], ew[8];
        load_words8(vw, V + i * 8);
        load_words8(sw, sid + i * 8);
        load_words8(ew, sids + b * 8);
        s = ed_dss_share_element(s, sw, ew, bad[b] != 0, vw, aff + b * T, T, idx[i], wide);
    }
    ok[i] = s == KYB_ST_OK ? 1 : 0;
    if (status) status[i] = (uint8_t)s;
}

// Lane first + i of a PartialSig call: element 0 is the signer's key A = priv B, element 1 + b the nonce point k_b B
__global__ __launch_bounds__(128, 3) void ed25519_dss_partial_points_kernel(size_t n, size_t first, const uint32_t* __restrict__ priv,
                                                                             const uint32_t* __restrict__ k,
                                                                             const int32_t* __restrict__ wide, int32_t* __restrict__ proj) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t g = first + i;
    uint32_t sw[8];
    load_words8(sw, g ? k + (g - 1) * 8 : priv);
    int8_t e[65];
    recode16(e, sw, false);
    ge_p3 R;
    ed_comb_mul_base(R, e, wide);
    store_proj(proj, i, R);
}

// One lane per session: V_b, the bytes signed, sig_b = R_b || k_b + SHA-512(R_b || A || m_b) priv.  enc: A's encoding, then
// the sessions' R
__global__ __launch_bounds__(128, 3) void ed25519_dss_partial_sign_kernel(size_t ns, uint32_t index, const uint32_t* __restrict__ priv,
                                                                           const uint32_t* __restrict__ alpha,
                                                                           const uint32_t* __restrict__ beta, const uint32_t* __restrict__ k,
                                                                           const uint32_t* __restrict__ hs, const uint32_t* __restrict__ sids,
                                                                           const uint32_t* __restrict__ enc, sf::Mod m,
                                                                           uint32_t* __restrict__ V, uint32_t* __restrict__ sigs) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ns) return;
    uint32_t hw[8], aw[8], bw[8], sw[8], vw[8], mw[8];
    load_words8(hw, hs + b * 8);
    load_words8(aw, alpha);
    load_words8(bw, beta + b * 8);
    load_words8(sw, sids + b * 8);
    ed_dss_partial_value(vw, mw, hw, aw, bw, index, sw, m);
    store_words8(V + b * 8, vw);
    uint32_t rw[8], kw[8], xw[8], sig[16];
    load_words8(aw, enc);
    load_words8(rw, enc + (1 + b) * 8);
    load_words8(kw, k + b * 8);
    load_words8(xw, priv);
    ed_dss_partial_sign(sig, rw, aw, kw, xw, mw, m);
    store_words8(sigs + b * 16, sig);
    store_words8(sigs + b * 16 + 8, sig + 8);
}

struct DssCheckArgs {
    size_t np;
    const void *participants;
    size_t tl;
    const void* long_commits;
    size_t ns, tr;
    const void *rand_commits, *msgs, *off, *sess, *idx, *V, *sid, *sigs;
    void *ok, *status, *sess_status;
};
struct DssPartialArgs {
    size_t ns;
    const void* priv;
    uint32_t index;
    const void *alpha, *beta, *k;
    size_t tl;
    const void* long_commits;
    size_t tr;
    const void *rand_commits, *msgs, *off;
    void *V, *sid, *sigs;
};

constexpr size_t DSS_MAX_COMMITS = size_t(1) << 31;
static size_t round256(size_t x) { return (x + 255) / 256 * 256; }
static bool dss_commits_too_many(size_t ns, size_t tl, size_t tr) {
    const size_t T = std::max(tl, tr);
    return tl > DSS_MAX_COMMITS || tr > DSS_MAX_COMMITS || ns > DSS_MAX_COMMITS / T;
}

// The (WS_ED_DSS, stream) workspace of a check:  [ h: ns x 32 B | session ids: ns x 32 B | per-session flags, ns bytes
// rounded up to 256, + 256 | the folded commitments' encodings: ns T x 32 B | ... decoded: ns T x 120 B ]
static int launch_dss_check(size_t n, const DssCheckArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    if (dss_commits_too_many(a.ns, a.tl, a.tr)) {
        set_error("kyb_ed25519_dss_check: ns * max(tl, tr) commitments do not fit the workspace");
        return KYB_E_ALLOC;
    }
    const size_t T = std::max(a.tl, a.tr), count = a.ns * T, flag_bytes = round256(a.ns) + 256;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the workspace, the slab and their kernels as one unit
    void* ws;
    if ((rc = ctx_workspace(ctx, WS_ED_DSS, st, a.ns * 64 + flag_bytes + count * (32 + sizeof(ge_precomp)), &ws))) return rc;
    uint32_t* hs = (uint32_t*)ws;
    uint32_t* sids = hs + a.ns * 8;
    uint8_t* bad = (uint8_t*)(sids + a.ns * 8);
    uint32_t* enc = (uint32_t*)(bad + flag_bytes);
    ge_precomp* aff = (ge_precomp*)(enc + count * 8);
    KYB_HIP_CHECK(hipMemsetAsync(bad, 0, flag_bytes, st));
    if (a.sess_status) KYB_HIP_CHECK(hipMemsetAsync(a.sess_status, 0, a.ns, st));
    hipLaunchKernelGGL(ed25519_dss_session_kernel, ed_grid(a.ns, 64), dim3(64), 0, st, a.ns,
                       (const uint32_t*)a.long_commits, a.tl, (const uint32_t*)a.rand_commits, a.tr, (const uint8_t*)a.msgs,
                       (const uint64_t*)a.off, ed_order(), hs, sids);
    KYB_HIP_CHECK(hipGetLastError());
    rc = ed_for_pieces(count, st, ED_SLAB_DSS_FOLD, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_dss_fold_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt, lo, T,
                           (const uint32_t*)a.long_commits, a.tl, (const uint32_t*)a.rand_commits, a.tr, (const uint32_t*)hs, w.proj, bad,
                           (uint8_t*)a.sess_status, w.gtab);
        hipLaunchKernelGGL(ed25519_dss_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt, (const int32_t*)w.proj,
                           enc + lo * 8);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(ed25519_dss_fold_decode_kernel, ed_grid(count, 64), dim3(64), 0, st, count, (const uint32_t*)enc,
                       aff);
    KYB_HIP_CHECK(hipGetLastError());
    return ed_for_pieces(n, st, ED_SLAB_DSS_VERIFY, [&](DeviceCtx* c, size_t lo, size_t cnt, const EdSlab& w) {
        const uint32_t *sess = (const uint32_t*)a.sess + lo, *idx = (const uint32_t*)a.idx + lo, *V = (const uint32_t*)a.V + lo * 8,
                       *sid = (const uint32_t*)a.sid + lo * 8, *sigs = (const uint32_t*)a.sigs + lo * 16;
        hipLaunchKernelGGL(ed25519_dss_verify_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt, a.np, a.ns,
                           (const uint32_t*)a.participants, sess, idx, V, sid, sigs, (const int32_t*)c->ed_wide_tab, ed_order(), w.proj,
                           w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_dss_verify_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt, (const int32_t*)w.proj,
                           sigs, w.status);
        hipLaunchKernelGGL(ed25519_dss_share_kernel, ed_grid(cnt, 64), dim3(64), 0, st, cnt, T, sess, idx, V, sid,
                           (const uint32_t*)sids, (const ge_precomp*)aff, (const uint8_t*)bad, (const uint8_t*)w.status,
                           (const int32_t*)c->ed_wide_tab, (uint8_t*)a.ok + lo, a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

// The (WS_ED_DSS, stream) workspace of a PartialSig call:  [ h: ns x 32 B | encodings: A, then ns nonce points, 32 B each ]
static int launch_dss_partial(const DssPartialArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    void* ws;
    if ((rc = ctx_workspace(ctx, WS_ED_DSS, st, a.ns * 32 + (a.ns + 1) * 32, &ws))) return rc;
    uint32_t* hs = (uint32_t*)ws;
    uint32_t* enc = hs + a.ns * 8;
    hipLaunchKernelGGL(ed25519_dss_session_kernel, ed_grid(a.ns, 64), dim3(64), 0, st, a.ns,
                       (const uint32_t*)a.long_commits, a.tl, (const uint32_t*)a.rand_commits, a.tr, (const uint8_t*)a.msgs,
                       (const uint64_t*)a.off, ed_order(), hs, (uint32_t*)a.sid);
    KYB_HIP_CHECK(hipGetLastError());
    rc = ed_for_pieces(a.ns + 1, st, ED_SLAB_DSS_PARTIAL, [&](DeviceCtx* c, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_dss_partial_points_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt, lo,
                           (const uint32_t*)a.priv, (const uint32_t*)a.k, (const int32_t*)c->ed_wide_tab, w.proj);
        hipLaunchKernelGGL(ed25519_dss_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt, (const int32_t*)w.proj,
                           enc + lo * 8);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(ed25519_dss_partial_sign_kernel, ed_grid(a.ns, 128), dim3(128), 0, st, a.ns, a.index,
                       (const uint32_t*)a.priv, (const uint32_t*)a.alpha, (const uint32_t*)a.beta, (const uint32_t*)a.k, (const uint32_t*)hs,
                       (const uint32_t*)a.sid, (const uint32_t*)enc, ed_order(), (uint32_t*)a.V, (uint32_t*)a.sigs);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}

static bool dss_check_args_bad(size_t n, const DssCheckArgs& a) {
    return n && (!a.participants || !a.long_commits || !a.rand_commits || !a.off || !a.sess || !a.idx || !a.V || !a.sid || !a.sigs ||
                 !a.ok || a.tl == 0 || a.tr == 0 || a.ns == 0);
}
static bool dss_partial_args_bad(const DssPartialArgs& a) {
    return a.ns && (!a.priv || !a.alpha || !a.beta || !a.k || !a.long_commits || !a.rand_commits || !a.off || !a.V || !a.sid ||
                    !a.sigs || a.tl == 0 || a.tr == 0);
}

}  // namespace kyb

using namespace kyb;

extern "C" {

// ProcessPartialSig (dss.go:141-173) without its sequential state, for n partial signatures over ns sessions
int kyb_ed25519_dss_check_dev(size_t n, size_t np, const void* d_participants, size_t tl, const void* d_long_commits, size_t ns,
                              size_t tr, const void* d_rand_commits, const void* d_msgs, const void* d_msg_off, const void* d_sess,
                              const void* d_idx, const void* d_V, const void* d_sid, const void* d_sigs, void* d_ok, void* d_status,
                              void* d_sess_status, void* stream) {
    const DssCheckArgs a{np, d_participants, tl, d_long_commits, ns, tr, d_rand_commits, d_msgs, d_msg_off, d_sess, d_idx, d_V, d_sid,
                         d_sigs, d_ok, d_status, d_sess_status};
    if (int rc; ed_entry_done(&rc, n, dss_check_args_bad(n, a), "kyb_ed25519_dss_check_dev: bad argument")) return rc;
    return launch_dss_check(n, a, (hipStream_t)stream);
}

int kyb_ed25519_dss_check(size_t n, size_t np, const uint8_t* participants, size_t tl, const uint8_t* long_commits, size_t ns,
                          size_t tr, const uint8_t* rand_commits, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* sess,
                          const uint32_t* idx, const uint8_t* V, const uint8_t* sid, const uint8_t* sigs, uint8_t* ok, uint8_t* status,
                          uint8_t* sess_status) {
    const DssCheckArgs a{np, participants, tl, long_commits, ns, tr, rand_commits, msgs, msg_off, sess, idx, V, sid, sigs, ok, status,
                         sess_status};
    if (int rc; ed_entry_done(&rc, n, dss_check_args_bad(n, a),
                              "kyb_ed25519_dss_check: bad argument (pointers; tl, tr and ns at least 1)")) return rc;
    if (dss_commits_too_many(ns, tl, tr)) {  // (before the ns + 1 offsets are walked)
        set_error("kyb_ed25519_dss_check: ns * max(tl, tr) commitments do not fit the workspace");
        return KYB_E_ALLOC;
    }
    if (EdHostSpans::offsets_bad(ns, msgs, msg_off)) {
        set_error("kyb_ed25519_dss_check: bad argument (offsets that do not decrease; bytes named only where msgs is given)");
        return KYB_E_ARG;
    }
    for (size_t i = 0; i < n; i++)
        if (sess[i] >= ns) {
            set_error("kyb_ed25519_dss_check: bad argument (a partial signature names a session the call does not hold)");
            return KYB_E_ARG;
        }
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(ns, msgs, msg_off);
    // the roster and the long-term commitments travel as one buffer: twelve staging buffers a call, outputs included
    std::vector<uint8_t> keys((np + tl) * 32);
    memcpy(keys.data(), participants, np * 32);
    memcpy(keys.data() + np * 32, long_commits, tl * 32);
    return staged_call(ctx,
                       {{keys.data(), keys.size()}, {rand_commits, ns * tr * 32}, {sp.base, sp.total},
                        {sp.offsets(), sp.offsets_bytes()}, {sess, n * 4}, {idx, n * 4}, {V, n * 32}, {sid, n * 32}, {sigs, n * 64}},
                       {{ok, n}, {status, n}, {sess_status, ns, /*slack=*/1}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_dss_check(n,
                                                   DssCheckArgs{np, in[0], tl, (const uint8_t*)in[0] + np * 32, ns, tr, in[1], in[2], in[3],
                                                                in[4], in[5], in[6], in[7], in[8], o[0], o[1], o[2]},
                                                   st);
                       });
}

// PartialSig (dss.go:113-134) for ns sessions of one signer
int kyb_ed25519_dss_partial_dev(size_t ns, const void* d_priv, uint32_t index, const void* d_alpha, const void* d_beta, const void* d_k,
                                size_t tl, const void* d_long_commits, size_t tr, const void* d_rand_commits, const void* d_msgs,
                                const void* d_msg_off, void* d_V, void* d_sid, void* d_sigs, void* stream) {
    const DssPartialArgs a{ns, d_priv, index, d_alpha, d_beta, d_k, tl, d_long_commits, tr, d_rand_commits, d_msgs, d_msg_off, d_V, d_sid,
                           d_sigs};
    if (int rc; ed_entry_done(&rc, ns, dss_partial_args_bad(a), "kyb_ed25519_dss_partial_dev: bad argument")) return rc;
    if (dss_commits_too_many(ns, tl, tr)) {
        set_error("kyb_ed25519_dss_partial_dev: ns * max(tl, tr) commitments do not fit a call");
        return KYB_E_ALLOC;
    }
    return launch_dss_partial(a, (hipStream_t)stream);
}

int kyb_ed25519_dss_partial(size_t ns, const uint8_t* priv, uint32_t index, const uint8_t* alpha, const uint8_t* beta, const uint8_t* k,
                            size_t tl, const uint8_t* long_commits, size_t tr, const uint8_t* rand_commits, const uint8_t* msgs,
                            const uint64_t* msg_off, uint8_t* V, uint8_t* sid, uint8_t* sigs) {
    const DssPartialArgs a{ns, priv, index, alpha, beta, k, tl, long_commits, tr, rand_commits, msgs, msg_off, V, sid, sigs};
    if (int rc; ed_entry_done(&rc, ns, dss_partial_args_bad(a),
                              "kyb_ed25519_dss_partial: bad argument (pointers; tl and tr at least 1)")) return rc;
    if (dss_commits_too_many(ns, tl, tr)) {
        set_error("kyb_ed25519_dss_partial: ns * max(tl, tr) commitments do not fit a call");
        return KYB_E_ALLOC;
    }
    if (EdHostSpans::offsets_bad(ns, msgs, msg_off)) {
        set_error("kyb_ed25519_dss_partial: bad argument (offsets that do not decrease; bytes named only where msgs is given)");
        return KYB_E_ARG;
    }
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(ns, msgs, msg_off);
    return staged_call(ctx,
                       {{priv, 32}, {alpha, 32}, {beta, ns * 32}, {k, ns * 32}, {long_commits, tl * 32}, {rand_commits, ns * tr * 32},
                        {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{V, ns * 32}, {sid, ns * 32}, {sigs, ns * 64}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_dss_partial(DssPartialArgs{ns, in[0], index, in[1], in[2], in[3], tl, in[4], tr, in[5], in[6], in[7],
                                                                    o[0], o[1], o[2]},
                                                     st);
                       });
}
}
