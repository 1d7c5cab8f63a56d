// share/vss (Pedersen and Rabin) on Ed25519: kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_vss.cuh's; this unit is their kernels' own, so that the other Ed25519 units keep their kernels and their
// register allocation.
//
// Replaces, in the reference:
//   sign/schnorr Sign        schnorr.go:56-82   -> ed25519_schnorr_points_kernel, ed25519_schnorr_encode_kernel,
//                                                  ed25519_schnorr_sign_kernel
//   Dealer.EncryptedDeal     pedersen/vss.go:222-255, rabin/vss.go:263-297
//                                               -> ed25519_vss_seal_kernel, ed25519_vss_encode_kernel<3>, ed25519_vss_seal_aead_kernel
//   decryptDeal's second half   pedersen/vss.go:443-457
//                                               -> ed25519_vss_open_kernel, ed25519_vss_encode_kernel<1>, ed25519_vss_open_aead_kernel
//   Rabin's share check      rabin/vss.go:611-651 over share/poly.go:340-348
//                                               -> ed25519_vss_deal_decode_kernel, ed25519_vss_deal_check2_kernel
// A signature, a seal or an open is three launches per piece of ED_PIECE elements, as in ed25519_dkg.hip: the point
// pass parks (X, Y, Z); the shared-inversion encoder writes the points' bytes (a signature's two into the slab's digit
// field, a deal's into the front of the element's window table, dead by then); the last pass, one lane per element,
// hashes, signs and runs the AEAD.  LDS of the AEAD passes: the S-box (256 B) and the block's round keys (64 lanes x 60
// words) -- ED_AEAD_LDS_BYTES.  Every call runs on the current device: none shards over a device set.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_vss.cuh"
#include "ed25519_launch.h"

namespace kyb {

static_assert(ED_DKG_ST_OK == KYB_ST_OK && ED_DKG_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_ECIES_SHORT == KYB_ST_ECIES_SHORT &&
                  ED_ST_ECIES_AUTH == KYB_ST_ECIES_AUTH,
              "status values of include/kyber_hip.h");

// ------------------------------------------------------------------------------------------------ schnorr.Sign
// One lane per signature: R = k B and A = x B parked.  priv_stride: 8 words, or 0 for one signer.
__global__ __launch_bounds__(128, 3) void ed25519_schnorr_points_kernel(size_t n, const uint32_t* __restrict__ k,
                                                                         const uint32_t* __restrict__ privs, size_t priv_stride,
                                                                         const int32_t* __restrict__ wide, int32_t* __restrict__ proj) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t kw[8], xw[8];
    load_words8(kw, k + idx * 8);
    load_words8(xw, privs + idx * priv_stride);
    ge_p3 R, A;
    ed_schnorr_points_lane(R, A, kw, xw, wide);
    store_proj(proj, 2 * idx, R);
    store_proj(proj, 2 * idx + 1, A);
}

// The encodings of R and A, one inversion per ENC_CHUNK points, into the slab's digit field: 16 words an element
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_schnorr_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                            uint32_t* __restrict__ bytes) {
    EncPreScratch pre;
    ed_encode_chunk<2>(n, proj, ed_encode_first<2>(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) { store_words8(bytes + i * 8, w); });
}

// One lane per signature: h = SHA-512(R || A || msg) mod l, S = k + h x mod l, sig = R || S
__global__ __launch_bounds__(128, 3) void ed25519_schnorr_sign_kernel(size_t n, const uint32_t* __restrict__ k,
                                                                       const uint32_t* __restrict__ privs, size_t priv_stride,
                                                                       const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                                                       const uint32_t* __restrict__ bytes, sf::Mod m,
                                                                       uint32_t* __restrict__ sigs, uint8_t* __restrict__ status) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t kw[8], xw[8], rw[8], aw[8], sig[16];
    load_words8(kw, k + idx * 8);
    load_words8(xw, privs + idx * priv_stride);
    load_words8(rw, bytes + idx * 16);
    load_words8(aw, bytes + idx * 16 + 8);
    ed_schnorr_sign_element(sig, rw, aw, kw, xw, msgs + off[idx], (size_t)element_len(off, idx), m);
    store_words8(sigs + idx * 16, sig);
    store_words8(sigs + idx * 16 + 8, sig + 8);
    if (status) status[idx] = KYB_ST_OK;
}

// ---------------------------------------------------------------------------------------- EncryptedDeal / decryptDeal
// One lane per verifier; lanes past n leave before the table.  Parks DHKey = dh B, R = k B and pre = dh pub.
__global__ __launch_bounds__(128, 3) void ed25519_vss_seal_kernel(size_t n, const uint32_t* __restrict__ dh, const uint32_t* __restrict__ k,
                                                                   const uint32_t* __restrict__ pubs, const int32_t* __restrict__ wide,
                                                                   int32_t* __restrict__ proj, uint8_t* __restrict__ st,
                                                                   int4* __restrict__ gtab) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t sw[8], pw[8];
    load_words8(sw, dh + idx * 8);
    load_words8(pw, pubs + idx * 8);
    TabGlobal tab{gtab + idx * ED_TAB_INT4};
    int s;
    {
        ge_p3 K, D;
        s = ed_vss_seal_lane(K, D, sw, pw, wide, tab);
        store_proj(proj, 3 * idx, K);
        store_proj(proj, 3 * idx + 2, D);
    }
    load_words8(sw, k + idx * 8);
    ge_p3 R;
    ed_vss_seal_nonce_point(R, sw, s, wide);
    store_proj(proj, 3 * idx + 1, R);
    st[idx] = (uint8_t)s;
}

// priv_stride: 8 words, or 0 for one receiver.  Parks pre = x DHKey.
__global__ __launch_bounds__(128, 3) void ed25519_vss_open_kernel(size_t n, const uint32_t* __restrict__ privs, size_t priv_stride,
                                                                   const uint32_t* __restrict__ dhkeys, const uint64_t* __restrict__ off,
                                                                   int32_t* __restrict__ proj, uint8_t* __restrict__ st,
                                                                   int4* __restrict__ gtab) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t xw[8], kw[8];
    load_words8(xw, privs + idx * priv_stride);
    load_words8(kw, dhkeys + idx * 8);
    TabGlobal tab{gtab + idx * ED_TAB_INT4};
    ge_p3 D;
    const int s = ed_vss_open_lane(D, xw, kw, element_len(off, idx), tab);
    store_proj(proj, idx, D);
    st[idx] = (uint8_t)s;
}

// The encodings of an element's GROUP parked points, one inversion per lane, into the front of the element's window
// table: point k at word 8 k.  n: elements.  A lane owns ENC_CHUNK / GROUP elements.
template <int GROUP>
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_vss_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                        int4* __restrict__ gtab) {
    static_assert(GROUP * 32 <= (int)ED_TAB_BYTES, "the bytes fit the table they replace");
    EncPreScratch pre;
    ed_encode_chunk<GROUP>(n, proj, ed_encode_first<GROUP>(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        store_words8((uint32_t*)gtab + (i / GROUP) * ED_TAB_WORDS32 + (i % GROUP) * 8, w);
    });
}
template <int GROUP>
static dim3 vss_encode_grid(size_t n) {  // elements per block: ED_ENC_BLOCK lanes x ENC_CHUNK / GROUP
    const size_t span = size_t(ED_ENC_BLOCK) * (ENC_CHUNK / GROUP);
    return ed_grid(n, span);
}

// first: the batch index of the piece's element 0 (its cipher lies 16 bytes further for every element before it).
// ctx_stride: cwords words (the context's length, 8 or 32), or 0 for one context.
__global__ __launch_bounds__(ED_AEAD_BLOCK, KYB_TU_WAVES) void ed25519_vss_seal_aead_kernel(
    size_t n, size_t first, const uint32_t* __restrict__ k, const uint32_t* __restrict__ priv, const uint32_t* __restrict__ pub,
    const uint32_t* __restrict__ ctx, size_t ctx_stride, int cwords, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
    const int4* __restrict__ gtab, const uint8_t* __restrict__ st, sf::Mod m, uint32_t* __restrict__ dhkeys, uint32_t* __restrict__ sigs,
    uint8_t* __restrict__ ciphers, uint8_t* __restrict__ status) {
    __shared__ uint8_t sbox[256];
    __shared__ uint32_t keys[AesKeysLds<ED_AEAD_BLOCK>::WORDS];
    static_assert(sizeof(sbox) + sizeof(keys) == ED_AEAD_LDS_BYTES, "the layout the header of this file states");
    aes_fill_sbox(sbox, (int)threadIdx.x, (int)ED_AEAD_BLOCK);
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    AesKeysLds<ED_AEAD_BLOCK> rk{keys + threadIdx.x};
    uint32_t enc[24], kw[8], xw[8], aw[8], dhkey[8], sig[16];
    const uint32_t* front = (const uint32_t*)gtab + idx * ED_TAB_WORDS32;
    load_words8(enc, front);
    load_words8(enc + 8, front + 8);
    load_words8(enc + 16, front + 16);
    load_words8(kw, k + idx * 8);
    load_words8(xw, priv);
    load_words8(aw, pub);
    const uint32_t* cw = ctx + (first + idx) * ctx_stride;
    const int s = st[idx];
    ed_vss_seal_element(ciphers + off[idx] + VSS_OVERHEAD * (first + idx), dhkey, sig, msgs + off[idx], element_len(off, idx), enc, kw,
                        xw, aw, cw, cwords, s, m, rk, sbox);
    store_words8(dhkeys + idx * 8, dhkey);
    store_words8(sigs + idx * 16, sig);
    store_words8(sigs + idx * 16 + 8, sig + 8);
    if (status) status[idx] = (uint8_t)s;
}

__global__ __launch_bounds__(ED_AEAD_BLOCK, KYB_TU_WAVES) void ed25519_vss_open_aead_kernel(
    size_t n, size_t first, const uint32_t* __restrict__ ctx, size_t ctx_stride, int cwords, const uint8_t* __restrict__ ciphers,
    const uint64_t* __restrict__ off, const int4* __restrict__ gtab, const uint8_t* __restrict__ st, uint8_t* __restrict__ out,
    uint8_t* __restrict__ status) {
    __shared__ uint8_t sbox[256];
    __shared__ uint32_t keys[AesKeysLds<ED_AEAD_BLOCK>::WORDS];
    static_assert(sizeof(sbox) + sizeof(keys) == ED_AEAD_LDS_BYTES, "the layout the header of this file states");
    aes_fill_sbox(sbox, (int)threadIdx.x, (int)ED_AEAD_BLOCK);
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    AesKeysLds<ED_AEAD_BLOCK> rk{keys + threadIdx.x};
    uint32_t pre[8];
    load_words8(pre, (const uint32_t*)gtab + idx * ED_TAB_WORDS32);
    const int s = ed_vss_open_element(out + off[idx], ciphers + off[idx], element_len(off, idx), pre, ctx + (first + idx) * ctx_stride, cwords,
                                      st[idx], rk, sbox);
    if (status) status[idx] = (uint8_t)s;
}

// --------------------------------------------------------------------------------------------- Rabin's share check
// Lanes below `count`: one commitment each, aff[j] = its mixed-addition operand.  The nh lanes behind them: one H each,
// decoded and its window table parked at htab + 80 k.  A commitment or an H that does not decode marks its polynomial;
// the one H of a batch (nh = 1 < m) marks them all.
__global__ __launch_bounds__(64, 3) void ed25519_vss_deal_decode_kernel(size_t count, size_t m, size_t t, size_t nh,
                                                                         const uint32_t* __restrict__ commits,
                                                                         const uint32_t* __restrict__ H, ge_precomp* __restrict__ aff,
                                                                         int4* __restrict__ htab, uint8_t* __restrict__ bad,
                                                                         uint8_t* __restrict__ status) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count + nh) return;
    uint32_t w[8];
    if (j < count) {
        load_words8(w, commits + j * 8);
        ge_precomp a;
        const bool ok = ed_deal_decode(a, w);
        aff[j] = a;
        if (!ok) {  // (every lane that stores here stores the same value)
            bad[j / t] = 1;
            if (status) status[j / t] = KYB_ST_BAD_POINT;
        }
        return;
    }
    const size_t k = j - count;
    load_words8(w, H + k * 8);
    TabGlobal tab{htab + k * ED_TAB_INT4};
    if (ed_vss_htab(tab, w)) return;
    const size_t lo = nh == 1 ? 0 : k, hi = nh == 1 ? m : k + 1;
    for (size_t p = lo; p < hi; p++) {
        bad[p] = 1;
        if (status) status[p] = KYB_ST_BAD_POINT;
    }
}

// One lane per check.  A polynomial index outside the table reads nothing.  h_stride: 1 table per polynomial, or 0.
__global__ __launch_bounds__(64, 3) void ed25519_vss_deal_check2_kernel(size_t n, const uint32_t* __restrict__ poly,
                                                                         const uint32_t* __restrict__ idx, const uint32_t* __restrict__ f,
                                                                         const uint32_t* __restrict__ g, size_t m, size_t t,
                                                                         const ge_precomp* __restrict__ aff, const int4* __restrict__ htab,
                                                                         size_t h_stride, const uint8_t* __restrict__ bad,
                                                                         const int32_t* __restrict__ wide, uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t k = poly[i];
    if (k >= m || bad[k]) {
        ok[i] = 0;
        return;
    }
    uint32_t fw[8], gw[8];
    load_words8(fw, f + i * 8);
    load_words8(gw, g + i * 8);
    const TabGlobal tab{const_cast<int4*>(htab) + k * h_stride * ED_TAB_INT4};
    ok[i] = ed_deal_check2_lane(fw, gw, aff + k * t, t, idx[i], wide, tab) ? 1 : 0;
}

struct SignArgs {
    const void *k, *privs;
    size_t priv_stride;
    const void *msgs, *off;
    void *sigs, *status;
};
struct VssSealArgs {
    const void *dh, *k, *priv, *pub, *pubs, *ctx;
    size_t ctx_stride, ctx_len;
    const void *msgs, *off;
    void *dhkeys, *sigs, *ciphers, *status;
};
struct VssOpenArgs {
    const void* privs;
    size_t priv_stride;
    const void *dhkeys, *ctx;
    size_t ctx_stride, ctx_len;
    const void *ciphers, *off;
    void *out, *status;
};
struct Deal2Args {
    const void *poly, *idx, *f, *g;
    size_t m, t;
    const void *commits, *H;
    size_t h_stride;
    void *ok, *status;
};

static int launch_sign(size_t n, const SignArgs& a, hipStream_t st) {
    const size_t ps = a.priv_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_SCHNORR_SIGN, [&](DeviceCtx* ctx, size_t lo, size_t cnt, const EdSlab& w) {
        const dim3 lanes = ed_grid(cnt, 128);
        const uint32_t *k = (const uint32_t*)a.k + lo * 8, *x = (const uint32_t*)a.privs + lo * ps;
        hipLaunchKernelGGL(ed25519_schnorr_points_kernel, lanes, dim3(128), 0, st, cnt, k, x, ps, (const int32_t*)ctx->ed_wide_tab,
                           w.proj);
        hipLaunchKernelGGL(ed25519_schnorr_encode_kernel, ed_encode_grid(2 * cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, w.digits);
        hipLaunchKernelGGL(ed25519_schnorr_sign_kernel, lanes, dim3(128), 0, st, cnt, k, x, ps, (const uint8_t*)a.msgs,
                           (const uint64_t*)a.off + lo, (const uint32_t*)w.digits, ed_order(), (uint32_t*)a.sigs + lo * 16,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static int launch_vss_seal(size_t n, const VssSealArgs& a, hipStream_t st) {
    const size_t cs = a.ctx_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_VSS_SEAL, [&](DeviceCtx* ctx, size_t lo, size_t cnt, const EdSlab& w) {
        const uint32_t* k = (const uint32_t*)a.k + lo * 8;
        hipLaunchKernelGGL(ed25519_vss_seal_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.dh + lo * 8, k, (const uint32_t*)a.pubs + lo * 8, (const int32_t*)ctx->ed_wide_tab, w.proj,
                           w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_vss_encode_kernel<3>, vss_encode_grid<3>(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, w.gtab);
        hipLaunchKernelGGL(ed25519_vss_seal_aead_kernel, ed_grid(cnt, ED_AEAD_BLOCK),
                           dim3(ED_AEAD_BLOCK), 0, st, cnt, lo, k, (const uint32_t*)a.priv, (const uint32_t*)a.pub,
                           (const uint32_t*)a.ctx, cs, (int)(a.ctx_len / 4), (const uint8_t*)a.msgs, (const uint64_t*)a.off + lo, (const int4*)w.gtab,
                           (const uint8_t*)w.status, ed_order(), (uint32_t*)a.dhkeys + lo * 8, (uint32_t*)a.sigs + lo * 16,
                           (uint8_t*)a.ciphers, a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static int launch_vss_open(size_t n, const VssOpenArgs& a, hipStream_t st) {
    const size_t ps = a.priv_stride / 4, cs = a.ctx_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_VSS_OPEN, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_vss_open_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.privs + lo * ps, ps, (const uint32_t*)a.dhkeys + lo * 8, (const uint64_t*)a.off + lo,
                           w.proj, w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_vss_encode_kernel<1>, vss_encode_grid<1>(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, w.gtab);
        hipLaunchKernelGGL(ed25519_vss_open_aead_kernel, ed_grid(cnt, ED_AEAD_BLOCK),
                           dim3(ED_AEAD_BLOCK), 0, st, cnt, lo, (const uint32_t*)a.ctx, cs, (int)(a.ctx_len / 4), (const uint8_t*)a.ciphers,
                           (const uint64_t*)a.off + lo, (const int4*)w.gtab, (const uint8_t*)w.status, (uint8_t*)a.out,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

constexpr size_t DEAL2_MAX_COMMITS = size_t(1) << 31;

// The (WS_ED_VSS, stream) workspace of a check call:  [ per-polynomial flags, m bytes rounded up to 256, + 256 |
// H's window tables: nh x 1 280 B | decoded commitments: m t x 120 B ]
static int launch_deal_check2(size_t n, const Deal2Args& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    if (a.t && a.m > DEAL2_MAX_COMMITS / a.t) {
        set_error("kyb_ed25519_deal_check2: m * t commitments do not fit the workspace");
        return KYB_E_ALLOC;
    }
    const size_t count = a.m * a.t, flag_bytes = (a.m + 255) / 256 * 256 + 256;
    const size_t nh = a.m ? (a.h_stride ? a.m : 1) : 0;
    if (nh > DEAL2_MAX_COMMITS / 16) {
        set_error("kyb_ed25519_deal_check2: m window tables do not fit the workspace");
        return KYB_E_ALLOC;
    }
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the workspace and its kernels as one unit
    void* ws;
    if ((rc = ctx_workspace(ctx, WS_ED_VSS, st, flag_bytes + (nh ? nh : 1) * ED_TAB_BYTES + (count ? count : 1) * sizeof(ge_precomp), &ws)))
        return rc;
    uint8_t* bad = (uint8_t*)ws;
    int4* htab = (int4*)((uint8_t*)ws + flag_bytes);
    ge_precomp* aff = (ge_precomp*)((uint8_t*)ws + flag_bytes + (nh ? nh : 1) * ED_TAB_BYTES);
    KYB_HIP_CHECK(hipMemsetAsync(bad, 0, flag_bytes, st));
    if (a.status && a.m) KYB_HIP_CHECK(hipMemsetAsync(a.status, 0, a.m, st));
    if (count + nh)
        hipLaunchKernelGGL(ed25519_vss_deal_decode_kernel, ed_grid(count + nh, 64), dim3(64), 0, st, count, a.m, a.t, nh,
                           (const uint32_t*)a.commits, (const uint32_t*)a.H, aff, htab, bad, (uint8_t*)a.status);
    hipLaunchKernelGGL(ed25519_vss_deal_check2_kernel, ed_grid(n, 64), dim3(64), 0, st, n, (const uint32_t*)a.poly,
                       (const uint32_t*)a.idx, (const uint32_t*)a.f, (const uint32_t*)a.g, a.m, a.t, (const ge_precomp*)aff,
                       (const int4*)htab, a.h_stride ? size_t(1) : size_t(0), (const uint8_t*)bad, (const int32_t*)ctx->ed_wide_tab,
                       (uint8_t*)a.ok);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}

static bool sign_args_bad(size_t n, const SignArgs& a) {
    return stride_bad(a.priv_stride) || (n && (!a.k || !a.privs || !a.off || !a.sigs));
}
// a context of 32 bytes (pedersen) or 128 (rabin); one for the batch (stride 0) or one per element (stride = length)
static bool ctx_bad(size_t stride, size_t len) {
    return (len != VSS_CTX_PEDERSEN && len != VSS_CTX_RABIN) || (stride != 0 && stride != len);
}
static bool vss_seal_args_bad(size_t n, const VssSealArgs& a) {
    return ctx_bad(a.ctx_stride, a.ctx_len) ||
           (n && (!a.dh || !a.k || !a.priv || !a.pub || !a.pubs || !a.ctx || !a.off || !a.dhkeys || !a.sigs || !a.ciphers));
}
static bool vss_open_args_bad(size_t n, const VssOpenArgs& a) {
    return stride_bad(a.priv_stride) || ctx_bad(a.ctx_stride, a.ctx_len) || (n && (!a.privs || !a.dhkeys || !a.ctx || !a.off || !a.out));
}
static bool deal2_args_bad(size_t n, const Deal2Args& a) {
    return stride_bad(a.h_stride) || (n && (!a.poly || !a.idx || !a.f || !a.g || !a.ok || (a.m && !a.H) || (a.m && a.t && !a.commits)));
}

}  // namespace kyb

using namespace kyb;

extern "C" {

// schnorr.Sign (schnorr.go:56-82) for a batch
int kyb_ed25519_schnorr_sign_dev(size_t n, const void* d_k, const void* d_privs, size_t priv_stride, const void* d_msgs,
                                 const void* d_msg_off, void* d_sigs, void* d_status, void* stream) {
    const SignArgs a{d_k, d_privs, priv_stride, d_msgs, d_msg_off, d_sigs, d_status};
    if (int rc; ed_entry_done(&rc, n, sign_args_bad(n, a), "kyb_ed25519_schnorr_sign_dev: bad argument")) return rc;
    return launch_sign(n, a, (hipStream_t)stream);
}

int kyb_ed25519_schnorr_sign(size_t n, const uint8_t* k, const uint8_t* privs, size_t priv_stride, const uint8_t* msgs,
                             const uint64_t* msg_off, uint8_t* sigs, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n,
                              sign_args_bad(n, SignArgs{k, privs, priv_stride, msgs, msg_off, sigs, status}) ||
                                  (n && EdHostSpans::offsets_bad(n, msgs, msg_off)),
                              "kyb_ed25519_schnorr_sign: bad argument (pointers; a stride of 0 or 32; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, msg_off);
    return staged_call(ctx, {{k, n * 32}, {privs, priv_stride ? n * 32 : 32}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sigs, n * 64}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_sign(n, SignArgs{in[0], in[1], priv_stride, in[2], in[3], o[0], o[1]}, st);
                       });
}

// Dealer.EncryptedDeal (pedersen/vss.go:222-255, rabin/vss.go:263-297) for the n verifiers of one dealer
int kyb_ed25519_vss_seal_dev(size_t n, const void* d_dh, const void* d_k, const void* d_dealer_priv, const void* d_dealer_pub,
                             const void* d_pubs, const void* d_ctx, size_t ctx_stride, size_t ctx_len, const void* d_msgs,
                             const void* d_msg_off, void* d_dhkeys, void* d_sigs, void* d_ciphers, void* d_status, void* stream) {
    const VssSealArgs a{d_dh, d_k, d_dealer_priv, d_dealer_pub, d_pubs, d_ctx, ctx_stride, ctx_len, d_msgs, d_msg_off, d_dhkeys, d_sigs, d_ciphers,
                        d_status};
    if (int rc; ed_entry_done(&rc, n, vss_seal_args_bad(n, a), "kyb_ed25519_vss_seal_dev: bad argument")) return rc;
    return launch_vss_seal(n, a, (hipStream_t)stream);
}

int kyb_ed25519_vss_seal(size_t n, const uint8_t* dh, const uint8_t* k, const uint8_t* dealer_priv, const uint8_t* dealer_pub,
                         const uint8_t* pubs, const uint8_t* ctx_bytes, size_t ctx_stride, size_t ctx_len, const uint8_t* msgs,
                         const uint64_t* msg_off, uint8_t* dhkeys, uint8_t* sigs, uint8_t* ciphers, uint8_t* status) {
    const VssSealArgs a{dh, k, dealer_priv, dealer_pub, pubs, ctx_bytes, ctx_stride, ctx_len, msgs, msg_off, dhkeys, sigs, ciphers, status};
    if (int rc; ed_entry_done(&rc, n, vss_seal_args_bad(n, a) || (n && EdHostSpans::offsets_bad(n, msgs, msg_off)),
                              "kyb_ed25519_vss_seal: bad argument (pointers; a context of 32 or 128 bytes at a stride of 0 or its "
                              "length; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, msg_off);
    return staged_call(ctx,
                       {{dh, n * 32}, {k, n * 32}, {dealer_priv, 32}, {dealer_pub, 32}, {pubs, n * 32},
                        {ctx_bytes, ctx_stride ? n * ctx_len : ctx_len}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{dhkeys, n * 32}, {sigs, n * 64}, {sp.at(ciphers), sp.total + VSS_OVERHEAD * n}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_vss_seal(n,
                                                  VssSealArgs{in[0], in[1], in[2], in[3], in[4], in[5], ctx_stride, ctx_len, in[6], in[7], o[0], o[1],
                                                              o[2], o[3]},
                                                  st);
                       });
}

// The second half of decryptDeal (pedersen/vss.go:443-457): pre = x DHKey, newAEAD, Open
int kyb_ed25519_vss_open_dev(size_t n, const void* d_privs, size_t priv_stride, const void* d_dhkeys, const void* d_ctx,
                             size_t ctx_stride, size_t ctx_len, const void* d_ciphers, const void* d_ct_off, void* d_out, void* d_status,
                             void* stream) {
    const VssOpenArgs a{d_privs, priv_stride, d_dhkeys, d_ctx, ctx_stride, ctx_len, d_ciphers, d_ct_off, d_out, d_status};
    if (int rc; ed_entry_done(&rc, n, vss_open_args_bad(n, a), "kyb_ed25519_vss_open_dev: bad argument")) return rc;
    return launch_vss_open(n, a, (hipStream_t)stream);
}

int kyb_ed25519_vss_open(size_t n, const uint8_t* privs, size_t priv_stride, const uint8_t* dhkeys, const uint8_t* ctx_bytes,
                         size_t ctx_stride, size_t ctx_len, const uint8_t* ciphers, const uint64_t* ct_off, uint8_t* out, uint8_t* status) {
    const VssOpenArgs a{privs, priv_stride, dhkeys, ctx_bytes, ctx_stride, ctx_len, ciphers, ct_off, out, status};
    if (int rc; ed_entry_done(&rc, n, vss_open_args_bad(n, a) || (n && EdHostSpans::offsets_bad(n, ciphers, ct_off)),
                              "kyb_ed25519_vss_open: bad argument (pointers; a key stride of 0 or 32; a context of 32 or 128 bytes at "
                              "a stride of 0 or its length; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, ciphers, ct_off);
    return staged_call(ctx,
                       {{privs, priv_stride ? n * 32 : 32}, {dhkeys, n * 32}, {ctx_bytes, ctx_stride ? n * ctx_len : ctx_len},
                        {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sp.at(out), sp.total}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_vss_open(n, VssOpenArgs{in[0], priv_stride, in[1], in[2], ctx_stride, ctx_len, in[3], in[4], o[0], o[1]},
                                                  st);
                       });
}

// Rabin's VerifyDeal equation (rabin/vss.go:611-651): f B + g H against the commitments' evaluation
int kyb_ed25519_deal_check2_dev(size_t n, const void* d_poly, const void* d_idx, const void* d_f, const void* d_g, size_t m, size_t t,
                                const void* d_commits, const void* d_H, size_t h_stride, void* d_ok, void* d_status, void* stream) {
    const Deal2Args a{d_poly, d_idx, d_f, d_g, m, t, d_commits, d_H, h_stride, d_ok, d_status};
    if (int rc; ed_entry_done(&rc, n, deal2_args_bad(n, a), "kyb_ed25519_deal_check2_dev: bad argument")) return rc;
    return launch_deal_check2(n, a, (hipStream_t)stream);
}

int kyb_ed25519_deal_check2(size_t n, const uint32_t* poly, const uint32_t* idx, const uint8_t* f_shares, const uint8_t* g_shares,
                            size_t m, size_t t, const uint8_t* commits, const uint8_t* H, size_t h_stride, uint8_t* ok,
                            uint8_t* status) {
    const Deal2Args a{poly, idx, f_shares, g_shares, m, t, commits, H, h_stride, ok, status};
    if (int rc; ed_entry_done(&rc, n, deal2_args_bad(n, a), "kyb_ed25519_deal_check2: bad argument (pointers; an H stride of 0 or 32)"))
        return rc;
    for (size_t i = 0; i < n; i++)
        if (poly[i] >= m) {
            set_error("kyb_ed25519_deal_check2: bad argument (a check names a polynomial the table does not hold)");
            return KYB_E_ARG;
        }
    if ((t && m > DEAL2_MAX_COMMITS / t) || m > DEAL2_MAX_COMMITS / 16) {
        set_error("kyb_ed25519_deal_check2: m polynomials of t commitments do not fit the workspace");
        return KYB_E_ALLOC;
    }
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx, {{poly, n * 4}, {idx, n * 4}, {f_shares, n * 32}, {g_shares, n * 32}, {commits, m * t * 32},
                             {H, h_stride ? m * 32 : 32}},  // (m >= 1: some check names a polynomial)
                       {{ok, n}, {status, m, /*slack=*/1}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_deal_check2(n, Deal2Args{in[0], in[1], in[2], in[3], m, t, in[4], in[5], h_stride, o[0], o[1]},
                                                     st);
                       });
}
}
