// share/dkg and encrypt/ecies on Ed25519: kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_dkg.cuh's and aes256gcm.cuh's; this unit is their kernels' own, so that ed25519.o, ed25519_verify.o,
// ed25519_dleq.o, ed25519_ring.o and ed25519_shuffle.o keep their kernels and their register allocation (DESIGN.md
// section 5 items 41-42).
//
// Replaces, in the reference:
//   encrypt/ecies Encrypt   ecies.go:23-69   -> ed25519_ecies_seal_kernel, ed25519_ecies_encode_kernel<2>, ed25519_ecies_seal_aead_kernel
//   encrypt/ecies Decrypt   ecies.go:77-112  -> ed25519_ecies_open_kernel, ed25519_ecies_encode_kernel<1>, ed25519_ecies_open_aead_kernel
//   the share check of ProcessDeals / ProcessJustifications   dkg.go:488-495, 824-832 over share/poly.go:340-348, 405-409
//                                            -> ed25519_deal_decode_kernel, ed25519_deal_check_kernel
// A seal or an open is three launches per piece of ED_PIECE elements: the point pass parks (X, Y, Z) of r B and r pub
// (or of x R) and keeps its window table in the slab; the shared-inversion encoder writes the points' bytes into the
// first 64 bytes of the element's table, which is dead by then; the AEAD pass, one lane per element, derives key and
// nonce from those bytes and streams the message.  LDS of the AEAD pass: the S-box (256 B) and the block's round keys
// (64 lanes x 60 words, [word][lane]) -- ED_AEAD_LDS_BYTES.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_dkg.cuh"
#include "ed25519_launch.h"

namespace kyb {

static_assert(ED_DKG_ST_OK == KYB_ST_OK && ED_DKG_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_ECIES_SHORT == KYB_ST_ECIES_SHORT &&
                  ED_ST_ECIES_AUTH == KYB_ST_ECIES_AUTH,
              "status values of include/kyber_hip.h");

// One lane per element; lanes past n leave before the table.  pub_stride: 8 words, or 0 for one recipient.
__global__ __launch_bounds__(128, 3) void ed25519_ecies_seal_kernel(size_t n, const uint32_t* __restrict__ r,
                                                                     const uint32_t* __restrict__ pubs, size_t pub_stride,
                                                                     const int32_t* __restrict__ wide, int32_t* __restrict__ proj,
                                                                     uint8_t* __restrict__ st, int4* __restrict__ gtab) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t rw[8], pw[8];
    load_words8(rw, r + idx * 8);
    load_words8(pw, pubs + idx * pub_stride);
    TabGlobal tab{gtab + idx * 80};
    ge_p3 R, D;
    const int s = ed_ecies_seal_lane(R, D, rw, pw, wide, tab);
    store_proj(proj, 2 * idx, R);
    store_proj(proj, 2 * idx + 1, D);
    st[idx] = (uint8_t)s;
}

// priv_stride: 8 words, or 0 for one receiver.  ctx + off[i]: the element's bytes, of any alignment.
__global__ __launch_bounds__(128, 3) void ed25519_ecies_open_kernel(size_t n, const uint32_t* __restrict__ privs, size_t priv_stride,
                                                                     const uint8_t* __restrict__ ctx, const uint64_t* __restrict__ off,
                                                                     int32_t* __restrict__ proj, uint8_t* __restrict__ st,
                                                                     int4* __restrict__ gtab) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t xw[8];
    load_words8(xw, privs + idx * priv_stride);
    TabGlobal tab{gtab + idx * 80};
    ge_p3 D;
    const int s = ed_ecies_open_lane(D, xw, ctx + off[idx], element_len(off, idx), tab);
    store_proj(proj, idx, D);
    st[idx] = (uint8_t)s;
}

// The encodings of an element's GROUP parked points, one inversion per ENC_CHUNK points, into the front of the
// element's window table: point k at word 8 k.  n: elements.
template <int GROUP>
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_ecies_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                          int4* __restrict__ gtab) {
    static_assert(GROUP * 32 <= (int)ED_TAB_BYTES, "the bytes fit the table they replace");
    EncPreScratch pre;
    ed_encode_chunk<GROUP>(n, proj, ed_encode_first<GROUP>(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        store_words8((uint32_t*)gtab + (i / GROUP) * ED_TAB_WORDS32 + (i % GROUP) * 8, w);
    });
}

// first: the batch index of the piece's element 0 (its slot lies 48 bytes further for every element before it)
__global__ __launch_bounds__(ED_AEAD_BLOCK, KYB_TU_WAVES) void ed25519_ecies_seal_aead_kernel(
    size_t n, size_t first, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off, const int4* __restrict__ gtab,
    const uint8_t* __restrict__ st, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    __shared__ uint8_t sbox[256];
    __shared__ uint32_t keys[AesKeysLds<ED_AEAD_BLOCK>::WORDS];
    static_assert(sizeof(sbox) + sizeof(keys) == ED_AEAD_LDS_BYTES, "the layout the header of this file states");
    aes_fill_sbox(sbox, (int)threadIdx.x, (int)ED_AEAD_BLOCK);
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    AesKeysLds<ED_AEAD_BLOCK> rk{keys + threadIdx.x};
    uint32_t Rw[8], dh[8];
    load_words8(Rw, (const uint32_t*)gtab + idx * ED_TAB_WORDS32);
    load_words8(dh, (const uint32_t*)gtab + idx * ED_TAB_WORDS32 + 8);
    const int s = st[idx];
    ed_ecies_seal_element(out + off[idx] + ECIES_OVERHEAD * (first + idx), msgs + off[idx], element_len(off, idx), Rw, dh, s, rk, sbox);
    if (status) status[idx] = (uint8_t)s;
}

__global__ __launch_bounds__(ED_AEAD_BLOCK, KYB_TU_WAVES) void ed25519_ecies_open_aead_kernel(
    size_t n, const uint8_t* __restrict__ ctx, const uint64_t* __restrict__ off, const int4* __restrict__ gtab,
    const uint8_t* __restrict__ st, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    __shared__ uint8_t sbox[256];
    __shared__ uint32_t keys[AesKeysLds<ED_AEAD_BLOCK>::WORDS];
    static_assert(sizeof(sbox) + sizeof(keys) == ED_AEAD_LDS_BYTES, "the layout the header of this file states");
    aes_fill_sbox(sbox, (int)threadIdx.x, (int)ED_AEAD_BLOCK);
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    AesKeysLds<ED_AEAD_BLOCK> rk{keys + threadIdx.x};
    uint32_t dh[8];
    load_words8(dh, (const uint32_t*)gtab + idx * ED_TAB_WORDS32);
    const int s = ed_ecies_open_element(out + off[idx], ctx + off[idx], element_len(off, idx), dh, st[idx], rk, sbox);
    if (status) status[idx] = (uint8_t)s;
}

// One lane per commitment: aff[j] = its mixed-addition operand; a commitment that does not decode marks its polynomial
__global__ __launch_bounds__(64, 3) void ed25519_deal_decode_kernel(size_t count, size_t t, const uint32_t* __restrict__ commits,
                                                                     ge_precomp* __restrict__ aff, uint8_t* __restrict__ bad,
                                                                     uint8_t* __restrict__ status) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    uint32_t w[8];
    load_words8(w, commits + j * 8);
    ge_precomp a;
    const bool ok = ed_deal_decode(a, w);
    aff[j] = a;
    if (!ok) {  // (every lane that stores here stores the same value)
        bad[j / t] = 1;
        if (status) status[j / t] = KYB_ST_BAD_POINT;
    }
}

// One lane per check.  A polynomial index outside the table reads nothing.
__global__ __launch_bounds__(64, 3) void ed25519_deal_check_kernel(size_t n, const uint32_t* __restrict__ poly,
                                                                    const uint32_t* __restrict__ idx, const uint32_t* __restrict__ shares,
                                                                    size_t m, size_t t, const ge_precomp* __restrict__ aff,
                                                                    const uint8_t* __restrict__ bad, const int32_t* __restrict__ wide,
                                                                    uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t k = poly[i];
    if (k >= m || bad[k]) {
        ok[i] = 0;
        return;
    }
    uint32_t sw[8];
    load_words8(sw, shares + i * 8);
    ok[i] = ed_deal_check_lane(sw, aff + k * t, t, idx[i], wide) ? 1 : 0;
}

struct SealArgs {
    const void *r, *pubs;
    size_t pub_stride;
    const void *msgs, *off;
    void *out, *status;
};
struct OpenArgs {
    const void* privs;
    size_t priv_stride;
    const void *ctx, *off;
    void *out, *status;
};

static int launch_seal(size_t n, const SealArgs& a, hipStream_t st) {
    const size_t ps = a.pub_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_ECIES_SEAL, [&](DeviceCtx* ctx, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_ecies_seal_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.r + lo * 8, (const uint32_t*)a.pubs + lo * ps, ps, (const int32_t*)ctx->ed_wide_tab,
                           w.proj, w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_ecies_encode_kernel<2>, ed_encode_grid(2 * cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, w.gtab);
        hipLaunchKernelGGL(ed25519_ecies_seal_aead_kernel, ed_grid(cnt, ED_AEAD_BLOCK),
                           dim3(ED_AEAD_BLOCK), 0, st, cnt, lo, (const uint8_t*)a.msgs, (const uint64_t*)a.off + lo,
                           (const int4*)w.gtab, (const uint8_t*)w.status, (uint8_t*)a.out,
                           a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static int launch_open(size_t n, const OpenArgs& a, hipStream_t st) {
    const size_t ps = a.priv_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_ECIES_OPEN, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_ecies_open_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.privs + lo * ps, ps, (const uint8_t*)a.ctx, (const uint64_t*)a.off + lo, w.proj,
                           w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_ecies_encode_kernel<1>, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, w.gtab);
        hipLaunchKernelGGL(ed25519_ecies_open_aead_kernel, ed_grid(cnt, ED_AEAD_BLOCK),
                           dim3(ED_AEAD_BLOCK), 0, st, cnt, (const uint8_t*)a.ctx, (const uint64_t*)a.off + lo, (const int4*)w.gtab,
                           (const uint8_t*)w.status, (uint8_t*)a.out, a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static bool seal_args_bad(size_t n, const SealArgs& a) {
    return stride_bad(a.pub_stride) || (n && (!a.r || !a.pubs || !a.off || !a.out));
}
static bool open_args_bad(size_t n, const OpenArgs& a) {
    return stride_bad(a.priv_stride) || (n && (!a.privs || !a.off || !a.out));
}

struct DealArgs {
    const void *poly, *idx, *shares;
    size_t m, t;
    const void* commits;
    void *ok, *status;
};
static bool deal_args_bad(size_t n, const DealArgs& a) {
    return n && (!a.poly || !a.idx || !a.shares || !a.ok || (a.m && a.t && !a.commits));
}
// the decoded table of m polynomials: 120 B a commitment behind the per-polynomial flags
constexpr size_t DEAL_MAX_COMMITS = size_t(1) << 31;

static int launch_deal_check(size_t n, const DealArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    if (a.t && a.m > DEAL_MAX_COMMITS / a.t) {
        set_error("kyb_ed25519_deal_check: m * t commitments do not fit the workspace");
        return KYB_E_ALLOC;
    }
    const size_t count = a.m * a.t, flag_bytes = (a.m + 255) / 256 * 256 + 256;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the workspace and its kernels as one unit
    void* ws;
    if ((rc = ctx_workspace(ctx, WS_ED, st, flag_bytes + (count ? count : 1) * sizeof(ge_precomp), &ws))) return rc;
    uint8_t* bad = (uint8_t*)ws;
    ge_precomp* aff = (ge_precomp*)((uint8_t*)ws + flag_bytes);
    KYB_HIP_CHECK(hipMemsetAsync(bad, 0, flag_bytes, st));
    if (a.status && a.m) KYB_HIP_CHECK(hipMemsetAsync(a.status, 0, a.m, st));
    if (count)
        hipLaunchKernelGGL(ed25519_deal_decode_kernel, ed_grid(count, 64), dim3(64), 0, st, count, a.t,
                           (const uint32_t*)a.commits, aff, bad, (uint8_t*)a.status);
    hipLaunchKernelGGL(ed25519_deal_check_kernel, ed_grid(n, 64), dim3(64), 0, st, n, (const uint32_t*)a.poly,
                       (const uint32_t*)a.idx, (const uint32_t*)a.shares, a.m, a.t, (const ge_precomp*)aff, (const uint8_t*)bad,
                       (const int32_t*)ctx->ed_wide_tab, (uint8_t*)a.ok);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_ecies_seal_dev(size_t n, const void* d_r, const void* d_pubs, size_t pub_stride, const void* d_msgs,
                               const void* d_msg_off, void* d_out, void* d_status, void* stream) {
    const SealArgs a{d_r, d_pubs, pub_stride, d_msgs, d_msg_off, d_out, d_status};
    if (int rc; ed_entry_done(&rc, n, seal_args_bad(n, a), "kyb_ed25519_ecies_seal_dev: bad argument")) return rc;
    return launch_seal(n, a, (hipStream_t)stream);
}

int kyb_ed25519_ecies_seal(size_t n, const uint8_t* r, const uint8_t* pubs, size_t pub_stride, const uint8_t* msgs,
                           const uint64_t* msg_off, uint8_t* out, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n,
                              seal_args_bad(n, SealArgs{r, pubs, pub_stride, msgs, msg_off, out, status}) ||
                                  (n && EdHostSpans::offsets_bad(n, msgs, msg_off)),
                              "kyb_ed25519_ecies_seal: bad argument (pointers; a stride of 0 or 32; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, msg_off);
    return staged_call(ctx, {{r, n * 32}, {pubs, pub_stride ? n * 32 : 32}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sp.at(out), sp.total + ECIES_OVERHEAD * n}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_seal(n, SealArgs{in[0], in[1], pub_stride, in[2], in[3], o[0], o[1]}, st);
                       });
}

int kyb_ed25519_ecies_open_dev(size_t n, const void* d_privs, size_t priv_stride, const void* d_ctx, const void* d_ctx_off,
                               void* d_out, void* d_status, void* stream) {
    const OpenArgs a{d_privs, priv_stride, d_ctx, d_ctx_off, d_out, d_status};
    if (int rc; ed_entry_done(&rc, n, open_args_bad(n, a), "kyb_ed25519_ecies_open_dev: bad argument")) return rc;
    return launch_open(n, a, (hipStream_t)stream);
}

int kyb_ed25519_ecies_open(size_t n, const uint8_t* privs, size_t priv_stride, const uint8_t* ctx_bytes, const uint64_t* ctx_off,
                           uint8_t* out, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n,
                              open_args_bad(n, OpenArgs{privs, priv_stride, ctx_bytes, ctx_off, out, status}) ||
                                  (n && EdHostSpans::offsets_bad(n, ctx_bytes, ctx_off)),
                              "kyb_ed25519_ecies_open: bad argument (pointers; a stride of 0 or 32; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, ctx_bytes, ctx_off);
    return staged_call(ctx, {{privs, priv_stride ? n * 32 : 32}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sp.at(out), sp.total}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_open(n, OpenArgs{in[0], priv_stride, in[1], in[2], o[0], o[1]}, st);
                       });
}

int kyb_ed25519_deal_check_dev(size_t n, const void* d_poly, const void* d_idx, const void* d_shares, size_t m, size_t t,
                               const void* d_commits, void* d_ok, void* d_status, void* stream) {
    const DealArgs a{d_poly, d_idx, d_shares, m, t, d_commits, d_ok, d_status};
    if (int rc; ed_entry_done(&rc, n, deal_args_bad(n, a), "kyb_ed25519_deal_check_dev: bad argument")) return rc;
    return launch_deal_check(n, a, (hipStream_t)stream);
}

int kyb_ed25519_deal_check(size_t n, const uint32_t* poly, const uint32_t* idx, const uint8_t* shares, size_t m, size_t t,
                           const uint8_t* commits, uint8_t* ok, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n, deal_args_bad(n, DealArgs{poly, idx, shares, m, t, commits, ok, status}),
                              "kyb_ed25519_deal_check: bad argument")) return rc;
    for (size_t i = 0; i < n; i++)
        if (poly[i] >= m) {
            set_error("kyb_ed25519_deal_check: bad argument (a check names a polynomial the table does not hold)");
            return KYB_E_ARG;
        }
    if (t && m > DEAL_MAX_COMMITS / t) {
        set_error("kyb_ed25519_deal_check: m * t commitments do not fit the workspace");
        return KYB_E_ALLOC;
    }
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx, {{poly, n * 4}, {idx, n * 4}, {shares, n * 32}, {commits, m * t * 32}}, {{ok, n}, {status, m, /*slack=*/1}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_deal_check(n, DealArgs{in[0], in[1], in[2], m, t, in[3], o[0], o[1]}, st);
                       });
}
}
