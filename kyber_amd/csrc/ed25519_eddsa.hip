// sign/eddsa signing on Ed25519: kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_eddsa.cuh's; this unit is their kernels' own, so that the other Ed25519 units keep their kernels and their
// register allocation.
//
// Replaces, in the reference:
//   NewKeyAndSeedWithInput, Mul(secret, nil)   curve.go:51-60, eddsa.go:50-51, 81-86
//                                              -> ed25519_eddsa_expand_kernel, ed25519_eddsa_encode_kernel
//   (*EdDSA).Sign                              eddsa.go:91-142
//                                              -> ed25519_eddsa_nonce_kernel, ed25519_eddsa_encode_kernel, ed25519_eddsa_sign_kernel
// A signature is three launches per piece of ED_PIECE elements, as a Schnorr signature is (ed25519_vss.hip): the nonce
// pass hashes prefix || msg, parks R = r B as (X, Y, Z) and r behind the place of R's bytes; the shared-inversion
// encoder writes R's bytes into the slab's digit field; the last pass, one lane per element, hashes R || A || msg and
// signs.  A key expansion is two: the seed's hash and the comb in one lane, then the encoder straight into pubs.
// Every call runs on the current device: none shards over a device set.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_eddsa.cuh"
#include "ed25519_launch.h"

namespace kyb {

constexpr size_t EDDSA_PARK_WORDS = 16;  // an element's 64 B of the digit field: R's bytes, then r

// ------------------------------------------------------------------------------------------------ key expansion
// One lane per seed: secret and prefix written, A = secret B parked
__global__ __launch_bounds__(128, 3) void ed25519_eddsa_expand_kernel(size_t n, const uint32_t* __restrict__ seeds,
                                                                       const int32_t* __restrict__ wide, uint32_t* __restrict__ secrets,
                                                                       uint32_t* __restrict__ prefixes, int32_t* __restrict__ proj) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t seed[8], secret[8], prefix[8];
    load_words8(seed, seeds + idx * 8);
    ge_p3 A;
    ed_eddsa_expand_lane(A, secret, prefix, seed, wide);
    store_words8(secrets + idx * 8, secret);
    store_words8(prefixes + idx * 8, prefix);
    store_proj(proj, idx, A);
}

// The encodings of n parked points, one inversion per ENC_CHUNK points: point i's eight words at out + i * stride
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_eddsa_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                          uint32_t* __restrict__ out, size_t stride) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) { store_words8(out + i * stride, w); });
}

// ------------------------------------------------------------------------------------------------ (*EdDSA).Sign
// One lane per signature: r = SHA-512(prefix || msg) mod l behind the place of R's bytes, R = r B parked.
// key_stride: 8 words, or 0 for one key.
__global__ __launch_bounds__(128, 3) void ed25519_eddsa_nonce_kernel(size_t n, const uint32_t* __restrict__ prefixes, size_t key_stride,
                                                                      const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                                                      const int32_t* __restrict__ wide, sf::Mod m,
                                                                      int32_t* __restrict__ proj, uint32_t* __restrict__ park) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t pw[8], rw[8];
    load_words8(pw, prefixes + idx * key_stride);
    ge_p3 R;
    ed_eddsa_nonce_lane(R, rw, pw, msgs + off[idx], (size_t)element_len(off, idx), wide, m);
    store_proj(proj, idx, R);
    store_words8(park + idx * EDDSA_PARK_WORDS + 8, rw);
}

// One lane per signature: h = SHA-512(R || A || msg) mod l, S = r + h a mod l, sig = R || S
__global__ __launch_bounds__(128, 3) void ed25519_eddsa_sign_kernel(size_t n, const uint32_t* __restrict__ secrets,
                                                                     const uint32_t* __restrict__ pubs, size_t key_stride,
                                                                     const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ park, sf::Mod m,
                                                                     uint32_t* __restrict__ sigs, uint8_t* __restrict__ status) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t sw[8], aw[8], rb[8], rw[8], sig[16];
    load_words8(sw, secrets + idx * key_stride);
    load_words8(aw, pubs + idx * key_stride);
    load_words8(rb, park + idx * EDDSA_PARK_WORDS);
    load_words8(rw, park + idx * EDDSA_PARK_WORDS + 8);
    ed_eddsa_sign_element(sig, rb, aw, rw, sw, msgs + off[idx], (size_t)element_len(off, idx), m);
    store_words8(sigs + idx * 16, sig);
    store_words8(sigs + idx * 16 + 8, sig + 8);
    if (status) status[idx] = KYB_ST_OK;
}

struct ExpandArgs {
    const void* seeds;
    void *secrets, *prefixes, *pubs;
};
struct SignArgs {
    const void *secrets, *prefixes, *pubs;
    size_t key_stride;
    const void *msgs, *off;
    void *sigs, *status;
};

static int launch_expand(size_t n, const ExpandArgs& a, hipStream_t st) {
    return ed_for_pieces(n, st, ED_SLAB_MUL_BASE, [&](DeviceCtx* ctx, size_t lo, size_t cnt, const EdSlab& w) {
        hipLaunchKernelGGL(ed25519_eddsa_expand_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)a.seeds + lo * 8, (const int32_t*)ctx->ed_wide_tab, (uint32_t*)a.secrets + lo * 8,
                           (uint32_t*)a.prefixes + lo * 8, w.proj);
        hipLaunchKernelGGL(ed25519_eddsa_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt, (const int32_t*)w.proj,
                           (uint32_t*)a.pubs + lo * 8, size_t(8));
    });
}

static int launch_sign(size_t n, const SignArgs& a, hipStream_t st) {
    const size_t ks = a.key_stride / 4;
    return ed_for_pieces(n, st, ED_SLAB_EDDSA_SIGN, [&](DeviceCtx* ctx, size_t lo, size_t cnt, const EdSlab& w) {
        const dim3 lanes = ed_grid(cnt, 128);
        const uint8_t* msgs = (const uint8_t*)a.msgs;
        const uint64_t* off = (const uint64_t*)a.off + lo;
        hipLaunchKernelGGL(ed25519_eddsa_nonce_kernel, lanes, dim3(128), 0, st, cnt, (const uint32_t*)a.prefixes + lo * ks, ks, msgs, off,
                           (const int32_t*)ctx->ed_wide_tab, ed_order(), w.proj, w.digits);
        hipLaunchKernelGGL(ed25519_eddsa_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt, (const int32_t*)w.proj,
                           w.digits, EDDSA_PARK_WORDS);
        hipLaunchKernelGGL(ed25519_eddsa_sign_kernel, lanes, dim3(128), 0, st, cnt, (const uint32_t*)a.secrets + lo * ks,
                           (const uint32_t*)a.pubs + lo * ks, ks, msgs, off, (const uint32_t*)w.digits, ed_order(),
                           (uint32_t*)a.sigs + lo * 16, a.status ? (uint8_t*)a.status + lo : nullptr);
    });
}

static bool expand_args_bad(size_t n, const ExpandArgs& a) { return n && (!a.seeds || !a.secrets || !a.prefixes || !a.pubs); }
static bool sign_args_bad(size_t n, const SignArgs& a) {
    return stride_bad(a.key_stride) || (n && (!a.secrets || !a.prefixes || !a.pubs || !a.off || !a.sigs));
}

}  // namespace kyb

using namespace kyb;

extern "C" {

// NewKeyAndSeedWithInput and Mul(secret, nil) (curve.go:51-60, eddsa.go:50-51, 81-86) for a batch of seeds
int kyb_ed25519_eddsa_expand_dev(size_t n, const void* d_seeds, void* d_secrets, void* d_prefixes, void* d_pubs, void* stream) {
    const ExpandArgs a{d_seeds, d_secrets, d_prefixes, d_pubs};
    if (int rc; ed_entry_done(&rc, n, expand_args_bad(n, a), "kyb_ed25519_eddsa_expand_dev: bad argument")) return rc;
    return launch_expand(n, a, (hipStream_t)stream);
}

int kyb_ed25519_eddsa_expand(size_t n, const uint8_t* seeds, uint8_t* secrets, uint8_t* prefixes, uint8_t* pubs) {
    if (int rc; ed_entry_done(&rc, n, expand_args_bad(n, ExpandArgs{seeds, secrets, prefixes, pubs}),
                              "kyb_ed25519_eddsa_expand: bad argument (a NULL pointer)")) return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx, {{seeds, n * 32}}, {{secrets, n * 32}, {prefixes, n * 32}, {pubs, n * 32}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return launch_expand(n, ExpandArgs{in[0], o[0], o[1], o[2]}, st); });
}

// (*EdDSA).Sign (eddsa.go:91-142) for a batch
int kyb_ed25519_eddsa_sign_dev(size_t n, const void* d_secrets, const void* d_prefixes, const void* d_pubs, size_t key_stride,
                               const void* d_msgs, const void* d_msg_off, void* d_sigs, void* d_status, void* stream) {
    const SignArgs a{d_secrets, d_prefixes, d_pubs, key_stride, d_msgs, d_msg_off, d_sigs, d_status};
    if (int rc; ed_entry_done(&rc, n, sign_args_bad(n, a), "kyb_ed25519_eddsa_sign_dev: bad argument")) return rc;
    return launch_sign(n, a, (hipStream_t)stream);
}

int kyb_ed25519_eddsa_sign(size_t n, const uint8_t* secrets, const uint8_t* prefixes, const uint8_t* pubs, size_t key_stride,
                           const uint8_t* msgs, const uint64_t* msg_off, uint8_t* sigs, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n,
                              sign_args_bad(n, SignArgs{secrets, prefixes, pubs, key_stride, msgs, msg_off, sigs, status}) ||
                                  (n && EdHostSpans::offsets_bad(n, msgs, msg_off)),
                              "kyb_ed25519_eddsa_sign: bad argument (pointers; a stride of 0 or 32; offsets that do not decrease)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, msg_off);
    const size_t keys = key_stride ? n * 32 : 32;
    return staged_call(ctx,
                       {{secrets, keys}, {prefixes, keys}, {pubs, keys}, {sp.base, sp.total}, {sp.offsets(), sp.offsets_bytes()}},
                       {{sigs, n * 64}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_sign(n, SignArgs{in[0], in[1], in[2], key_stride, in[3], in[4], o[0], o[1]}, st);
                       });
}

}  // extern "C"
