// encrypt/ibe on BLS12-381: EncryptCCAonG1 / DecryptCCAonG1 and EncryptCCAonG2 / DecryptCCAonG2 (ibe.go:51-232) as
// batch operations, one ciphertext per lane, the suite hash SHA-256 and kilic's 576-byte GT layout.  The heavy parts are
// the engine's own: the tower machine's PAIR program, GTMUL (GT exponentiation) and the fixed-base tables; the kernels
// here do the per-lane hashing between them (bls12381_ibe.cuh) and the CCA check.
//
// Decrypt, per piece of at most PIECE ciphertexts, all on the caller's stream:
//   operand kernel + PAIR        gt = e(U, private)  (OnG2: e(private, U)); the private key is argument 0, U argument 1
//   bls12381_ibe_open_kernel     sigma = V ^ H2(gt), msg = W ^ H4(sigma), r = h3(sigma, msg)
//   fixed-base table (fb_run)    r * Base of U's group
//   bls12381_ibe_check_kernel    status (key, then U, then the rP check) and the message or zero bytes
// Encrypt: once per call, the operand kernel hashes the ID and PAIR gives Gid = e(master, H(ID)) (OnG2: e(H(ID), master));
// then per piece
//   bls12381_ibe_seal_kernel     r = h3(sigma, msg), W = msg ^ H4(sigma)
//   fixed-base table (fb_run)    U = r * Base
//   GTMUL                        Gid^r, Gid read by every lane (stride 0)
//   bls12381_ibe_mask_kernel     V = sigma ^ H2(Gid^r); status; zero bytes for a rejected master key
// The intermediates live in a (WS_IBE, stream) workspace sized for one piece, so a batch of 2^20 ciphertexts pins the
// ~55 MB of a 2^16 piece, not gigabytes.
#include "bls12381.cuh"
#include "bls12381_ibe.cuh"
#include "bls12381_tvm.h"
#include "pairing_abi.cuh"

#include <string>

namespace kyb {
int bls12381_fb_run(bool g2, size_t n, const void* d_scalars, const void* d_points, void* d_out, void* d_status, uint32_t flags,
                    hipStream_t st, const std::string* key);

namespace ibe {

constexpr size_t PIECE = size_t(1) << 16;

// the groups' generators (G1().Point().Base(), G2().Point().Base()), compressed, written into the workspace: the fixed
// bases of r * Base (one lane; the bytes are literals of the kernel's code)
__global__ __launch_bounds__(1) void bls12381_ibe_base_kernel(uint8_t* __restrict__ out, int g2) {
    constexpr uint8_t G1[48] = {
        0x97, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f, 0xc3, 0x68, 0x8c, 0x4f,
        0x97, 0x74, 0xb9, 0x05, 0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58, 0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef,
        0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};
    constexpr uint8_t G2[96] = {
        0x93, 0xe0, 0x2b, 0x60, 0x52, 0x71, 0x9f, 0x60, 0x7d, 0xac, 0xd3, 0xa0, 0x88, 0x27, 0x4f, 0x65, 0x59, 0x6b, 0xd0, 0xd0,
        0x99, 0x20, 0xb6, 0x1a, 0xb5, 0xda, 0x61, 0xbb, 0xdc, 0x7f, 0x50, 0x49, 0x33, 0x4c, 0xf1, 0x12, 0x13, 0x94, 0x5d, 0x57,
        0xe5, 0xac, 0x7d, 0x05, 0x5d, 0x04, 0x2b, 0x7e, 0x02, 0x4a, 0xa2, 0xb2, 0xf0, 0x8f, 0x0a, 0x91, 0x26, 0x08, 0x05, 0x27,
        0x2d, 0xc5, 0x10, 0x51, 0xc6, 0xe4, 0x7a, 0xd4, 0xfa, 0x40, 0x3b, 0x02, 0xb4, 0x51, 0x0b, 0x64, 0x7a, 0xe3, 0xd1, 0x77,
        0x0b, 0xac, 0x03, 0x26, 0xa8, 0x05, 0xbb, 0xef, 0xd4, 0x80, 0x56, 0xc8, 0xc1, 0x21, 0xbd, 0xb8};
    if (threadIdx.x != 0) return;
    if (g2) {
#pragma unroll
        for (int j = 0; j < 96; j++) out[j] = G2[j];
    } else {
#pragma unroll
        for (int j = 0; j < 48; j++) out[j] = G1[j];
    }
}

// eight big-endian words to 32 bytes at a 16-byte aligned address of the workspace
__device__ __forceinline__ void put_words(uint8_t* p, const uint32_t (&w)[8]) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(__builtin_bswap32(w[0]), __builtin_bswap32(w[1]), __builtin_bswap32(w[2]), __builtin_bswap32(w[3]));
    q[1] = make_uint4(__builtin_bswap32(w[4]), __builtin_bswap32(w[5]), __builtin_bswap32(w[6]), __builtin_bswap32(w[7]));
}
__device__ __forceinline__ void get_words(uint32_t (&w)[8], const uint8_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    w[0] = __builtin_bswap32(a.x); w[1] = __builtin_bswap32(a.y); w[2] = __builtin_bswap32(a.z); w[3] = __builtin_bswap32(a.w);
    w[4] = __builtin_bswap32(b.x); w[5] = __builtin_bswap32(b.y); w[6] = __builtin_bswap32(b.z); w[7] = __builtin_bswap32(b.w);
}

// Decrypt steps 1-3 but the multiplication (ibe.go:100-126): gt (576 B per element, the PAIR launch's output) ->
// r (32 B big-endian, the fixed-base launch's scalar), msg (32 B, zero beyond len), h3's status.
__global__ __launch_bounds__(64) void bls12381_ibe_open_kernel(size_t n, const uint8_t* __restrict__ gt, const uint8_t* __restrict__ v,
                                                               const uint8_t* __restrict__ w, int len, uint8_t* __restrict__ r_out,
                                                               uint8_t* __restrict__ m_out, uint8_t* __restrict__ hst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8], c[8], sigma[8], msg[8], r[8];
    h2(d, gt + (size_t)GT_BYTES * i);
    load_words(c, v + (size_t)len * i, len);
    xor_words(sigma, c, d, len);
    h4(d, sigma, len);
    load_words(c, w + (size_t)len * i, len);
    xor_words(msg, c, d, len);
    hst[i] = (uint8_t)h3(r, sigma, msg, len);
    put_words(r_out + 32 * i, r);
    put_words(m_out + 32 * i, msg);
}

// Decrypt step 3's comparison (ibe.go:123-131) and the verdict.  Status precedence: the PAIR launch's (the private key,
// argument 0, then U, argument 1 -- UnmarshalBinary's errors, ibe.go's callers unmarshal both before decrypting), then
// h3's, then rP == U.
//
// rP.Equal(U) is decided on the encodings: r * Base encoded in U's input format (compressed, or uncompressed under
// KYB_F_UNCOMPRESSED) against the caller's U bytes.  That is Point.Equal because a U that got here decoded, and the
// decoders (bls12381.cuh g1_decode / g2_decode and their uncompressed forms) accept only canonical encodings --
// coordinates below p, no stray flag bits, an all-zero body for infinity -- so each point has one accepted encoding.
__global__ __launch_bounds__(64) void bls12381_ibe_check_kernel(size_t n, const uint8_t* __restrict__ pst, const uint8_t* __restrict__ hst,
                                                                const uint8_t* __restrict__ ru, const uint8_t* __restrict__ u, uint32_t usz,
                                                                const uint8_t* __restrict__ m, int len, uint8_t* __restrict__ msgs,
                                                                uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int st = pst[i] ? pst[i] : (hst[i] ? ST_IBE_H3 : 0);
    if (!st) {
        const uint8_t* a = ru + (size_t)usz * i;
        const uint8_t* b = u + (size_t)usz * i;
        uint32_t diff = 0;
        for (uint32_t k = 0; k < usz; k++) diff |= a[k] ^ b[k];
        if (diff) st = ST_IBE_CHECK;
    }
    uint32_t msg[8];
    get_words(msg, m + 32 * i);
#pragma unroll
    for (int k = 0; k < 8; k++) msg[k] = st ? 0u : msg[k];
    store_words(msgs + (size_t)len * i, msg, len);
    if (status) status[i] = (uint8_t)st;
}

// Encrypt steps 3 and 6 (ibe.go:66-72, 84-89): r = h3(sigma, msg) for the fixed-base and GTMUL launches, W = msg ^ H4(sigma).
__global__ __launch_bounds__(64) void bls12381_ibe_seal_kernel(size_t n, const uint8_t* __restrict__ sigmas, const uint8_t* __restrict__ msgs,
                                                               int len, uint8_t* __restrict__ r_out, uint8_t* __restrict__ w,
                                                               uint8_t* __restrict__ hst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t sigma[8], msg[8], d[8], r[8];
    load_words(sigma, sigmas + (size_t)len * i, len);
    load_words(msg, msgs + (size_t)len * i, len);
    hst[i] = (uint8_t)h3(r, sigma, msg, len);
    put_words(r_out + 32 * i, r);
    h4(d, sigma, len);
    xor_words(msg, msg, d, len);
    store_words(w + (size_t)len * i, msg, len);
}

// Encrypt step 5 (ibe.go:76-82): V = sigma ^ H2(Gid^r), and the verdict: the master key's UnmarshalBinary status (the
// Gid launch's), then h3's.  A rejected element gets zero bytes in U, V and W.
__global__ __launch_bounds__(64) void bls12381_ibe_mask_kernel(size_t n, const uint8_t* __restrict__ gt, const uint8_t* __restrict__ sigmas,
                                                               int len, const uint8_t* __restrict__ gid_st, const uint8_t* __restrict__ hst,
                                                               uint8_t* __restrict__ u, uint32_t usz, uint8_t* __restrict__ v,
                                                               uint8_t* __restrict__ w, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int st = gid_st[0] ? gid_st[0] : (hst[i] ? ST_IBE_H3 : 0);
    uint32_t sigma[8], d[8];
    if (st) {
        for (uint32_t k = 0; k < usz; k++) u[(size_t)usz * i + k] = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) sigma[k] = 0;
        store_words(w + (size_t)len * i, sigma, len);
    } else {
        h2(d, gt + (size_t)GT_BYTES * i);
        load_words(sigma, sigmas + (size_t)len * i, len);
        xor_words(sigma, sigma, d, len);
    }
    store_words(v + (size_t)len * i, sigma, len);
    if (status) status[i] = (uint8_t)st;
}

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// (WS_IBE, stream) workspace of one piece of p elements: the layout is shared by both directions
struct Ws {
    uint8_t *gt, *r, *m, *ru, *pst, *hst, *gid, *gid_st, *base;
};
static int workspace(DeviceCtx* ctx, hipStream_t st, size_t p, Ws* ws) {
    const size_t o_r = al256(GT_BYTES * p), o_m = o_r + al256(32 * p), o_ru = o_m + al256(32 * p), o_pst = o_ru + al256(192 * p),
                 o_hst = o_pst + al256(p), o_gid = o_hst + al256(p), o_gst = o_gid + al256(GT_BYTES), o_base = o_gst + 256, total = o_base + 256;
    void* base;
    KYB_TRY(ctx_workspace(ctx, WS_IBE, st, total, &base));
    uint8_t* b = (uint8_t*)base;
    *ws = Ws{b, b + o_r, b + o_m, b + o_ru, b + o_pst, b + o_hst, b + o_gid, b + o_gst, b + o_base};
    return KYB_OK;
}
// enqueues the generator's bytes into the workspace's base slot
static int base_point(const Ws& ws, bool g2, hipStream_t st) {
    hipLaunchKernelGGL(bls12381_ibe_base_kernel, dim3(1), dim3(1), 0, st, ws.base, g2 ? 1 : 0);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}
// the decrypt's fixed-base flags: the generator is compressed and vouched for; r * Base comes out in U's input format
static uint32_t fb_flags(uint32_t flags) { return KYB_F_TRUSTED(0) | ((flags & KYB_F_UNCOMPRESSED) ? KYB_F_UNCOMPRESSED_OUT : 0u); }

// on_g2: the scheme of EncryptCCAonG2 / DecryptCCAonG2 (master key and U on G2, identity and private key on G1)
static int decrypt_dev(bool on_g2, const char* who, size_t n, const uint8_t* d_priv, size_t priv_stride, const uint8_t* d_u,
                       const uint8_t* d_v, const uint8_t* d_w, size_t msg_len, uint8_t* d_msgs, uint8_t* d_status, uint32_t flags,
                       hipStream_t st) {
    KYB_TRY(check_flags(flags, 2, false, who));
    const size_t ksz = on_g2 ? bls::g1_wire_size(flags) : bls::g2_wire_size(flags);
    const size_t usz = on_g2 ? bls::g2_wire_size(flags) : bls::g1_wire_size(flags);
    if (msg_len > (size_t)MSG_MAX || (priv_stride != 0 && priv_stride != ksz) ||
        (n && (!d_priv || !d_u || ((!d_v || !d_w || !d_msgs) && msg_len)))) {
        set_error(std::string(who) + ": bad argument (msg_len 0..32, private_stride 0 or the key's wire size, non-null buffers)");
        return KYB_E_ARG;
    }
    if (!n) return KYB_OK;
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    const int len = (int)msg_len;
    Ws ws;
    KYB_TRY(workspace(ctx, st, n < PIECE ? n : PIECE, &ws));
    KYB_TRY(base_point(ws, on_g2, st));
    for (size_t lo = 0; lo < n; lo += PIECE) {
        const size_t cnt = n - lo < PIECE ? n - lo : PIECE;
        blsvm::Work w;
        KYB_TRY(blsvm::workspace(ctx, st, cnt, blsvm::PAIR_INPUTS, &w));
        // slot 0 the private key, slot 1 U: the machine reports the first operand that failed, in that order; the
        // input indices put the G1 point first (0-1) and the G2 point after it (2-5) whichever is which
        const uint8_t* key = d_priv + priv_stride * lo;
        const uint8_t* u = d_u + usz * lo;
        const blsvm::Operand ops[2] = {
            {key, on_g2 ? blsvm::OPND_G1 : blsvm::OPND_G2, (uint32_t)priv_stride, on_g2 ? 0u : 2u, 0, 0},
            {u, on_g2 ? blsvm::OPND_G2 : blsvm::OPND_G1, (uint32_t)usz, on_g2 ? 2u : 0u, 0, 1}};
        KYB_TRY(blsvm::launch_prep(w, cnt, ops, 2, flags, nullptr, 0, st));
        KYB_TRY(blsvm::launch_pair(w, cnt, ws.gt, ws.pst, st));
        hipLaunchKernelGGL(bls12381_ibe_open_kernel, dim3(grid_for(cnt, 64)), dim3(64), 0, st, cnt, ws.gt, d_v + msg_len * lo,
                           d_w + msg_len * lo, len, ws.r, ws.m, ws.hst);
        KYB_HIP_CHECK(hipGetLastError());
        KYB_TRY(bls12381_fb_run(on_g2, cnt, ws.r, ws.base, ws.ru, nullptr, fb_flags(flags), st, nullptr));
        hipLaunchKernelGGL(bls12381_ibe_check_kernel, dim3(grid_for(cnt, 64)), dim3(64), 0, st, cnt, ws.pst, ws.hst, ws.ru, u,
                           (uint32_t)usz, ws.m, len, d_msgs + msg_len * lo, d_status ? d_status + lo : nullptr);
        KYB_HIP_CHECK(hipGetLastError());
    }
    return KYB_OK;
}

static int encrypt_dev(bool on_g2, const char* who, size_t n, const uint8_t* d_master, const uint8_t* d_id, size_t id_len,
                       const uint8_t* dst, size_t dst_len, const uint8_t* d_sigmas, const uint8_t* d_msgs, size_t msg_len,
                       uint8_t* d_u, uint8_t* d_v, uint8_t* d_w, uint8_t* d_status, uint32_t flags, hipStream_t st) {
    KYB_TRY(check_flags(flags, 1, true, who));
    if (msg_len > (size_t)MSG_MAX || dst_len > 255 || (dst_len && !dst) ||
        (n && (!d_master || (!d_id && id_len) || !d_u || ((!d_sigmas || !d_msgs || !d_v || !d_w) && msg_len)))) {
        set_error(std::string(who) + ": bad argument (msg_len 0..32, dst at most 255 bytes, non-null buffers)");
        return KYB_E_ARG;
    }
    if (!n) return KYB_OK;
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    const size_t usz = on_g2 ? bls::g2_out_size(flags) : bls::g1_out_size(flags);
    const int len = (int)msg_len;
    Ws ws;
    KYB_TRY(workspace(ctx, st, n < PIECE ? n : PIECE, &ws));
    KYB_TRY(base_point(ws, on_g2, st));
    {  // Gid = e(master, H(ID)) (OnG2: e(H(ID), master)), one lane; the master key in slot 0 (its status is the call's)
        blsvm::Work w;
        KYB_TRY(blsvm::workspace(ctx, st, 1, blsvm::PAIR_INPUTS, &w));
        const uint32_t msz = (uint32_t)(on_g2 ? bls::g2_wire_size(flags) : bls::g1_wire_size(flags));
        const blsvm::Operand ops[2] = {
            {d_master, on_g2 ? blsvm::OPND_G2 : blsvm::OPND_G1, msz, on_g2 ? 2u : 0u, 0, 0},
            {d_id ? d_id : d_master, on_g2 ? blsvm::OPND_G1_HASH : blsvm::OPND_G2_HASH, (uint32_t)id_len, on_g2 ? 0u : 2u, 0, 0}};
        KYB_TRY(blsvm::launch_prep(w, 1, ops, 2, flags & ~KYB_F_UNCOMPRESSED_OUT, dst, dst_len, st));
        KYB_TRY(blsvm::launch_pair(w, 1, ws.gid, ws.gid_st, st));
    }
    for (size_t lo = 0; lo < n; lo += PIECE) {
        const size_t cnt = n - lo < PIECE ? n - lo : PIECE;
        const uint8_t* sig = d_sigmas + msg_len * lo;
        hipLaunchKernelGGL(bls12381_ibe_seal_kernel, dim3(grid_for(cnt, 64)), dim3(64), 0, st, cnt, sig, d_msgs + msg_len * lo, len,
                           ws.r, d_w + msg_len * lo, ws.hst);
        KYB_HIP_CHECK(hipGetLastError());
        KYB_TRY(bls12381_fb_run(on_g2, cnt, ws.r, ws.base, d_u + usz * lo, nullptr, KYB_F_TRUSTED(0) | (flags & KYB_F_UNCOMPRESSED_OUT), st, nullptr));
        KYB_TRY(blsvm::gt_mul_strided(cnt, ws.r, ws.gid, 0, ws.gt, nullptr, st));
        hipLaunchKernelGGL(bls12381_ibe_mask_kernel, dim3(grid_for(cnt, 64)), dim3(64), 0, st, cnt, ws.gt, sig, len, ws.gid_st, ws.hst,
                           d_u + usz * lo, (uint32_t)usz, d_v + msg_len * lo, d_w + msg_len * lo, d_status ? d_status + lo : nullptr);
        KYB_HIP_CHECK(hipGetLastError());
    }
    return KYB_OK;
}

static int decrypt_host(bool on_g2, const char* who, size_t n, const uint8_t* priv, size_t priv_stride, const uint8_t* u, const uint8_t* v,
                        const uint8_t* w, size_t msg_len, uint8_t* msgs, uint8_t* status, uint32_t flags) {
    KYB_TRY(check_flags(flags, 2, false, who));
    const size_t ksz = on_g2 ? bls::g1_wire_size(flags) : bls::g2_wire_size(flags);
    const size_t usz = on_g2 ? bls::g2_wire_size(flags) : bls::g1_wire_size(flags);
    if (msg_len > (size_t)MSG_MAX || (priv_stride != 0 && priv_stride != ksz) ||
        (n && (!priv || !u || ((!v || !w || !msgs) && msg_len)))) {
        set_error(std::string(who) + ": bad argument (msg_len 0..32, private_stride 0 or the key's wire size, non-null buffers)");
        return KYB_E_ARG;
    }
    if (!n) return KYB_OK;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return decrypt_host(on_g2, who, hi - lo, priv + priv_stride * lo, priv_stride, u + usz * lo, v ? v + msg_len * lo : nullptr,
                                w ? w + msg_len * lo : nullptr, msg_len, msgs ? msgs + msg_len * lo : nullptr, status ? status + lo : nullptr,
                                flags);
        });
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    return staged_call(ctx, {{priv, priv_stride ? n * priv_stride : ksz}, {u, n * usz}, {v, n * msg_len}, {w, n * msg_len}},
                       {{msgs, n * msg_len}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return decrypt_dev(on_g2, who, n, (const uint8_t*)in[0], priv_stride, (const uint8_t*)in[1], (const uint8_t*)in[2],
                                              (const uint8_t*)in[3], msg_len, (uint8_t*)o[0], (uint8_t*)o[1], flags, st);
                       });
}

static int encrypt_host(bool on_g2, const char* who, size_t n, const uint8_t* master, const uint8_t* id, size_t id_len, const uint8_t* dst,
                        size_t dst_len, const uint8_t* sigmas, const uint8_t* msgs, size_t msg_len, uint8_t* u, uint8_t* v, uint8_t* w,
                        uint8_t* status, uint32_t flags) {
    KYB_TRY(check_flags(flags, 1, true, who));
    if (msg_len > (size_t)MSG_MAX || dst_len > 255 || (dst_len && !dst) ||
        (n && (!master || (!id && id_len) || !u || ((!sigmas || !msgs || !v || !w) && msg_len)))) {
        set_error(std::string(who) + ": bad argument (msg_len 0..32, dst at most 255 bytes, non-null buffers)");
        return KYB_E_ARG;
    }
    if (!n) return KYB_OK;
    const size_t usz = on_g2 ? bls::g2_out_size(flags) : bls::g1_out_size(flags);
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {  // every shard computes Gid itself
            return encrypt_host(on_g2, who, hi - lo, master, id, id_len, dst, dst_len, sigmas ? sigmas + msg_len * lo : nullptr,
                                msgs ? msgs + msg_len * lo : nullptr, msg_len, u + usz * lo, v ? v + msg_len * lo : nullptr,
                                w ? w + msg_len * lo : nullptr, status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    const size_t msz = on_g2 ? bls::g2_wire_size(flags) : bls::g1_wire_size(flags);
    const uint8_t none = 0;
    return staged_call(ctx, {{master, msz}, {id_len ? id : &none, id_len ? id_len : 1}, {sigmas, n * msg_len}, {msgs, n * msg_len}},
                       {{u, n * usz}, {v, n * msg_len}, {w, n * msg_len}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return encrypt_dev(on_g2, who, n, (const uint8_t*)in[0], (const uint8_t*)in[1], id_len, dst, dst_len,
                                              (const uint8_t*)in[2], (const uint8_t*)in[3], msg_len, (uint8_t*)o[0], (uint8_t*)o[1],
                                              (uint8_t*)o[2], (uint8_t*)o[3], flags, st);
                       });
}

}  // namespace ibe
}  // namespace kyb

using namespace kyb;

extern "C" {
int kyb_bls12381_ibe_encrypt_g1(size_t n, const uint8_t* master, const uint8_t* id, size_t id_len, const uint8_t* dst, size_t dst_len,
                                const uint8_t* sigmas, const uint8_t* msgs, size_t msg_len, uint8_t* u, uint8_t* v, uint8_t* w,
                                uint8_t* status, uint32_t flags) {
    return ibe::encrypt_host(false, "kyb_bls12381_ibe_encrypt_g1", n, master, id, id_len, dst, dst_len, sigmas, msgs, msg_len, u, v, w,
                             status, flags);
}
int kyb_bls12381_ibe_encrypt_g2(size_t n, const uint8_t* master, const uint8_t* id, size_t id_len, const uint8_t* dst, size_t dst_len,
                                const uint8_t* sigmas, const uint8_t* msgs, size_t msg_len, uint8_t* u, uint8_t* v, uint8_t* w,
                                uint8_t* status, uint32_t flags) {
    return ibe::encrypt_host(true, "kyb_bls12381_ibe_encrypt_g2", n, master, id, id_len, dst, dst_len, sigmas, msgs, msg_len, u, v, w,
                             status, flags);
}
int kyb_bls12381_ibe_decrypt_g1(size_t n, const uint8_t* privates, size_t private_stride, const uint8_t* u, const uint8_t* v,
                                const uint8_t* w, size_t msg_len, uint8_t* msgs, uint8_t* status, uint32_t flags) {
    return ibe::decrypt_host(false, "kyb_bls12381_ibe_decrypt_g1", n, privates, private_stride, u, v, w, msg_len, msgs, status, flags);
}
int kyb_bls12381_ibe_decrypt_g2(size_t n, const uint8_t* privates, size_t private_stride, const uint8_t* u, const uint8_t* v,
                                const uint8_t* w, size_t msg_len, uint8_t* msgs, uint8_t* status, uint32_t flags) {
    return ibe::decrypt_host(true, "kyb_bls12381_ibe_decrypt_g2", n, privates, private_stride, u, v, w, msg_len, msgs, status, flags);
}
int kyb_bls12381_ibe_encrypt_g1_dev(size_t n, const void* d_master, const void* d_id, size_t id_len, const uint8_t* dst, size_t dst_len,
                                    const void* d_sigmas, const void* d_msgs, size_t msg_len, void* d_u, void* d_v, void* d_w,
                                    void* d_status, uint32_t flags, void* stream) {
    return ibe::encrypt_dev(false, "kyb_bls12381_ibe_encrypt_g1_dev", n, (const uint8_t*)d_master, (const uint8_t*)d_id, id_len, dst,
                            dst_len, (const uint8_t*)d_sigmas, (const uint8_t*)d_msgs, msg_len, (uint8_t*)d_u, (uint8_t*)d_v,
                            (uint8_t*)d_w, (uint8_t*)d_status, flags, (hipStream_t)stream);
}
int kyb_bls12381_ibe_encrypt_g2_dev(size_t n, const void* d_master, const void* d_id, size_t id_len, const uint8_t* dst, size_t dst_len,
                                    const void* d_sigmas, const void* d_msgs, size_t msg_len, void* d_u, void* d_v, void* d_w,
                                    void* d_status, uint32_t flags, void* stream) {
    return ibe::encrypt_dev(true, "kyb_bls12381_ibe_encrypt_g2_dev", n, (const uint8_t*)d_master, (const uint8_t*)d_id, id_len, dst,
                            dst_len, (const uint8_t*)d_sigmas, (const uint8_t*)d_msgs, msg_len, (uint8_t*)d_u, (uint8_t*)d_v,
                            (uint8_t*)d_w, (uint8_t*)d_status, flags, (hipStream_t)stream);
}
int kyb_bls12381_ibe_decrypt_g1_dev(size_t n, const void* d_privates, size_t private_stride, const void* d_u, const void* d_v,
                                    const void* d_w, size_t msg_len, void* d_msgs, void* d_status, uint32_t flags, void* stream) {
    return ibe::decrypt_dev(false, "kyb_bls12381_ibe_decrypt_g1_dev", n, (const uint8_t*)d_privates, private_stride, (const uint8_t*)d_u,
                            (const uint8_t*)d_v, (const uint8_t*)d_w, msg_len, (uint8_t*)d_msgs, (uint8_t*)d_status, flags,
                            (hipStream_t)stream);
}
int kyb_bls12381_ibe_decrypt_g2_dev(size_t n, const void* d_privates, size_t private_stride, const void* d_u, const void* d_v,
                                    const void* d_w, size_t msg_len, void* d_msgs, void* d_status, uint32_t flags, void* stream) {
    return ibe::decrypt_dev(true, "kyb_bls12381_ibe_decrypt_g2_dev", n, (const uint8_t*)d_privates, private_stride, (const uint8_t*)d_u,
                            (const uint8_t*)d_v, (const uint8_t*)d_w, msg_len, (uint8_t*)d_msgs, (uint8_t*)d_status, flags,
                            (hipStream_t)stream);
}
}
