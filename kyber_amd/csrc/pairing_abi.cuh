// Batch kernels + C-ABI entry points shared by the pairing suites (BLS12-381, bn256, bn254), written once as templates
// over a suite policy S and a group policy G (S::G1 / S::G2: the end of bls12381.cuh and of bn_suite.inc): one kernel per
// operation -- one group operation per lane, one wave per workgroup -- and the host / device-pointer functions behind the
// entry points kyb_<pfx>_* of include/kyber_hip.h.  The macros at the end of the file only paste those names: each
// entry point is one call of a template with its own name (`who`) for the messages.  Pair / ValidatePairing are NOT
// per-lane code: each suite's *_pair.hip supplies the `_dev` entry points on the cooperative tower machine
// (tower_vm.cuh) and pair_host / pair_check_host add the host-buffer ones.
#pragma once
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>

#include "context.h"
#include "fixed_base.cuh"

#define KYB_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

namespace kyb {
static inline unsigned grid_for(size_t n, int block) { return (unsigned)((n + block - 1) / block); }
inline int bad_argument(const char* who) {
    set_error(std::string(who) + ": bad argument");
    return KYB_E_ARG;
}

// ---- same-base batches: when does the fixed-base table (fixed_base.cuh) take over?
// from this many scalars a table is worth building for an unknown base (KYB_FB_MIN overrides both; 0 disables the path)
static inline size_t fb_min_batch(bool g2) {
    static const long forced = [] {
        const char* e = getenv("KYB_FB_MIN");
        return e ? atol(e) : -1L;
    }();
    if (forced == 0) return ~size_t(0);
    if (forced > 0) return (size_t)forced;
    (void)g2;
    return size_t(1) << 17;  // measured break-even, table build included: ~1e5 (G1) / ~0.5e5-0.9e5 (G2) scalars
}
constexpr size_t FB_MIN_KNOWN = 64;  // ... and from this many when the table is (about to be) there anyway
// Host entry points stage through the per-device pool of context.h (staged_call; StageScope / StageBuf where a wrapper
// does work of its own between the copies).

// Register budget of fb::mul_kernel in waves per SIMD (a suite's translation unit may set it before including this file)
#ifndef KYB_FB_G1_WAVES
#define KYB_FB_G1_WAVES 2
#endif
#ifndef KYB_FB_G2_WAVES
#define KYB_FB_G2_WAVES 2
#endif
// The fixed-base traits (fixed_base.cuh) of group G of suite S.
template <class S, class G>
struct FbTraits {
    using F = typename G::F;
    using P = typename G::Fb;
    static constexpr int MUL_WAVES = G::IS_G2 ? KYB_FB_G2_WAVES : KYB_FB_G1_WAVES;
    static constexpr int KIND = WS_FB + 2 * S::FB_SUITE + (G::IS_G2 ? 1 : 0);
    // fixed_base.cuh chain_rows_kernel: the table's doubling chain on rowfp.cuh -- G1 only, where the base field has its limb shape
    static constexpr int ROW_CHAIN = (!G::IS_G2 && S::FC::N == 13 && S::FC::W == 30) ? 1 : 0;
    using RowC = typename S::FC;
    static constexpr uint32_t KEY_FLAGS = KYB_F_UNCOMPRESSED | KYB_F_TRUSTED(0);
    __host__ __device__ static int decode_on_curve(Aff<F>& a, const uint8_t* in, uint32_t flags) { return P::decode_on_curve(a, in, flags); }
    __host__ __device__ static bool needs_member(uint32_t flags) { return P::needs_member(flags); }
    __device__ static bool member(const Aff<F>& a, const fb::Entry<F, P::NI>* tab) { return P::member(a, tab); }
    __host__ __device__ static void encode(uint8_t* out, const Aff<F>& a, uint32_t flags) { G::encode(out, a, flags); }
    __host__ __device__ static size_t wire_size(uint32_t flags) { return G::wire_size(flags); }
    __host__ __device__ static size_t out_size(uint32_t flags) { return G::out_size(flags); }
    __host__ __device__ static void scalar(uint32_t (&k)[8], const uint8_t* in) { G::scalar_from_be(k, in); }
    static void generator(Aff<F>& a) { G::generator(a); }
};
// the suite generator's wire form under `flags` (host side): a same-base batch over it is worth a table at any size
template <class G>
static std::string fb_generator_key(uint32_t flags) {
    Aff<typename G::F> g;
    G::generator(g);
    uint8_t buf[fb::WIRE_MAX];
    // the INPUT form the flags select: compressed unless KYB_F_UNCOMPRESSED
    G::encode(buf, g, (flags & KYB_F_UNCOMPRESSED) ? KYB_F_UNCOMPRESSED_OUT : 0u);
    return std::string((const char*)buf, G::wire_size(flags));
}
// Runs a same-base batch through the traits.  KYB_FB_EXTERN (set by a suite's scalar-multiplication unit before including
// this file): only declared here and instantiated in a translation unit of its own (bls12381_fb.hip), whose kernels then
// share no out-of-line code -- and no register budget -- with this unit's.
#ifdef KYB_FB_EXTERN
template <class S, class G>
int fb_run(size_t n, const void* d_scalars, const void* d_points, void* d_out, void* d_status, uint32_t flags, hipStream_t st, const std::string* key);
#else
template <class S, class G>
int fb_run(size_t n, const void* d_scalars, const void* d_points, void* d_out, void* d_status, uint32_t flags, hipStream_t st, const std::string* key) {
    return fb::run<FbTraits<S, G>>(n, d_scalars, d_points, d_out, d_status, flags, st, key);
}
#endif

// ---- kernels
// tabs: a slab of G::TAB_WORDS words per lane for the ladder's window tables (groups that keep them in global memory:
// BLS12-381 G1, the BN suites' G2), indexed by the lane's position in THIS launch
template <class G>
__global__ __launch_bounds__(64, G::MUL_WAVES) void group_mul_kernel(size_t n, const uint8_t* __restrict__ scalars, const uint8_t* __restrict__ pts,
                                                          size_t pt_stride, uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                          uint32_t flags, const uint8_t* __restrict__ only, uint32_t* __restrict__ tabs) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    if (only && !only[idx]) return;  // the lane machine did this element (bls12381_lvm.cuh step 4)
    const int st = G::mul_wire(out + G::out_size(flags) * idx, scalars + 32 * idx, pts + pt_stride * idx, flags, tabs + G::TAB_WORDS * idx);
    if (status) status[idx] = (uint8_t)st;
}
template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void group_unmarshal_kernel(size_t n, const uint8_t* __restrict__ pts, uint8_t* __restrict__ out,
                                                                uint8_t* __restrict__ status, uint32_t flags) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int st = G::unmarshal_wire(out + G::out_size(flags) * idx, pts + G::wire_size(flags) * idx, flags);
    if (status) status[idx] = (uint8_t)st;
}
template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void group_add_kernel(size_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                          uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int st = G::add_wire(out + G::POINT * idx, a + G::POINT * idx, b + G::POINT * idx);
    if (status) status[idx] = (uint8_t)st;
}

// ---- UnmarshalBinary, Point.Add
template <class S, class G>
int unmarshal_dev(const char* who, size_t n, const void* d_points, void* d_out, void* d_status, uint32_t flags, void* stream) {
    KYB_TRY(check_flags(flags, 1, true, who));
    if (n && (!d_points || !d_out)) return bad_argument(who);
    if (!n) return KYB_OK;
    bool small = false;  // the suite's small-batch kernel took it (BLS12-381: cooperating lanes)
    KYB_TRY(S::unmarshal_small(G::IS_G2, n, (const uint8_t*)d_points, (uint8_t*)d_out, (uint8_t*)d_status, flags, (hipStream_t)stream, &small));
    if (small) return KYB_OK;
    hipLaunchKernelGGL(group_unmarshal_kernel<G>, dim3(grid_for(n, 64)), dim3(64), 0, (hipStream_t)stream, n, (const uint8_t*)d_points,
                       (uint8_t*)d_out, (uint8_t*)d_status, flags);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}
template <class S, class G>
int unmarshal_host(const char* who, size_t n, const uint8_t* points, uint8_t* out, uint8_t* status, uint32_t flags) {
    KYB_TRY(check_flags(flags, 1, true, who));
    if (n && (!points || !out)) return bad_argument(who);
    if (!n) return KYB_OK;
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    return staged_call(ctx, {{points, n * G::wire_size(flags)}}, {{out, n * G::out_size(flags)}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return unmarshal_dev<S, G>(who, n, in[0], o[0], o[1], flags, st); });
}
template <class G>
int add_dev(const char* who, size_t n, const void* d_a, const void* d_b, void* d_out, void* d_status, void* stream) {
    if (n && (!d_a || !d_b || !d_out)) return bad_argument(who);
    if (!n) return KYB_OK;
    hipLaunchKernelGGL(group_add_kernel<G>, dim3(grid_for(n, 64)), dim3(64), 0, (hipStream_t)stream, n, (const uint8_t*)d_a, (const uint8_t*)d_b,
                       (uint8_t*)d_out, (uint8_t*)d_status);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}
template <class G>
int add_host(const char* who, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* status) {
    if (n && (!a || !b || !out)) return bad_argument(who);
    if (!n) return KYB_OK;
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    return staged_call(ctx, {{a, n * G::POINT}, {b, n * G::POINT}}, {{out, n * G::POINT}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return add_dev<G>(who, n, in[0], in[1], o[0], o[1], st); });
}

// ---- scalar multiplication
// Lanes per launch of a group whose ladder keeps its tables in the per-lane slab: the slab is sized by one piece
// (KYB_MUL_PIECE overrides it: tests)
inline size_t mul_piece() {
    static const size_t piece = [] {
        const char* e = getenv("KYB_MUL_PIECE");
        const long long v = e ? atoll(e) : 0;
        return v > 0 ? (size_t)v : size_t(1) << 20;
    }();
    return piece;
}
template <class S, class G>
int mul_dev(const char* who, size_t n, const void* d_scalars, const void* d_points, size_t point_stride, void* d_out, void* d_status,
            uint32_t flags, void* stream) {
    KYB_TRY(check_flags(flags, 1, true, who));
    if ((n && (!d_scalars || !d_points || !d_out)) || (point_stride != 0 && point_stride != G::wire_size(flags))) return bad_argument(who);
    if (!n) return KYB_OK;
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t *scalars = (const uint8_t*)d_scalars, *points = (const uint8_t*)d_points;
    uint8_t *out = (uint8_t*)d_out, *status = (uint8_t*)d_status;
    if (point_stride == 0 && n >= fb_min_batch(G::IS_G2))  // one base, many scalars: fixed_base.cuh
        return fb_run<S, G>(n, d_scalars, d_points, d_out, d_status, flags, st, nullptr);
    // the machine's steps and the per-lane redo launches are ONE unit on the stream: `only` points into the (WS_LVM,
    // stream) workspace, which another thread's call on the same stream may rewrite or grow (enq_mu is recursive)
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    std::lock_guard<std::recursive_mutex> enq(ctx->enq_mu);
    const uint8_t* only = nullptr;
    bool handled = false;  // the suite's hook did the whole batch (BLS12-381: the small-batch kernels on cooperating lanes)
    KYB_TRY(S::lvm_mul(G::IS_G2, n, scalars, points, point_stride, out, status, flags, st, &only, &handled));
    if (handled) return KYB_OK;
    // The per-lane table slab is the (G::WS_TAB, stream) workspace, one piece's worth: a larger launch -- the redo launch
    // after the lane machine covers all n lanes, whatever n is -- goes through it in pieces (stream-ordered: a piece's
    // kernel has read its tables before the next one writes them), each with its part of the redo mask.
    size_t piece = n;
    uint32_t* tabs = nullptr;
    if (G::TAB_WORDS) {
        piece = std::min(n, mul_piece());
        void* tw;
        KYB_TRY(ctx_workspace(ctx, G::WS_TAB, st, piece * G::TAB_WORDS * sizeof(uint32_t), &tw));
        tabs = (uint32_t*)tw;
    }
    const size_t osz = G::out_size(flags);
    for (size_t off = 0; off < n; off += piece) {
        const size_t cnt = std::min(piece, n - off);
        hipLaunchKernelGGL(group_mul_kernel<G>, dim3(grid_for(cnt, 64)), dim3(64), 0, st, cnt, scalars + 32 * off, points + point_stride * off,
                           point_stride, out + osz * off, status ? status + off : nullptr, flags, only ? only + off : nullptr, tabs);
    }
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}
// stride: 0 = every scalar multiplies points[0] (Mul(s, nil), PriPoly.Commit); anything else = one point per scalar.
// (`who` also names the device-pointer calls made from here: their own checks have passed by then.)
template <class S, class G>
int mul_host(const char* who, size_t n, const uint8_t* scalars, const uint8_t* points, size_t stride, uint8_t* out, uint8_t* status,
             uint32_t flags) {
    KYB_TRY(check_flags(flags, 1, true, who));
    const size_t psz = G::out_size(flags), isz = G::wire_size(flags);
    if (stride) stride = isz;
    if (n && (!scalars || !points || !out)) return bad_argument(who);
    if (!n) return KYB_OK;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return mul_host<S, G>(who, hi - lo, scalars + 32 * lo, points + (stride ? isz * lo : 0), stride, out + psz * lo,
                                  status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    StageScope sc(ctx);
    StageBuf s, p, o, st;
    KYB_TRY(s.upload(scalars, n * 32));
    KYB_TRY(p.upload(points, (stride ? n : 1) * isz));
    KYB_TRY(o.alloc(n * psz));
    KYB_TRY(st.alloc(n));
    if (!stride && fb_min_batch(G::IS_G2) != ~size_t(0)) {
        // same base: the fixed-base table takes the batch when it is large, or from FB_MIN_KNOWN scalars when the
        // table is there already (the base of the previous such call on this device) or is the suite's generator
        std::string key((const char*)points, isz);
        key.push_back((char)(flags & 0xff));
        key.push_back((char)((flags >> 8) & 0xff));
        bool use = n >= fb_min_batch(G::IS_G2);
        if (!use && n >= FB_MIN_KNOWN) {
            use = fb_hint_is(ctx, FbTraits<S, G>::KIND, sc.stream(), key);
            if (!use) {
                const std::string gk = fb_generator_key<G>(flags);
                use = gk.size() == isz && memcmp(gk.data(), points, isz) == 0;
            }
        }
        if (use) {
            KYB_TRY((fb_run<S, G>(n, s.p, p.p, o.p, st.p, flags, sc.stream(), &key)));
            KYB_TRY(o.download(out, n * psz));
            if (status) KYB_TRY(st.download(status, n));
            return KYB_OK;
        }
    }
    if (!stride && n >= (size_t(1) << 18) && !(flags & KYB_F_TRUSTED(0)) && G::decode_proves_subgroup()) {
        // one shared base and MANY coefficients (PriPoly.Commit): UnmarshalBinary's checks run once, in one lane, and
        // the lanes take the point as validated.  A lone lane needs as long for them (~2 ms on BLS12-381 G1) as a full
        // chip of lanes does side by side, so this pays only once every SIMD has several waves to run one after the
        // other (measured: 2^16 coefficients 6.0 ms per-lane against 6.9 ms this way; from 2^18 on it wins).  Not for a G2
        // base of a suite whose UnmarshalBinary does not prove subgroup membership (bn256): there TRUSTED selects the GLS
        // walk, which differs from the reference's double-and-add on off-subgroup points whatever n is
        KYB_TRY((unmarshal_dev<S, G>(who, 1, p.p, o.p, st.p, flags & ~KYB_F_UNCOMPRESSED_OUT, sc.stream())));
        uint8_t st0 = 0;
        KYB_HIP_CHECK(hipMemcpy(&st0, st.p, 1, hipMemcpyDeviceToHost));
        if (st0) {
            memset(out, 0, n * psz);
            if (status) memset(status, st0, n);
            return KYB_OK;
        }
        flags |= KYB_F_TRUSTED(0);
    }
    KYB_TRY((mul_dev<S, G>(who, n, s.p, p.p, stride, o.p, st.p, flags, sc.stream())));
    KYB_TRY(o.download(out, n * psz));
    if (status) KYB_TRY(st.download(status, n));
    return KYB_OK;
}

// ---- GT exponentiation: the suite's GTMUL program on the tower machine (its *_pair translation unit defines `enqueue`)
using GtMulEnqueue = int (*)(size_t n, const uint8_t* d_scalars, const uint8_t* d_gt, uint8_t* d_out, uint8_t* d_status, hipStream_t st);
inline int gt_mul_dev(const char* who, GtMulEnqueue enqueue, size_t n, const void* d_scalars, const void* d_gt, void* d_out, void* d_status,
                      void* stream) {
    if (n && (!d_scalars || !d_gt || !d_out)) return bad_argument(who);
    if (!n) return KYB_OK;
    return enqueue(n, (const uint8_t*)d_scalars, (const uint8_t*)d_gt, (uint8_t*)d_out, (uint8_t*)d_status, (hipStream_t)stream);
}
template <class S>
int gt_mul_host(const char* who, GtMulEnqueue enqueue, size_t n, const uint8_t* scalars, const uint8_t* gt, uint8_t* out, uint8_t* status) {
    if (n && (!scalars || !gt || !out)) return bad_argument(who);
    if (!n) return KYB_OK;
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    return staged_call(ctx, {{scalars, n * 32}, {gt, n * S::GT_SIZE}}, {{out, n * S::GT_SIZE}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return gt_mul_dev(who, enqueue, n, in[0], in[1], o[0], o[1], st); });
}

// ---- Pair / ValidatePairing on host buffers: stage and call the suite's own `_dev` entry points (the tower machine)
using PairDev = int (*)(size_t n, const void* d_g1, const void* d_g2, void* d_gt, void* d_status, uint32_t flags, void* stream);
using PairCheckDev = int (*)(size_t n, const void* d_p1, const void* d_p2, const void* d_inv1, const void* d_inv2, void* d_ok, void* d_status,
                             uint32_t flags, void* stream);
template <class S>
int pair_host(const char* who, PairDev dev, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, uint8_t* status, uint32_t flags) {
    KYB_TRY(check_flags(flags, 2, false, who));
    if (n && (!g1 || !g2 || !gt)) return bad_argument(who);
    if (!n) return KYB_OK;
    const size_t s1 = S::G1::wire_size(flags), s2 = S::G2::wire_size(flags);
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return pair_host<S>(who, dev, hi - lo, g1 + s1 * lo, g2 + s2 * lo, gt + S::GT_SIZE * lo, status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    return staged_call(ctx, {{g1, n * s1}, {g2, n * s2}}, {{gt, n * S::GT_SIZE}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return dev(n, in[0], in[1], o[0], o[1], flags, st); });
}
template <class S>
int pair_check_host(const char* who, PairCheckDev dev, size_t n, const uint8_t* p1, const uint8_t* p2, const uint8_t* inv1, const uint8_t* inv2,
                    uint8_t* ok, uint8_t* status, uint32_t flags) {
    KYB_TRY(check_flags(flags, 4, false, who));
    if (n && (!p1 || !p2 || !inv1 || !inv2 || !ok)) return bad_argument(who);
    if (!n) return KYB_OK;
    const size_t s1 = S::G1::wire_size(flags), s2 = S::G2::wire_size(flags);
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {
            return pair_check_host<S>(who, dev, hi - lo, p1 + s1 * lo, p2 + s2 * lo, inv1 + s1 * lo, inv2 + s2 * lo, ok + lo,
                                      status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    KYB_TRY(get_ctx(&ctx));
    return staged_call(ctx, {{p1, n * s1}, {p2, n * s2}, {inv1, n * s1}, {inv2, n * s2}}, {{ok, n}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return dev(n, in[0], in[1], in[2], in[3], o[0], o[1], flags, st); });
}
}  // namespace kyb

// ---- the exported names.  PFX: bls12381 / bn256 / bn254; S: the suite policy; g / G: g1, G1 or g2, G2.
#define KYB_EXPORT_GROUP_ABI(PFX, S, g, G) \
extern "C" { \
int kyb_##PFX##_##g##_mul_dev(size_t n, const void* d_scalars, const void* d_points, size_t point_stride, void* d_out, void* d_status, uint32_t flags, void* stream) { \
    return kyb::mul_dev<S, S::G>("kyb_" #PFX "_" #g "_mul_dev", n, d_scalars, d_points, point_stride, d_out, d_status, flags, stream); \
} \
int kyb_##PFX##_##g##_mul(size_t n, const uint8_t* scalars, const uint8_t* points, uint8_t* out, uint8_t* status, uint32_t flags) { \
    return kyb::mul_host<S, S::G>("kyb_" #PFX "_g*_mul", n, scalars, points, S::G::POINT, out, status, flags); \
} \
int kyb_##PFX##_##g##_mul_same_base(size_t n, const uint8_t* scalars, const uint8_t* point, uint8_t* out, uint8_t* status, uint32_t flags) { \
    return kyb::mul_host<S, S::G>("kyb_" #PFX "_g*_mul", n, scalars, point, 0, out, status, flags); \
} \
int kyb_##PFX##_##g##_unmarshal_dev(size_t n, const void* d_points, void* d_out, void* d_status, uint32_t flags, void* stream) { \
    return kyb::unmarshal_dev<S, S::G>("kyb_" #PFX "_" #g "_unmarshal_dev", n, d_points, d_out, d_status, flags, stream); \
} \
int kyb_##PFX##_##g##_unmarshal(size_t n, const uint8_t* points, uint8_t* out, uint8_t* status, uint32_t flags) { \
    return kyb::unmarshal_host<S, S::G>("kyb_" #PFX "_g*_unmarshal", n, points, out, status, flags); \
} \
int kyb_##PFX##_##g##_add_dev(size_t n, const void* d_a, const void* d_b, void* d_out, void* d_status, void* stream) { \
    return kyb::add_dev<S::G>("kyb_" #PFX "_" #g "_add_dev", n, d_a, d_b, d_out, d_status, stream); \
} \
int kyb_##PFX##_##g##_add(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* status) { \
    return kyb::add_host<S::G>("kyb_" #PFX "_g*_add", n, a, b, out, status); \
} \
}
#define KYB_EXPORT_MUL_ABI(PFX, S) KYB_EXPORT_GROUP_ABI(PFX, S, g1, G1) KYB_EXPORT_GROUP_ABI(PFX, S, g2, G2)

// (kyb::PFX_gt_mul_enqueue: the suite's *_pair translation unit)
#define KYB_EXPORT_GT_ABI(PFX, S) \
extern "C" { \
int kyb_##PFX##_gt_mul_dev(size_t n, const void* d_scalars, const void* d_gt, void* d_out, void* d_status, void* stream) { \
    return kyb::gt_mul_dev("kyb_" #PFX "_gt_mul_dev", kyb::PFX##_gt_mul_enqueue, n, d_scalars, d_gt, d_out, d_status, stream); \
} \
int kyb_##PFX##_gt_mul(size_t n, const uint8_t* scalars, const uint8_t* gt, uint8_t* out, uint8_t* status) { \
    return kyb::gt_mul_host<S>("kyb_" #PFX "_gt_mul", kyb::PFX##_gt_mul_enqueue, n, scalars, gt, out, status); \
} \
}
#define KYB_EXPORT_PAIR_HOST(PFX, S) \
extern "C" { \
int kyb_##PFX##_pair(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, uint8_t* status, uint32_t flags) { \
    return kyb::pair_host<S>("kyb_" #PFX "_pair", kyb_##PFX##_pair_dev, n, g1, g2, gt, status, flags); \
} \
int kyb_##PFX##_pair_check(size_t n, const uint8_t* p1, const uint8_t* p2, const uint8_t* inv1, const uint8_t* inv2, uint8_t* ok, uint8_t* status, uint32_t flags) { \
    return kyb::pair_check_host<S>("kyb_" #PFX "_pair_check", kyb_##PFX##_pair_check_dev, n, p1, p2, inv1, inv2, ok, status, flags); \
} \
}

// sign/bdn (bdn_launch.cuh, which a suite's *_bdn unit includes before it pastes these names): NewMask's coefficients and
// terms over one roster, and the masked sums over them; g / G as above.
#define KYB_EXPORT_BDN_GROUP_ABI(PFX, S, g, G) \
extern "C" { \
int kyb_##PFX##_bdn_terms_##g##_dev(size_t m, const void* d_roster, void* d_coefs, void* d_terms, void* d_status, uint32_t flags, void* stream) { \
    return kyb::bdn_terms_dev<S::G>("kyb_" #PFX "_bdn_terms_" #g "_dev", m, d_roster, d_coefs, d_terms, d_status, flags, stream); \
} \
int kyb_##PFX##_bdn_terms_##g(size_t m, const uint8_t* roster, uint8_t* coefs, uint8_t* terms, uint8_t* status, uint32_t flags) { \
    return kyb::bdn_terms_host<S::G>("kyb_" #PFX "_bdn_terms_" #g, m, roster, coefs, terms, status, flags); \
} \
int kyb_##PFX##_mask_aggregate_##g##_dev(size_t n, size_t m, const void* d_points, const void* d_masks, size_t mask_stride, void* d_out, void* d_count, void* d_status, uint32_t flags, void* stream) { \
    return kyb::bdn_aggregate_dev<S::G>("kyb_" #PFX "_mask_aggregate_" #g "_dev", n, m, d_points, d_masks, mask_stride, d_out, d_count, d_status, flags, stream); \
} \
int kyb_##PFX##_mask_aggregate_##g(size_t n, size_t m, const uint8_t* points, const uint8_t* masks, size_t mask_stride, uint8_t* out, uint32_t* count, uint8_t* status, uint32_t flags) { \
    return kyb::bdn_aggregate_host<S::G>("kyb_" #PFX "_mask_aggregate_" #g, n, m, points, masks, mask_stride, out, count, status, flags); \
} \
}
#define KYB_EXPORT_BDN_ABI(PFX, S) KYB_EXPORT_BDN_GROUP_ABI(PFX, S, g1, G1) KYB_EXPORT_BDN_GROUP_ABI(PFX, S, g2, G2)
