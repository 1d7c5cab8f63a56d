// sign/bdn on the pairing suites: the kernels for gfx950 over bdn.cuh's lane programs and the host functions behind the
// entry points kyb_<suite>_bdn_terms_<g> / kyb_<suite>_mask_aggregate_<g> (pairing_abi.cuh pastes the names).  A suite's
// *_bdn.hip includes this file, so the kernels are that unit's own and the other units keep theirs.
//
// Replaces, in the reference:
//   NewMask (hashPointToR, publicTerms)   mask.go:51-61, bdn.go:29-63   -> bdn_roster_kernel, bdn_root_kernel, bdn_terms_kernel
//   AggregatePublicKeys                   bdn.go:166-181                -> bdn_points_kernel, bdn_tables_kernel, bdn_total_kernel,
//                                                                          bdn_slices_kernel, bdn_fold_kernel, bdn_finish_kernel
// bdn_terms: a lane per key decodes and re-encodes it; ONE lane hashes the canonical roster (the root node is
// sequential); a lane per key then takes its half of an output node and runs the ladder.
// mask_aggregate: the points are decoded and the subset tables and T_all built ONCE per call into the (WS_BDN, stream)
// workspace; then, piece by piece, a lane per (mask, slice) sums its table entries into a partial sum, a wave per mask
// sums the S partial sums as a tree (S > 1 only), and a lane per mask finishes: T_all - acc for a flipped mask, one
// inversion, MarshalBinary.  Both calls run on the current device: they do not shard over a device set.
#pragma once
#include "bdn.cuh"
#include "context.h"

namespace kyb {

static_assert(BDN_MAX_ROSTER == KYB_COSI_MAX_ROSTER, "include/kyber_hip.h");

constexpr unsigned BDN_BUILD_BLOCK = 256;  // the table kernel: one group of 2^8 subsets, or sixteen of 2^4

// The slices kyb_bdn_debug_set_slices asked for (bdn_plan.hip; 0 = the plan's own): A/B runs of tools/bdn_probe.py
size_t bdn_forced_slices();

// ---- NewMask
// The (WS_BDN, stream) workspace of bdn_terms:  [ canon: m x POINT | h0: 32 B, then the roster's one flag | bad: m ]
struct BdnTermsWs {
    uint8_t* canon;
    uint32_t* h0;  // eight words, then any_bad at h0[8]
    uint8_t* bad;
};
constexpr size_t bdn_terms_ws_bytes(size_t m, size_t point) { return m * point + 64 + m; }

template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void bdn_roster_kernel(size_t m, const uint8_t* __restrict__ roster, uint8_t* __restrict__ canon,
                                                                      uint8_t* __restrict__ bad, uint8_t* __restrict__ status,
                                                                      uint32_t flags) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int st = bdn_roster_lane<G>(canon + G::POINT * j, roster + G::POINT * j, flags);
    bad[j] = (uint8_t)st;
    if (status) status[j] = (uint8_t)st;
}
// One block: the roster's flag by a vote, then -- in lane 0 alone -- the root hash over the canonical roster.
template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void bdn_root_kernel(size_t m, const uint8_t* __restrict__ canon, const uint8_t* __restrict__ bad,
                                                      uint32_t* __restrict__ h0) {
    int mine = 0;
    for (size_t j = threadIdx.x; j < m; j += blockDim.x) mine |= bad[j];
    const int any = __syncthreads_or(mine);
    if (threadIdx.x != 0) return;
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!any) blake2xs_root(h, canon, m * G::POINT);
#pragma unroll
    for (int i = 0; i < 8; i++) h0[i] = h[i];
    h0[8] = any ? 1u : 0u;
}
// One lane per key: its coefficient and its term, or zero bytes for every key of a roster with a rejected one.
template <class G>
__global__ __launch_bounds__(64, G::MUL_WAVES) void bdn_terms_kernel(size_t m, const uint8_t* __restrict__ canon, const uint32_t* __restrict__ h0,
                                                                     uint8_t* __restrict__ coefs, uint8_t* __restrict__ terms, uint32_t flags,
                                                                     uint32_t* __restrict__ tabs) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    uint32_t c[4] = {0, 0, 0, 0};
    if (h0[8]) {
        if (coefs) bdn_coef_bytes(coefs + 16 * j, c);
        uint32_t* q = reinterpret_cast<uint32_t*>(terms + G::POINT * j);
        for (size_t k = 0; k < G::POINT / 4; k++) q[k] = 0;
        return;
    }
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = h0[i];
    bdn_coef_lane(c, h, j);
    if (coefs) bdn_coef_bytes(coefs + 16 * j, c);
    bdn_term_lane<G>(terms + G::POINT * j, canon + G::POINT * j, c, flags, tabs + G::TAB_WORDS * j);
}

inline bool bdn_flags_bad(uint32_t flags) { return (flags & ~KYB_F_TRUSTED(0)) != 0; }
inline bool bdn_terms_args_bad(size_t m, const void* roster, const void* terms, uint32_t flags) {
    return bdn_flags_bad(flags) || m < 1 || m > BDN_MAX_ROSTER || !roster || !terms;
}
inline int bdn_bad_argument(const char* who, const char* rules) {
    set_error(std::string(who) + ": bad argument (" + rules + ")");
    return KYB_E_ARG;
}
#define KYB_BDN_TERMS_RULES "flags is 0 or KYB_F_TRUSTED(0); 1 <= m <= 8192; roster and terms"
#define KYB_BDN_AGG_RULES "flags is 0 or KYB_F_TRUSTED(0); 1 <= m <= 8192; mask_stride >= (m + 7) >> 3; points, masks and out"

template <class G>
int bdn_terms_dev(const char* who, size_t m, const void* d_roster, void* d_coefs, void* d_terms, void* d_status, uint32_t flags, void* stream) {
    if (bdn_terms_args_bad(m, d_roster, d_terms, flags)) return bdn_bad_argument(who, KYB_BDN_TERMS_RULES);
    const hipStream_t st = (hipStream_t)stream;
    DeviceCtx* ctx;
    if (int rc = get_ctx(&ctx)) return rc;
    std::lock_guard<std::recursive_mutex> enq(ctx->enq_mu);  // the workspace and the three kernels as one unit
    void* base;
    if (int rc = ctx_workspace(ctx, WS_BDN, st, bdn_terms_ws_bytes(m, G::POINT), &base)) return rc;
    BdnTermsWs w;
    w.canon = (uint8_t*)base;
    w.h0 = (uint32_t*)(w.canon + m * G::POINT);
    w.bad = (uint8_t*)(w.h0 + 16);
    uint32_t* tabs = nullptr;
    if (G::TAB_WORDS) {
        void* tw;
        if (int rc = ctx_workspace(ctx, G::WS_TAB, st, m * G::TAB_WORDS * sizeof(uint32_t), &tw)) return rc;
        tabs = (uint32_t*)tw;
    }
    const dim3 lanes((unsigned)((m + 63) / 64));
    hipLaunchKernelGGL(bdn_roster_kernel<G>, lanes, dim3(64), 0, st, m, (const uint8_t*)d_roster, w.canon, w.bad, (uint8_t*)d_status, flags);
    hipLaunchKernelGGL(bdn_root_kernel<G>, dim3(1), dim3(64), 0, st, m, (const uint8_t*)w.canon, (const uint8_t*)w.bad, w.h0);
    hipLaunchKernelGGL(bdn_terms_kernel<G>, lanes, dim3(64), 0, st, m, (const uint8_t*)w.canon, (const uint32_t*)w.h0, (uint8_t*)d_coefs,
                       (uint8_t*)d_terms, flags, tabs);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}
template <class G>
int bdn_terms_host(const char* who, size_t m, const uint8_t* roster, uint8_t* coefs, uint8_t* terms, uint8_t* status, uint32_t flags) {
    if (bdn_terms_args_bad(m, roster, terms, flags)) return bdn_bad_argument(who, KYB_BDN_TERMS_RULES);
    DeviceCtx* ctx;
    if (int rc = get_ctx(&ctx)) return rc;
    return staged_call(ctx, {{roster, m * G::POINT}}, {{coefs, m * 16}, {terms, m * G::POINT}, {status, m}},
                       [&](void* const* in, void* const* o, hipStream_t st) { return bdn_terms_dev<G>(who, m, in[0], o[0], o[1], o[2], flags, st); });
}

// ---- the masked sums
// The (WS_BDN, stream) workspace of mask_aggregate, E = sizeof(Jac<F>):
//   [ pts: m x E | tables: (groups << g) x E | T_all: E | tree: 64 x E | partial: min(n, BDN_PIECE) x S x E | bad: m, to 16 |
//     the points' one flag: 256 B ]
template <class F>
constexpr size_t bdn_agg_ws_bytes(size_t n, size_t m, int g, size_t S) {
    return (m + (((m + g - 1) / g) << g) + 1 + BDN_TREE + (n < BDN_PIECE ? n : BDN_PIECE) * S) * sizeof(Jac<F>) + (m + 15) / 16 * 16 + 256;
}

template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void bdn_points_kernel(size_t m, const uint8_t* __restrict__ points, Jac<typename G::F>* __restrict__ pts,
                                                                      uint8_t* __restrict__ bad, uint32_t flags) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    Jac<typename G::F> p;
    bad[j] = (uint8_t)bdn_point_lane<G>(p, points + G::POINT * j, flags);
    pts[j] = p;
}
// One lane per table entry, a block per 256 >> g groups.  Round k makes the entries whose highest point is k from the
// entries of the rounds before it, which the block's barrier has made visible: one addition per entry.
template <class G>
__global__ __launch_bounds__(BDN_BUILD_BLOCK, KYB_TU_WAVES) void bdn_tables_kernel(size_t m, int g, const Jac<typename G::F>* pts, Jac<typename G::F>* tables) {
    const size_t b = (size_t)blockIdx.x * (BDN_BUILD_BLOCK >> g) + (threadIdx.x >> g);
    const int s = (int)(threadIdx.x & ((1u << g) - 1u));
    const bool live = b < bdn_groups(m, g);
    if (live && s == 0) bdn_table_identity(tables, g, b);
    for (int k = 0; k < g; k++) {
        __syncthreads();
        if (live && (s >> k) == 1) bdn_table_round(tables, pts, m, g, b, s, k);
    }
}
// The tree of one wave over `tree`: slot t holds lane t's sum on entry, slot 0 the sum of the first `live` on exit.
template <class F>
__device__ void bdn_tree_reduce(Jac<F>* tree, unsigned t, unsigned live) {
    for (unsigned half = BDN_TREE / 2; half >= 1; half >>= 1) {
        __syncthreads();
        if (t < half && t + half < live) {
            Jac<F> a = tree[t], b = tree[t + half];
            bdn_combine(a, b);
            tree[t] = a;
        }
    }
    __syncthreads();
}
// One wave: T_all by a tree over its lanes, and the points' one flag: the status of the first rejected point.
template <class G>
__global__ __launch_bounds__(BDN_TREE, KYB_TU_WAVES) void bdn_total_kernel(size_t m, int g, const Jac<typename G::F>* tables, const uint8_t* __restrict__ bad,
                                                             Jac<typename G::F>* tree, Jac<typename G::F>* tall, uint32_t* __restrict__ flag) {
    __shared__ unsigned first;
    const unsigned t = threadIdx.x;
    if (t == 0) first = 0xffffffffu;
    __syncthreads();
    for (size_t j = t; j < m; j += BDN_TREE)
        if (bad[j]) {
            atomicMin(&first, (unsigned)j);
            break;
        }
    Jac<typename G::F> acc;
    bdn_total_partial(acc, tables, m, g, t, BDN_TREE);
    tree[t] = acc;
    bdn_tree_reduce(tree, t, BDN_TREE);
    if (t == 0) {
        *tall = tree[0];
        *flag = first == 0xffffffffu ? 0u : (uint32_t)bad[first];
    }
}
// One lane per (mask, slice): partial[i * S + s] = the sum of slice s's entries under mask i.
template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void bdn_slices_kernel(size_t n, size_t m, int g, size_t S, const uint8_t* __restrict__ masks,
                                                                      size_t mask_stride, const Jac<typename G::F>* __restrict__ tables,
                                                                      Jac<typename G::F>* __restrict__ partial) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= n * S) return;
    const size_t i = lane / S, s = lane % S;
    const uint8_t* mask = masks + i * mask_stride;
    const size_t nb = bdn_groups(m, g), per = bdn_slice_groups(nb, S);
    const size_t lo = s * per < nb ? s * per : nb, hi = lo + per < nb ? lo + per : nb;
    Jac<typename G::F> acc;
    bdn_slice_lane(acc, mask, m, g, bdn_mask_flips(bdn_mask_count(mask, m), m), tables, lo, hi);
    partial[lane] = acc;
}
// One wave per mask (S > 1): lane t sums the partial sums t, t + 64, ... into slot t, then the tree leaves the mask's
// sum in slot 0.  Lane t reads only the slots congruent to t before it writes slot t.
template <class G>
__global__ __launch_bounds__(BDN_TREE, KYB_TU_WAVES) void bdn_fold_kernel(size_t S, Jac<typename G::F>* partial) {
    Jac<typename G::F>* mine = partial + (size_t)blockIdx.x * S;
    const unsigned t = threadIdx.x;
    const unsigned live = S < (size_t)BDN_TREE ? (unsigned)S : (unsigned)BDN_TREE;
    if (t < live) {
        Jac<typename G::F> acc = mine[t];
        for (size_t s = (size_t)t + BDN_TREE; s < S; s += BDN_TREE) {
            Jac<typename G::F> o = mine[s];
            bdn_combine(acc, o);
        }
        mine[t] = acc;
    }
    bdn_tree_reduce(mine, t, live);
}
// One lane per mask: its sum's bytes, its count, the call's status.
template <class G>
__global__ __launch_bounds__(64, KYB_TU_WAVES) void bdn_finish_kernel(size_t n, size_t m, size_t S, const uint8_t* __restrict__ masks,
                                                                      size_t mask_stride, const Jac<typename G::F>* __restrict__ partial,
                                                                      const Jac<typename G::F>* __restrict__ tall, const uint32_t* __restrict__ flag,
                                                                      uint8_t* __restrict__ out, uint32_t* __restrict__ count,
                                                                      uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = bdn_mask_count(masks + i * mask_stride, m);
    const uint32_t bad = *flag;  // a rejected point is every element's (kyb_ed25519_mask_aggregate's rule)
    if (count) count[i] = cnt;
    if (status) status[i] = (uint8_t)bad;
    if (bad) {
        uint32_t* q = reinterpret_cast<uint32_t*>(out + G::POINT * i);
        for (size_t k = 0; k < G::POINT / 4; k++) q[k] = 0;
        return;
    }
    Jac<typename G::F> acc = partial[i * S], T = *tall;
    bdn_finish_lane<G>(out + G::POINT * i, acc, bdn_mask_flips(cnt, m), T);
}

inline bool bdn_agg_args_bad(size_t n, size_t m, const void* points, const void* masks, size_t mask_stride, const void* out, uint32_t flags) {
    if (bdn_flags_bad(flags) || m < 1 || m > BDN_MAX_ROSTER || mask_stride < ((m + 7) >> 3)) return true;
    return n != 0 && (!points || !masks || !out);
}

template <class G>
int bdn_aggregate_dev(const char* who, size_t n, size_t m, const void* d_points, const void* d_masks, size_t mask_stride, void* d_out,
                      void* d_count, void* d_status, uint32_t flags, void* stream) {
    using J = Jac<typename G::F>;
    if (bdn_agg_args_bad(n, m, d_points, d_masks, mask_stride, d_out, flags)) return bdn_bad_argument(who, KYB_BDN_AGG_RULES);
    if (n == 0) return KYB_OK;
    const hipStream_t st = (hipStream_t)stream;
    DeviceCtx* ctx;
    if (int rc = get_ctx(&ctx)) return rc;
    std::lock_guard<std::recursive_mutex> enq(ctx->enq_mu);  // the tables and the pieces as one unit
    const int g = bdn_group_width(n, m);
    const size_t nb = bdn_groups(m, g);
    size_t S = bdn_slices(n, m, g);
    if (const size_t forced = bdn_forced_slices()) {  // never more partial sums than two fills of the device
        const size_t piece = n < BDN_PIECE ? n : BDN_PIECE, cap = 2 * BDN_FILL / piece ? 2 * BDN_FILL / piece : 1;
        S = forced < nb ? forced : nb;
        if (S > cap) S = cap;
    }
    void* base;
    if (int rc = ctx_workspace(ctx, WS_BDN, st, bdn_agg_ws_bytes<typename G::F>(n, m, g, S), &base)) return rc;
    J* pts = (J*)base;
    J* tables = pts + m;
    J* tall = tables + (nb << g);
    J* tree = tall + 1;
    J* partial = tree + BDN_TREE;
    uint8_t* bad = (uint8_t*)(partial + (n < BDN_PIECE ? n : BDN_PIECE) * S);
    uint32_t* flag = (uint32_t*)(bad + (m + 15) / 16 * 16);
    const unsigned per_block = BDN_BUILD_BLOCK >> g;
    hipLaunchKernelGGL(bdn_points_kernel<G>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, m, (const uint8_t*)d_points, pts, bad, flags);
    hipLaunchKernelGGL(bdn_tables_kernel<G>, dim3((unsigned)((nb + per_block - 1) / per_block)), dim3(BDN_BUILD_BLOCK), 0, st, m, g,
                       (const J*)pts, tables);
    hipLaunchKernelGGL(bdn_total_kernel<G>, dim3(1), dim3(BDN_TREE), 0, st, m, g, (const J*)tables, (const uint8_t*)bad, tree, tall, flag);
    for (size_t lo = 0; lo < n; lo += BDN_PIECE) {
        const size_t cnt = n - lo < BDN_PIECE ? n - lo : BDN_PIECE;
        const uint8_t* masks = (const uint8_t*)d_masks + lo * mask_stride;
        hipLaunchKernelGGL(bdn_slices_kernel<G>, dim3((unsigned)((cnt * S + 63) / 64)), dim3(64), 0, st, cnt, m, g, S, masks, mask_stride,
                           (const J*)tables, partial);
        if (S > 1) hipLaunchKernelGGL(bdn_fold_kernel<G>, dim3((unsigned)cnt), dim3(BDN_TREE), 0, st, S, partial);
        hipLaunchKernelGGL(bdn_finish_kernel<G>, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st, cnt, m, S, masks, mask_stride,
                           (const J*)partial, (const J*)tall, (const uint32_t*)flag, (uint8_t*)d_out + lo * G::POINT,
                           d_count ? (uint32_t*)d_count + lo : nullptr, d_status ? (uint8_t*)d_status + lo : nullptr);
    }
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}
template <class G>
int bdn_aggregate_host(const char* who, size_t n, size_t m, const uint8_t* points, const uint8_t* masks, size_t mask_stride, uint8_t* out,
                       uint32_t* count, uint8_t* status, uint32_t flags) {
    if (bdn_agg_args_bad(n, m, points, masks, mask_stride, out, flags)) return bdn_bad_argument(who, KYB_BDN_AGG_RULES);
    if (n == 0) return KYB_OK;
    DeviceCtx* ctx;
    if (int rc = get_ctx(&ctx)) return rc;
    const size_t L = (m + 7) >> 3;  // the last element's mask ends the buffer: no stride of slack is read
    return staged_call(ctx, {{points, m * G::POINT}, {masks, (n - 1) * mask_stride + L}}, {{out, n * G::POINT}, {count, n * 4}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           return bdn_aggregate_dev<G>(who, n, m, in[0], in[1], mask_stride, o[0], o[1], o[2], flags, st);
                       });
}

}  // namespace kyb
