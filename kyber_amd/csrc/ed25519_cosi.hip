// Collective signatures on Ed25519 (sign/cosi): kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_cosi.cuh's; this unit is their kernels' own, so that the other Ed25519 units keep their kernels and their
// register allocation.
//
// Replaces, in the reference:
//   cosi Mask.SetMask / AggregatePublic / CountEnabled   cosi.go:300-317, 361-372   -> ed25519_cosi_roster_kernel,
//        ed25519_cosi_tables_kernel, ed25519_cosi_total_kernel, ed25519_cosi_aggregate_kernel, ed25519_cosi_encode_kernel
//   cosi Verify                                          cosi.go:214-232            -> the same five, then
//        ed25519_cosi_check_kernel and ed25519_cosi_verdict_kernel
// One call: the roster is decoded and the subset tables and T_all are built ONCE, into the (WS_ED_COSI, stream)
// workspace; then, piece by piece (ed_for_pieces), a lane per element sums its mask's table entries and parks
// (X, Y, Z), the shared-inversion encoder writes the aggregate's bytes, and -- for a verification -- a lane per element
// hashes, runs the ladder on -A taken from the parked triple with the comb for r B in the same accumulator, and a second
// encode pass compares with V on bytes.  The tables are read through the cache; a copy of a small roster's tables in LDS
// has not been measured against that.  Both calls run on the current device: they do not shard over a device set.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_launch.h"
#include "ed25519_cosi.cuh"

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT, "status values of include/kyber_hip.h");
static_assert(ED_COSI_MAX_ROSTER == KYB_COSI_MAX_ROSTER, "include/kyber_hip.h");

constexpr unsigned ED_COSI_BUILD_BLOCK = 256;  // the table and T_all kernels: one group of 2^8 subsets, or sixteen of 2^4

// One lane per roster key: the key decoded into the workspace, bad[j] != 0 where it has no x.
__global__ __launch_bounds__(64) void ed25519_cosi_roster_kernel(size_t m, const uint32_t* __restrict__ roster,
                                                                 int32_t* __restrict__ keys, uint8_t* __restrict__ bad) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    bad[j] = ed_cosi_roster_lane(keys + j * ED_COSI_KEY_WORDS, roster + 8 * j) ? 0 : 1;
}

// One lane per table entry, a block per 256 >> g groups.  Round k makes the entries whose highest key is k from the
// entries of the rounds before it, which the block's barrier has made visible: one addition per entry.
__global__ __launch_bounds__(ED_COSI_BUILD_BLOCK) void ed25519_cosi_tables_kernel(size_t m, int g, const int32_t* __restrict__ keys,
                                                                                  int4* tables) {
    const size_t b = (size_t)blockIdx.x * (ED_COSI_BUILD_BLOCK >> g) + (threadIdx.x >> g);
    const int s = (int)(threadIdx.x & ((1u << g) - 1u));
    const bool live = b < ed_cosi_groups(m, g);
    if (live && s == 0) ed_cosi_table_identity(tables, g, b);
    for (int k = 0; k < g; k++) {
        __syncthreads();
        if (live && (s >> k) == 1) ed_cosi_table_round(tables, keys, m, g, b, s, k);
    }
}

// One block: T_all by a tree over the block's lanes (partial sums in registers, handed over through LDS, limb-major so
// that a wave's access is 64 consecutive words), and the roster's one flag: any key that did not decode.
__global__ __launch_bounds__(ED_COSI_BUILD_BLOCK) void ed25519_cosi_total_kernel(size_t m, int g, const int4* __restrict__ tables,
                                                                                 const uint8_t* __restrict__ bad, int4* __restrict__ tall,
                                                                                 uint32_t* __restrict__ any_bad) {
    __shared__ int32_t sh[ED_COSI_KEY_WORDS * ED_COSI_BUILD_BLOCK];
    const unsigned t = threadIdx.x;
    int mine = 0;
    for (size_t j = t; j < m; j += ED_COSI_BUILD_BLOCK) mine |= bad[j];
    const int any = __syncthreads_or(mine);
    ge_p3 acc;
    ed_cosi_total_partial(acc, tables, m, g, t, ED_COSI_BUILD_BLOCK);
    for (unsigned half = ED_COSI_BUILD_BLOCK / 2; half >= 1; half >>= 1) {
        __syncthreads();
        if (t >= half && t < 2 * half) {
            int32_t w[ED_COSI_KEY_WORDS];
            ed_cosi_store_p3(w, acc);
#pragma unroll
            for (int l = 0; l < ED_COSI_KEY_WORDS; l++) sh[l * ED_COSI_BUILD_BLOCK + t] = w[l];
        }
        __syncthreads();
        if (t < half) {
            int32_t w[ED_COSI_KEY_WORDS];
#pragma unroll
            for (int l = 0; l < ED_COSI_KEY_WORDS; l++) w[l] = sh[l * ED_COSI_BUILD_BLOCK + t + half];
            ge_p3 o;
            ed_cosi_load_p3(o, w);
            ed_cosi_total_combine(acc, o);
        }
    }
    if (t == 0) {
        ge_cached c;
        ge_p3_to_cached(c, acc);
        TabGlobal out{tall};
        out.put(0, c);
        *any_bad = any ? 1u : 0u;
    }
}

// One lane per element.  Lanes past n repeat element n - 1 (the skip of a group is a wave's decision) and store
// nothing.  count: n words, or nullptr.
__global__ __launch_bounds__(128, 3) void ed25519_cosi_aggregate_kernel(size_t n, size_t m, int g, const uint8_t* __restrict__ masks,
                                                                         size_t mask_stride, const int4* __restrict__ tables,
                                                                         const int4* __restrict__ tall,
                                                                         const uint32_t* __restrict__ any_bad, int32_t* __restrict__ proj,
                                                                         uint8_t* __restrict__ st, uint32_t* __restrict__ count) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    ge_p3 acc;
    const uint32_t cnt = ed_cosi_aggregate_lane(acc, masks + idx * mask_stride, m, g, tables, tall);
    if (lane >= n) return;
    const bool bad = *any_bad != 0;  // a wrong roster key is every element's (kyb_ed25519_mul_same_base's rule)
    if (bad) ge_p3_0(acc);
    store_proj(proj, idx, acc);
    st[idx] = bad ? KYB_ST_BAD_POINT : KYB_ST_OK;
    if (count) count[idx] = cnt;
}

// The aggregate keys' bytes, one inversion per ENC_CHUNK parked points; the parked triples are only read.  abytes: the
// slab's copy for the check lanes; out, status: the caller's, each may be null.  Zero bytes where the status is not 0.
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_cosi_encode_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                         const uint8_t* __restrict__ st,
                                                                                         uint32_t* __restrict__ abytes,
                                                                                         uint32_t* __restrict__ out,
                                                                                         uint8_t* __restrict__ status) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        const uint8_t s = st[i];
        if (s) {
#pragma unroll
            for (int k = 0; k < 8; k++) w[k] = 0;
        }
        if (abytes) store_words8(abytes + i * 8, w);
        if (out) store_words8(out + i * 8, w);
        if (status) status[i] = s;
    });
}

// One lane per cosignature; reads its parked aggregate and parks T over it.  Lanes past n repeat element n - 1 and
// store nothing but their window table, which the slab has room for (whole blocks).
__global__ __launch_bounds__(128, 3) void ed25519_cosi_check_kernel(size_t n, const uint32_t* __restrict__ abytes,
                                                                     const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ sigs, const int32_t* __restrict__ wide,
                                                                     sf::Mod m, int32_t* proj, const uint8_t* __restrict__ st,
                                                                     int4* __restrict__ gtab) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    uint32_t aw[8], vw[8], rw[8];
    load_words8(aw, abytes + idx * 8);
    load_words8(vw, sigs + idx * 16);
    load_words8(rw, sigs + idx * 16 + 8);
    const uint64_t lo = off[idx], hi = off[idx + 1];
    const size_t len = hi >= lo ? (size_t)(hi - lo) : 0;
    TabGlobal tab{gtab + lane * 80};
    ge_p3 T;
    ed_cosi_check_lane(T, vw, rw, aw, proj + idx * ED_PROJ_LIMBS, msgs + lo, len, wide, m, tab);
    if (lane >= n) return;
    if (st[idx]) ge_p3_0(T);
    store_proj(proj, idx, T);
}

// ok[i] = status 0 and encode(T_i) == canon(V_i), one inversion per ENC_CHUNK cosignatures
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_cosi_verdict_kernel(size_t n, const int32_t* __restrict__ proj,
                                                                                          const uint8_t* __restrict__ st,
                                                                                          const uint32_t* __restrict__ sigs,
                                                                                          uint8_t* __restrict__ ok) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        uint32_t v[8], cv[8];
        load_words8(v, sigs + i * 16);
        ed_canon_point_bytes(cv, v);
        ok[i] = (st[i] == KYB_ST_OK && ed_words8_equal(cv, w)) ? 1 : 0;
    });
}

struct CosiArgs {
    size_t m;
    const void *roster, *msgs, *off, *sigs, *masks;
    size_t mask_stride;
    void *agg, *count, *ok, *status;
    bool verify;
};

// The (WS_ED_COSI, stream) workspace of a call:  [ keys: m x 160 B | tables: (groups << g) x 160 B | T_all: 160 B |
// bad: m bytes, then the one flag ].  At g = 8 and 8 192 keys the tables take 42 MB.
constexpr size_t ed_cosi_ws_bytes(size_t m, int g) {
    return m * 160 + ((m + g - 1) / g << g) * 160 + 160 + (m + 15) / 16 * 16 + 256;
}
static_assert(ed_cosi_ws_bytes(ED_COSI_MAX_ROSTER, 8) < (size_t(45) << 20) && ed_cosi_ws_bytes(ED_COSI_MAX_ROSTER, 4) < (size_t(8) << 20),
              "42 MB of tables at the widest roster");

static bool cosi_args_bad(size_t n, const CosiArgs& a, uint32_t flags) {
    if (flags) return true;
    if (a.m < 1 || a.m > ED_COSI_MAX_ROSTER) return true;
    if (a.mask_stride < ((a.m + 7) >> 3)) return true;
    if (n == 0) return false;
    if (!a.roster || !a.masks) return true;
    return a.verify ? (!a.ok || !a.sigs || !a.off) : !a.agg;
}

static int launch_cosi(size_t n, const CosiArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the tables and the pieces as one unit
    const size_t m = a.m;
    const int g = ed_cosi_group_width(n, m);
    const size_t nb = ed_cosi_groups(m, g);
    void* base;
    if ((rc = ctx_workspace(ctx, WS_ED_COSI, st, ed_cosi_ws_bytes(m, g), &base))) return rc;
    int32_t* keys = (int32_t*)base;
    int4* tables = (int4*)((uint8_t*)base + m * 160);
    int4* tall = tables + (nb << g) * ED_COSI_ENTRY_INT4;
    uint8_t* bad = (uint8_t*)(tall + ED_COSI_ENTRY_INT4);
    uint32_t* any_bad = (uint32_t*)(bad + (m + 15) / 16 * 16);
    const unsigned per_block = ED_COSI_BUILD_BLOCK >> g;
    hipLaunchKernelGGL(ed25519_cosi_roster_kernel, ed_grid(m, 64), dim3(64), 0, st, m, (const uint32_t*)a.roster, keys,
                       bad);
    hipLaunchKernelGGL(ed25519_cosi_tables_kernel, ed_grid(nb, per_block), dim3(ED_COSI_BUILD_BLOCK), 0, st,
                       m, g, (const int32_t*)keys, tables);
    hipLaunchKernelGGL(ed25519_cosi_total_kernel, dim3(1), dim3(ED_COSI_BUILD_BLOCK), 0, st, m, g, (const int4*)tables,
                       (const uint8_t*)bad, tall, any_bad);
    KYB_HIP_CHECK(hipGetLastError());
    return ed_for_pieces(n, st, a.verify ? ED_SLAB_COSI_VERIFY : ED_SLAB_COSI_AGGREGATE,
                         [&](DeviceCtx* c, size_t lo, size_t cnt, const EdSlab& w) {
                             const dim3 lanes = ed_grid(cnt, ED_TAB_BLOCK);
                             hipLaunchKernelGGL(ed25519_cosi_aggregate_kernel, lanes, dim3(ED_TAB_BLOCK), 0, st, cnt, m, g,
                                                (const uint8_t*)a.masks + lo * a.mask_stride, a.mask_stride, (const int4*)tables,
                                                (const int4*)tall, (const uint32_t*)any_bad, w.proj, w.status,
                                                a.count ? (uint32_t*)a.count + lo : nullptr);
                             hipLaunchKernelGGL(ed25519_cosi_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                                                (const int32_t*)w.proj, (const uint8_t*)w.status, a.verify ? w.digits : nullptr,
                                                a.agg ? (uint32_t*)a.agg + lo * 8 : nullptr,
                                                a.status ? (uint8_t*)a.status + lo : nullptr);
                             if (!a.verify) return;
                             const uint32_t* sigs = (const uint32_t*)a.sigs + lo * 16;
                             hipLaunchKernelGGL(ed25519_cosi_check_kernel, lanes, dim3(ED_TAB_BLOCK), 0, st, cnt, (const uint32_t*)w.digits,
                                                (const uint8_t*)a.msgs, (const uint64_t*)a.off + lo, sigs, (const int32_t*)c->ed_wide_tab,
                                                ed_order(), w.proj, (const uint8_t*)w.status, w.gtab);
                             hipLaunchKernelGGL(ed25519_cosi_verdict_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                                                (const int32_t*)w.proj, (const uint8_t*)w.status, sigs, (uint8_t*)a.ok + lo);
                         });
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_cosi_group_width(size_t n, size_t m) { return ed_cosi_group_width(n, m); }

int kyb_ed25519_mask_aggregate_dev(size_t n, size_t m, const void* d_roster, const void* d_masks, size_t mask_stride, void* d_out,
                                   void* d_count, void* d_status, uint32_t flags, void* stream) {
    const CosiArgs a{m, d_roster, nullptr, nullptr, nullptr, d_masks, mask_stride, d_out, d_count, nullptr, d_status, false};
    if (int rc; ed_entry_done(&rc, n, cosi_args_bad(n, a, flags), "kyb_ed25519_mask_aggregate_dev: bad argument")) return rc;
    return launch_cosi(n, a, (hipStream_t)stream);
}

int kyb_ed25519_mask_aggregate(size_t n, size_t m, const uint8_t* roster, const uint8_t* masks, size_t mask_stride, uint8_t* out,
                               uint32_t* count, uint8_t* status, uint32_t flags) {
    const CosiArgs a{m, roster, nullptr, nullptr, nullptr, masks, mask_stride, out, count, nullptr, status, false};
    if (int rc; ed_entry_done(&rc, n, cosi_args_bad(n, a, flags),
                              "kyb_ed25519_mask_aggregate: bad argument (flags must be 0; 1 <= m <= 8192; mask_stride >= (m + 7) >> 3; "
                              "roster, masks and out)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const size_t L = (m + 7) >> 3;  // the last element's mask ends the buffer: no stride of slack is read
    return staged_call(ctx, {{roster, m * 32}, {masks, (n - 1) * mask_stride + L}}, {{out, n * 32}, {count, n * 4}, {status, n}},
                       [&](void* const* in, void* const* o, hipStream_t st) {
                           CosiArgs d = a;
                           d.roster = in[0];
                           d.masks = in[1];
                           d.agg = o[0];
                           d.count = o[1];
                           d.status = o[2];
                           return launch_cosi(n, d, st);
                       });
}

int kyb_ed25519_cosi_verify_dev(size_t n, size_t m, const void* d_roster, const void* d_msgs, const void* d_msg_off,
                                const void* d_sigs, const void* d_masks, size_t mask_stride, void* d_agg, void* d_count, void* d_ok,
                                void* d_status, uint32_t flags, void* stream) {
    const CosiArgs a{m, d_roster, d_msgs, d_msg_off, d_sigs, d_masks, mask_stride, d_agg, d_count, d_ok, d_status, true};
    if (int rc; ed_entry_done(&rc, n, cosi_args_bad(n, a, flags) || (n && !d_msgs), "kyb_ed25519_cosi_verify_dev: bad argument")) return rc;
    return launch_cosi(n, a, (hipStream_t)stream);
}

int kyb_ed25519_cosi_verify(size_t n, size_t m, const uint8_t* roster, const uint8_t* msgs, const uint64_t* msg_off,
                            const uint8_t* sigs, const uint8_t* masks, size_t mask_stride, uint8_t* agg, uint32_t* count, uint8_t* ok,
                            uint8_t* status, uint32_t flags) {
    const CosiArgs a{m, roster, msgs, msg_off, sigs, masks, mask_stride, agg, count, ok, status, true};
    if (int rc; ed_entry_done(&rc, n, cosi_args_bad(n, a, flags),
                              "kyb_ed25519_cosi_verify: bad argument (flags must be 0; 1 <= m <= 8192; mask_stride >= (m + 7) >> 3; "
                              "roster, offsets, sigs, masks and ok)"))
        return rc;
    if (EdHostSpans::offsets_bad(n, msgs, msg_off)) {
        set_error("kyb_ed25519_cosi_verify: bad argument (message offsets must not decrease, nor name bytes of a NULL msgs)");
        return KYB_E_ARG;
    }
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const EdHostSpans sp(n, msgs, msg_off);
    const size_t L = (m + 7) >> 3;
    // (msgs may be null when every message is empty: a present input of zero bytes)
    return staged_call(ctx,
                       {{roster, m * 32},
                        {sp.base, sp.total},
                        {sp.offsets(), sp.offsets_bytes()},
                        {sigs, n * 64},
                        {masks, (n - 1) * mask_stride + L}},
                       {{agg, n * 32}, {count, n * 4}, {ok, n}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           CosiArgs d = a;
                           d.roster = in[0];
                           d.msgs = in[1];
                           d.off = in[2];
                           d.sigs = in[3];
                           d.masks = in[4];
                           d.agg = o[0];
                           d.count = o[1];
                           d.ok = o[2];
                           d.status = o[3];
                           return launch_cosi(n, d, st);
                       });
}
}
