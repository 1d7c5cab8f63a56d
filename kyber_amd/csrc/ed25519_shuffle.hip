// Neff verifiable shuffles on Ed25519: kernels for gfx950 + their C-ABI entry points.  The lane programs are
// ed25519_shuffle.cuh's; this unit is their kernels' own, so that ed25519.o, ed25519_verify.o, ed25519_dleq.o and
// ed25519_ring.o keep their kernels and their register allocation.
//
// Replaces, in the reference:
//   proof hashVerifier.PubRand / hashProver.PubRand  hash.go:68-75, 111-142 -> ed25519_xof_count_kernel, _scan_kernel, _scatter_kernel
//   suite.Read of []kyber.Scalar from an XOF          rand.go:19-46, scalar.go:180-184 over blake.go:47-49 -> the same
//   shuffle thver, SimpleShuffle.Verify step 5         simple.go:178-183, 225-242 -> ed25519_theta_kernel + ed25519_theta_encode_kernel
// n sequential Picks become three launches over a fixed window of ed_xof_window(n) candidate draws: accept flags counted
// per wave, an exclusive scan of the wave totals by one workgroup, and a scatter that recomputes each draw (a node is
// one compression) and stores the accepted ones at their rank.  No workgroup waits on another: the order between the
// three passes is the stream's.  The theta kernel keeps two window tables per lane in the global slab (TabGlobal) and
// parks (X, Y, Z) for the shared-inversion encoder, where the verdict is taken; batches run in pieces of ED_PIECE lanes
// (ed25519_launch.h: ED_SLAB_THETA and the piece loop).
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_shuffle.cuh"
#include "ed25519_launch.h"

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT, "status values of include/kyber_hip.h");

// One wave per block: the wave's ballot is the block's, and its population count the block's total.
constexpr unsigned ED_XOF_BLOCK = 64;
constexpr unsigned ED_XOF_SCAN_BLOCK = 256;  // the one workgroup of the scan; each lane owns a run of consecutive totals

// accept flag (and value) of candidate draw j; lanes past the window hold no draw
__device__ __forceinline__ bool xof_lane_draw(uint32_t (&c)[8], uint64_t w, const uint64_t* __restrict__ root, uint64_t pos,
                                              uint64_t j) {
    if (j >= w) return false;
    uint64_t m[16];
    ed_xof_root_block(m, root);
    return ed_xof_draw(c, m, pos, j);
}

// totals[block] = accepted draws among the block's 64 candidates
__global__ __launch_bounds__(ED_XOF_BLOCK) void ed25519_xof_count_kernel(uint64_t w, const uint64_t* __restrict__ root,
                                                                         uint64_t pos, uint32_t* __restrict__ totals) {
    uint32_t c[8];
    const bool acc = xof_lane_draw(c, w, root, pos, (uint64_t)blockIdx.x * ED_XOF_BLOCK + threadIdx.x);
    const unsigned long long ballot = __ballot(acc);
    if (threadIdx.x == 0) totals[blockIdx.x] = (uint32_t)__popcll(ballot);
}

// totals[0 .. nblocks) -> their exclusive prefix sums, in place; totals[nblocks] = the sum.  One workgroup: lane t sums
// the run [t * per, (t + 1) * per), the 256 run sums are scanned in LDS, and the lane writes its run's prefixes.
__global__ __launch_bounds__(ED_XOF_SCAN_BLOCK) void ed25519_xof_scan_kernel(uint32_t nblocks, uint32_t* __restrict__ totals) {
    __shared__ uint32_t part[ED_XOF_SCAN_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nblocks + ED_XOF_SCAN_BLOCK - 1) / ED_XOF_SCAN_BLOCK;
    const uint64_t lo64 = (uint64_t)t * per;
    const uint32_t lo = lo64 < nblocks ? (uint32_t)lo64 : nblocks;
    const uint32_t hi = lo64 + per < nblocks ? (uint32_t)(lo64 + per) : nblocks;
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += totals[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < ED_XOF_SCAN_BLOCK; d <<= 1) {  // inclusive scan of the run sums
        const uint32_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t v = totals[i];
        totals[i] = run;
        run += v;
    }
    if (t == ED_XOF_SCAN_BLOCK - 1) totals[nblocks] = part[t];
}

// out[rank] = the accepted draw of that rank, for ranks below n; draws_used = 1 + the index of the draw of rank n - 1.
// A window with fewer than n accepted draws: out zeroed, draws_used = 0 (n <= w, so lanes 0 .. n - 1 exist).
__global__ __launch_bounds__(ED_XOF_BLOCK) void ed25519_xof_scatter_kernel(uint64_t n, uint64_t w, const uint64_t* __restrict__ root,
                                                                           uint64_t pos, const uint32_t* __restrict__ prefix,
                                                                           uint32_t nblocks, uint32_t* __restrict__ out,
                                                                           uint64_t* __restrict__ draws_used) {
    const uint64_t j = (uint64_t)blockIdx.x * ED_XOF_BLOCK + threadIdx.x;
    uint32_t c[8];
    const bool acc = xof_lane_draw(c, w, root, pos, j);
    const unsigned long long ballot = __ballot(acc);
    if (prefix[nblocks] < n) {
        if (j < n) {
            const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            store_words8(out + j * 8, z);
        }
        if (j == 0) *draws_used = 0;
        return;
    }
    const uint64_t rank = (uint64_t)prefix[blockIdx.x] + (uint64_t)__popcll(ballot & ((1ull << threadIdx.x) - 1ull));
    if (acc && rank < n) {
        store_words8(out + rank * 8, c);
        if (rank == n - 1) *draws_used = j + 1;
    }
}

// One lane per element.  Lanes past n repeat element n - 1 (the variable-time chain's wave reductions want every lane)
// and store nothing.  U, W: nullptr or one point shared by the batch.  table slab: 2 x 80 int4 per lane.
__global__ __launch_bounds__(128, 3) void ed25519_theta_kernel(
    size_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ A, const uint32_t* __restrict__ U,
    const uint32_t* __restrict__ b, const uint32_t* __restrict__ B, const uint32_t* __restrict__ W, uint32_t flags, sf::Mod m,
    int32_t* __restrict__ proj, uint8_t* __restrict__ st, int4* __restrict__ gtab) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    uint32_t aw[8], Aw[8], bw[8], Bw[8];
    load_words8(aw, a + idx * 8);
    load_words8(Aw, A + idx * 8);
    load_words8(bw, b + idx * 8);
    load_words8(Bw, B + idx * 8);
    TabGlobal tp{gtab + lane * 160}, tq{gtab + lane * 160 + 80};
    ge_p3 h;
    const int s = ed_theta_lane(h, aw, Aw, U, bw, Bw, W, (flags & KYB_F_VARTIME) != 0, m, tp, tq);
    if (lane >= n) return;
    store_proj(proj, idx, h);
    st[idx] = (uint8_t)s;
}

// ok[i] = status 0 and encode(h_i) == canon(T_i), one inversion per ENC_CHUNK parked points
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_theta_encode_kernel(
    size_t n, const int32_t* __restrict__ proj, const uint8_t* __restrict__ st, const uint32_t* __restrict__ T,
    uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        uint32_t v[8], cv[8];
        load_words8(v, T + i * 8);
        ed_canon_point_bytes(cv, v);
        const uint8_t s = st[i];
        ok[i] = (s == KYB_ST_OK && ed_words8_equal(cv, w)) ? 1 : 0;
        if (status) status[i] = s;
    });
}

static const sf::Mod& theta_order() {
    static const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    return m;
}

// The window must exist: W(n) draws counted in 32 bits (so n stays below about 2^31), every draw inside the 2^32 output
// nodes a BLAKE2Xb stream has (the node offset is 32 bits wide).
static bool xof_args_bad(size_t n, const void* root, uint64_t pos, const void* out, const void* draws_used) {
    if (!draws_used) return true;
    if (n == 0) return false;
    if (!root || !out) return true;
    if (n > (uint64_t(1) << 31)) return true;
    const uint64_t w = ed_xof_window(n);
    constexpr uint64_t STREAM_BYTES = uint64_t(1) << 38;  // 2^32 nodes of 64 bytes
    return w > 0xffffffffull || pos > STREAM_BYTES || 32 * w > STREAM_BYTES - pos;
}

static int launch_xof_pick(size_t n, const void* d_root, uint64_t pos, void* d_out, void* d_draws_used, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    const uint64_t w = ed_xof_window(n);
    const uint32_t nblocks = (uint32_t)((w + ED_XOF_BLOCK - 1) / ED_XOF_BLOCK);
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the workspace and its kernels as one unit
    void* ws;
    if ((rc = ctx_workspace(ctx, WS_ED, st, ((size_t)nblocks + 1) * sizeof(uint32_t), &ws))) return rc;
    uint32_t* totals = (uint32_t*)ws;
    hipLaunchKernelGGL(ed25519_xof_count_kernel, dim3(nblocks), dim3(ED_XOF_BLOCK), 0, st, w, (const uint64_t*)d_root, pos, totals);
    KYB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ed25519_xof_scan_kernel, dim3(1), dim3(ED_XOF_SCAN_BLOCK), 0, st, nblocks, totals);
    KYB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ed25519_xof_scatter_kernel, dim3(nblocks), dim3(ED_XOF_BLOCK), 0, st, (uint64_t)n, w,
                       (const uint64_t*)d_root, pos, (const uint32_t*)totals, nblocks, (uint32_t*)d_out, (uint64_t*)d_draws_used);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}

struct ThetaArgs {
    const void *a, *A, *U, *b, *B, *W, *T;
    void *ok, *status;
    uint32_t flags;
};

static bool theta_args_bad(size_t n, const ThetaArgs& t) {
    if (t.flags & ~KYB_F_VARTIME) return true;  // KYB_F_UNIFORM: no scanned Straus chain
    return n && (!t.a || !t.A || !t.b || !t.B || !t.T || !t.ok);
}

static int launch_theta(size_t n, const ThetaArgs& t, hipStream_t st) {
    return ed_for_pieces(n, st, ED_SLAB_THETA, [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
        const uint32_t* T = (const uint32_t*)t.T + lo * 8;
        hipLaunchKernelGGL(ed25519_theta_kernel, ed_grid(cnt, 128), dim3(128), 0, st, cnt,
                           (const uint32_t*)t.a + lo * 8, (const uint32_t*)t.A + lo * 8, (const uint32_t*)t.U,
                           (const uint32_t*)t.b + lo * 8, (const uint32_t*)t.B + lo * 8, (const uint32_t*)t.W, t.flags,
                           theta_order(), w.proj, w.status, w.gtab);
        hipLaunchKernelGGL(ed25519_theta_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                           (const int32_t*)w.proj, (const uint8_t*)w.status, T, (uint8_t*)t.ok + lo,
                           t.status ? (uint8_t*)t.status + lo : nullptr);
    });
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_xof_pick_dev(size_t n, const void* d_root, uint64_t pos, void* d_out, void* d_draws_used, void* stream) {
    // (the caller's draws_used is device memory: an empty call touches no device)
    if (int rc; ed_entry_done(&rc, n, xof_args_bad(n, d_root, pos, d_out, d_draws_used), "kyb_ed25519_xof_pick_dev: bad argument"))
        return rc;
    return launch_xof_pick(n, d_root, pos, d_out, d_draws_used, (hipStream_t)stream);
}

int kyb_ed25519_xof_pick(size_t n, const uint8_t root[64], uint64_t pos, uint8_t* out, uint64_t* draws_used) {
    if (xof_args_bad(n, root, pos, out, draws_used)) {
        set_error("kyb_ed25519_xof_pick: bad argument");
        return KYB_E_ARG;
    }
    *draws_used = 0;
    if (n == 0) return KYB_OK;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    rc = staged_call(ctx, {{root, 64}}, {{out, n * 32}, {draws_used, sizeof(uint64_t)}},
                     [&](void* const* in, void* const* o, hipStream_t st) { return launch_xof_pick(n, in[0], pos, o[0], o[1], st); });
    if (rc) return rc;
    if (*draws_used == 0) {
        set_error("kyb_ed25519_xof_pick: the window of 2n + 16 ceil(sqrt n) + 256 draws held fewer than n scalars below l");
        return KYB_E_EXHAUSTED;
    }
    return KYB_OK;
}

int kyb_ed25519_theta_check_dev(size_t n, const void* d_a, const void* d_A, const void* d_U, const void* d_b, const void* d_B,
                                const void* d_W, const void* d_T, void* d_ok, void* d_status, uint32_t flags, void* stream) {
    const ThetaArgs t{d_a, d_A, d_U, d_b, d_B, d_W, d_T, d_ok, d_status, flags};
    if (int rc; ed_entry_done(&rc, n, theta_args_bad(n, t), "kyb_ed25519_theta_check_dev: bad argument")) return rc;
    return launch_theta(n, t, (hipStream_t)stream);
}

int kyb_ed25519_theta_check(size_t n, const uint8_t* a, const uint8_t* A, const uint8_t* U, const uint8_t* b, const uint8_t* B,
                            const uint8_t* W, const uint8_t* T, uint8_t* ok, uint8_t* status, uint32_t flags) {
    if (int rc; ed_entry_done(&rc, n, theta_args_bad(n, ThetaArgs{a, A, U, b, B, W, T, ok, status, flags}),
                              "kyb_ed25519_theta_check: bad argument")) return rc;
    if (md_active(n))
        return md_run(n, [&](int, size_t lo, size_t hi) {  // U and W go to every shard
            return kyb_ed25519_theta_check(hi - lo, a + 32 * lo, A + 32 * lo, U, b + 32 * lo, B + 32 * lo, W, T + 32 * lo, ok + lo,
                                           status ? status + lo : nullptr, flags);
        });
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx, {{a, n * 32}, {A, n * 32}, {U, 32, /*absent=*/!U}, {b, n * 32}, {B, n * 32}, {W, 32, /*absent=*/!W}, {T, n * 32}},
                       {{ok, n}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_theta(n, ThetaArgs{in[0], in[1], in[2], in[3], in[4], in[5], in[6], o[0], o[1], flags}, st);
                       });
}
}
