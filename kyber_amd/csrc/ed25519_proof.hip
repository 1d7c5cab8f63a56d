// proof predicates on Ed25519 (proof/proof.go, proof/hash.go): kernels for gfx950 + their C-ABI entry points.  The lane
// programs are ed25519_proof.cuh's; this unit is their kernels' own, so that the other Ed25519 units keep their kernels
// and their register allocation.
//
// Replaces, in the reference:
//   proof repPred.commit / verify   proof.go:203-237, 298-322   -> ed25519_lincomb_tables_kernel, ed25519_lincomb_kernel,
//                                                                   ed25519_lincomb_encode_kernel
//   proof hashVerifier.PubRand      hash.go:111-142             -> ed25519_fs_challenge_kernel
// A linear combination is three launches: the points the batch shares are decoded and their window tables built once
// per call, one lane per table, into the (WS_ED_PROOF, stream) workspace; the lane kernel keeps the tables of its own
// points and every scalar's parked digits in the (WS_ED, stream) slab (ed25519_launch.h, ed_slab_lincomb) and reads the
// shared tables through the cache -- a copy per workgroup in LDS has not been measured against it; the shared-inversion
// encoder writes the bytes and takes the verdict against expect.  Both calls run on the current device: they do not
// shard over a device set.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "context.h"
#include "ed25519_launch.h"
#include "ed25519_proof.cuh"

#include <vector>

namespace kyb {

static_assert(ED_ST_OK == KYB_ST_OK && ED_ST_BAD_POINT == KYB_ST_BAD_POINT && ED_ST_PICK_EXHAUSTED == KYB_ST_PICK_EXHAUSTED,
              "status values of include/kyber_hip.h");

// Table j of the call's shared points, one lane per table: the standard base's where bit j of nil_mask is set (the 32
// bytes are then not read), else shared[j]'s; bad[j] != 0 where that point does not decode.
__global__ __launch_bounds__(64) void ed25519_lincomb_tables_kernel(size_t ks, const uint32_t* __restrict__ shared, uint32_t nil_mask,
                                                                    int4* __restrict__ tabs, uint8_t* __restrict__ bad) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ks) return;
    bad[j] = ed_lincomb_shared_table(tabs + 80 * j, shared + 8 * j, (nil_mask >> j) & 1u) ? 0 : 1;
}

// One lane per element.  Lanes past n repeat element n - 1 (the variable-time chain's wave reductions want every lane)
// and store nothing but their tables and digits, which the slab has room for (whole blocks).  gtab: ko x 80 int4 per
// lane; digits: a block's (ko + ks) x 8 words per lane, interleaved over the block's lanes.
__global__ __launch_bounds__(128, 3) void ed25519_lincomb_kernel(size_t n, int ko, int ks, uint32_t nil_mask,
                                                                  const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ own,
                                                                  const int4* __restrict__ sh_tab, const uint8_t* __restrict__ sh_bad,
                                                                  uint32_t flags, int32_t* __restrict__ proj, uint8_t* __restrict__ st,
                                                                  int4* __restrict__ gtab, uint32_t* __restrict__ digits) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t idx = lane < n ? lane : n - 1;
    const size_t K = (size_t)(ko + ks);
    const EdLincombMem mem{gtab + lane * 80 * (size_t)ko, sh_tab, digits + (size_t)blockIdx.x * blockDim.x * 8 * K + threadIdx.x,
                           blockDim.x};
    ge_p3 h;
    bool ok = ed_lincomb_lane(h, ko, ks, nil_mask, scalars + idx * 8 * K, own + idx * 8 * (size_t)ko, (flags & KYB_F_VARTIME) != 0, mem);
    if (lane >= n) return;
    for (int j = 0; j < ks; j++) ok &= sh_bad[j] == 0;  // a wrong shared point is every element's
    if (!ok) ge_p3_0(h);
    store_proj(proj, idx, h);
    st[idx] = ok ? KYB_ST_OK : KYB_ST_BAD_POINT;
}

// out[i] = the encoding (zero bytes where the status is not 0), ok[i] = status 0 and encoding == canon(expect[i]); one
// inversion per ENC_CHUNK parked points.  out, or expect and ok, may be null.
__global__ __launch_bounds__(ED_ENC_BLOCK, KYB_TU_WAVES) void ed25519_lincomb_encode_kernel(
    size_t n, const int32_t* __restrict__ proj, const uint8_t* __restrict__ st, const uint32_t* __restrict__ expect,
    uint32_t* __restrict__ out, uint8_t* __restrict__ ok, uint8_t* __restrict__ status) {
    EncPreScratch pre;
    ed_encode_chunk(n, proj, ed_encode_first(), blockDim.x, pre, [&](size_t i, uint32_t(&w)[8]) {
        const uint8_t s = st[i];
        if (s) {
#pragma unroll
            for (int k = 0; k < 8; k++) w[k] = 0;
        }
        if (out) store_words8(out + i * 8, w);
        if (ok) {
            uint32_t v[8], cv[8];
            load_words8(v, expect + i * 8);
            ed_canon_point_bytes(cv, v);
            ok[i] = (s == KYB_ST_OK && ed_words8_equal(cv, w)) ? 1 : 0;
        }
        if (status) status[i] = s;
    });
}

// One lane per proof; nothing here is wave-collective, so lanes past n simply leave.  off: n + 1 offsets into names,
// or nullptr when every proof has the one name of name_len bytes.  A pair of offsets that decreases is an empty name.
__global__ __launch_bounds__(64, KYB_TU_WAVES) void ed25519_fs_challenge_kernel(size_t n, const uint8_t* __restrict__ names,
                                                                                const uint64_t* __restrict__ off, size_t name_len,
                                                                                const uint8_t* __restrict__ data, size_t data_len,
                                                                                uint32_t* __restrict__ c, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* name = names;
    size_t len = name_len;
    if (off) {
        const uint64_t lo = off[i], hi = off[i + 1];
        name = names + lo;
        len = hi >= lo ? (size_t)(hi - lo) : 0;
    }
    uint32_t cw[8];
    const int s = ed_fs_challenge_lane(cw, name, len, data + i * data_len, data_len);
    store_words8(c + i * 8, cw);
    if (status) status[i] = (uint8_t)s;
}

struct LincombArgs {
    size_t ko, ks;
    const void *scalars, *own, *shared;
    uint32_t nil_mask;
    const void* expect;
    void *out, *ok, *status;
    uint32_t flags;
};

static bool lincomb_args_bad(size_t n, const LincombArgs& a) {
    if (a.flags & ~KYB_F_VARTIME) return true;  // KYB_F_UNIFORM: no scanned Straus chain
    if (a.ko + a.ks < 1 || a.ko > (size_t)ED_LINCOMB_MAX_OWN || a.ks > (size_t)ED_LINCOMB_MAX_SHARED) return true;
    if (a.nil_mask >> a.ks) return true;
    if ((a.expect != nullptr) != (a.ok != nullptr)) return true;
    if (!a.out && !a.ok) return true;
    if ((a.own != nullptr) != (a.ko != 0) || (a.shared != nullptr) != (a.ks != 0)) return true;
    return n && !a.scalars;
}

static int launch_lincomb(size_t n, const LincombArgs& a, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);  // the shared tables and the pieces as one unit
    const size_t K = a.ko + a.ks, tabs = a.ks ? a.ks : 1;
    void* base;
    if ((rc = ctx_workspace(ctx, WS_ED_PROOF, st, tabs * ED_TAB_BYTES + 256, &base))) return rc;
    const int4* sh_tab = (const int4*)base;
    uint8_t* sh_bad = (uint8_t*)base + tabs * ED_TAB_BYTES;
    if (a.ks) {
        hipLaunchKernelGGL(ed25519_lincomb_tables_kernel, dim3(1), dim3(64), 0, st, a.ks, (const uint32_t*)a.shared, a.nil_mask,
                           (int4*)base, sh_bad);
        KYB_HIP_CHECK(hipGetLastError());
    }
    return ed_for_pieces(
        n, st, ed_slab_lincomb(a.ko, K),
        [&](DeviceCtx*, size_t lo, size_t cnt, const EdSlab& w) {
            hipLaunchKernelGGL(ed25519_lincomb_kernel, ed_grid(cnt, ED_TAB_BLOCK), dim3(ED_TAB_BLOCK), 0,
                               st, cnt, (int)a.ko, (int)a.ks, a.nil_mask, (const uint32_t*)a.scalars + lo * 8 * K,
                               (const uint32_t*)a.own + lo * 8 * a.ko, sh_tab, (const uint8_t*)sh_bad, a.flags, w.proj, w.status,
                               w.gtab, w.digits);
            hipLaunchKernelGGL(ed25519_lincomb_encode_kernel, ed_encode_grid(cnt), dim3(ED_ENC_BLOCK), 0, st, cnt,
                               (const int32_t*)w.proj, (const uint8_t*)w.status,
                               a.expect ? (const uint32_t*)a.expect + lo * 8 : nullptr, a.out ? (uint32_t*)a.out + lo * 8 : nullptr,
                               a.ok ? (uint8_t*)a.ok + lo : nullptr, a.status ? (uint8_t*)a.status + lo : nullptr);
        },
        ed_lincomb_piece(a.ko));
}

static bool fs_args_bad(size_t n, const void* names, const void* off, size_t name_len, const void* data, size_t data_len,
                        const void* c) {
    if (data_len % 32) return true;
    return n && (!c || (data_len && !data) || (!names && (off || name_len)));
}

static int launch_fs_challenge(size_t n, const void* names, const void* off, size_t name_len, const void* data, size_t data_len,
                               void* c, void* status, hipStream_t st) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    hipLaunchKernelGGL(ed25519_fs_challenge_kernel, ed_grid(n, 64), dim3(64), 0, st, n, (const uint8_t*)names,
                       (const uint64_t*)off, name_len, (const uint8_t*)data, data_len, (uint32_t*)c, (uint8_t*)status);
    KYB_HIP_CHECK(hipGetLastError());
    return KYB_OK;
}

}  // namespace kyb

using namespace kyb;

extern "C" {

int kyb_ed25519_lincomb_dev(size_t n, size_t ko, size_t ks, const void* d_scalars, const void* d_own, const void* d_shared,
                            uint32_t nil_mask, const void* d_expect, void* d_out, void* d_ok, void* d_status, uint32_t flags,
                            void* stream) {
    const LincombArgs a{ko, ks, d_scalars, d_own, d_shared, nil_mask, d_expect, d_out, d_ok, d_status, flags};
    if (int rc; ed_entry_done(&rc, n, lincomb_args_bad(n, a), "kyb_ed25519_lincomb_dev: bad argument")) return rc;
    return launch_lincomb(n, a, (hipStream_t)stream);
}

int kyb_ed25519_lincomb(size_t n, size_t ko, size_t ks, const uint8_t* scalars, const uint8_t* own, const uint8_t* shared,
                        uint32_t nil_mask, const uint8_t* expect, uint8_t* out, uint8_t* ok, uint8_t* status, uint32_t flags) {
    const LincombArgs a{ko, ks, scalars, own, shared, nil_mask, expect, out, ok, status, flags};
    if (int rc; ed_entry_done(&rc, n, lincomb_args_bad(n, a),
                              "kyb_ed25519_lincomb: bad argument (flags other than KYB_F_VARTIME; 1 <= ko + ks, ko <= 4, ks <= 4; nil_mask "
                              "bits at or above ks; expect and ok go together; out or ok; own iff ko, shared iff ks)"))
        return rc;
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    return staged_call(ctx,
                       {{scalars, n * (ko + ks) * 32},
                        {own, n * ko * 32, /*absent=*/!own},
                        {shared, ks * 32, /*absent=*/!shared},
                        {expect, n * 32, /*absent=*/!expect}},
                       {{out, n * 32}, {ok, n}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           LincombArgs d = a;
                           d.scalars = in[0];
                           d.own = in[1];
                           d.shared = in[2];
                           d.expect = in[3];
                           d.out = out ? o[0] : nullptr;
                           d.ok = ok ? o[1] : nullptr;
                           d.status = o[2];
                           return launch_lincomb(n, d, st);
                       });
}

int kyb_ed25519_fs_challenge_dev(size_t n, const void* d_names, const void* d_name_off, size_t name_len, const void* d_data,
                                 size_t data_len, void* d_c, void* d_status, void* stream) {
    if (int rc; ed_entry_done(&rc, n, fs_args_bad(n, d_names, d_name_off, name_len, d_data, data_len, d_c),
                              "kyb_ed25519_fs_challenge_dev: bad argument")) return rc;
    return launch_fs_challenge(n, d_names, d_name_off, name_len, d_data, data_len, d_c, d_status, (hipStream_t)stream);
}

int kyb_ed25519_fs_challenge(size_t n, const uint8_t* names, const uint64_t* name_off, size_t name_len, const uint8_t* data,
                             size_t data_len, uint8_t* c, uint8_t* status) {
    if (int rc; ed_entry_done(&rc, n, fs_args_bad(n, names, name_off, name_len, data, data_len, c),
                              "kyb_ed25519_fs_challenge: bad argument (data_len a multiple of 32; names where offsets or a length name "
                              "bytes)"))
        return rc;
    if (name_off)
        for (size_t i = 0; i < n; i++)
            if (name_off[i + 1] < name_off[i]) {
                set_error("kyb_ed25519_fs_challenge: bad argument (name offsets must not decrease)");
                return KYB_E_ARG;
            }
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::vector<uint64_t> rel(name_off ? n + 1 : 0);
    for (size_t i = 0; i < rel.size(); i++) rel[i] = name_off[i] - name_off[0];
    const size_t name_bytes = name_off ? (size_t)rel[n] : name_len;
    return staged_call(ctx,
                       {{names ? names + (name_off ? name_off[0] : 0) : nullptr, name_bytes},
                        {rel.data(), rel.size() * sizeof(uint64_t), /*absent=*/!name_off},
                        {data, n * data_len}},
                       {{c, n * 32}, {status, n}}, [&](void* const* in, void* const* o, hipStream_t st) {
                           return launch_fs_challenge(n, in[0], in[1], name_len, in[2], data_len, o[0], o[1], st);
                       });
}
}
