// Host-side launch plumbing shared by every Ed25519 unit (ed25519.hip and the ed25519_*.hip next to it): the layout of
// the (WS_ED, stream) slab, the piece loop over a large batch, the encoder's launch geometry, and the small glue every
// entry point repeats (its opening, the group order, the stride check, the grid of a launch).  Host code only: no
// kernel is defined or instantiated here, each unit keeps its own.
#pragma once
#include "context.h"
#include "ed25519_dev.cuh"
#include "ed_spans.h"
#include "scalar_field.cuh"

namespace kyb {

// Lanes per piece of the fused calls (verify, a*P + b*Q, DLEQ): enough waves to fill the device at three per SIMD
// (256 CUs x 4 SIMDs x 3 waves x 64 lanes = 196 608), and a per-stream slab that is bounded whatever n is (below).
constexpr size_t ED_PIECE = size_t(1) << 18;
// Block size of the kernels that keep window tables in the slab: lanes past n of the last block write their tables too.
constexpr size_t ED_TAB_BLOCK = 128;

constexpr size_t ED_TAB_BYTES = sizeof(TabScratch);  // one window table: the 8 cached entries TabGlobal lays out per lane
constexpr size_t ED_PROJ_LIMBS = 3 * sizeof(fe) / sizeof(int32_t);  // one parked point: store_proj's (X, Y, Z)
static_assert(ED_TAB_BYTES == 80 * sizeof(int4) && ED_TAB_BYTES == 1280, "TabGlobal: 8 x 10 int4 per lane and table");
static_assert(ED_PROJ_LIMBS == 30, "store_proj / ed_encode_chunk: 30 limbs per parked point");

// The slab of `lanes` lanes:  [ window tables: lanes x tabs x 1 280 B | parked digits: lanes x digits x 32 B |
// (X, Y, Z): lanes x parked x 120 B | status: lanes ] + 256 B.  `whole_blocks`: lanes are rounded up to ED_TAB_BLOCK,
// so that the idle lanes of the last block (which run the ladder on a copy of element n - 1) keep their table writes
// inside the slab.
struct EdSlabDesc {
    size_t tabs, parked;
    bool status, whole_blocks;
    size_t digits = 0;  // scalars whose recoded digits are parked (ed25519_proof.cuh): 32 B per lane each
};
struct EdSlab {
    int4* gtab;       // lane l, table t: gtab + (l * tabs + t) * 80
    int32_t* proj;    // element i, point k: proj + (i * parked + k) * 30
    uint8_t* status;  // nullptr when the description has none
    uint32_t* digits;  // block b: digits + b * ED_TAB_BLOCK * 8 * desc.digits, the block's lanes interleaved
};
constexpr size_t ed_slab_lanes(const EdSlabDesc& d, size_t lanes) {
    return d.whole_blocks ? (lanes + ED_TAB_BLOCK - 1) / ED_TAB_BLOCK * ED_TAB_BLOCK : lanes;
}
constexpr size_t ed_slab_bytes(const EdSlabDesc& d, size_t lanes) {
    return ed_slab_lanes(d, lanes) *
               (d.tabs * ED_TAB_BYTES + d.digits * 32 + d.parked * ED_PROJ_LIMBS * sizeof(int32_t) + (d.status ? 1 : 0)) +
           256;
}
constexpr EdSlabDesc ED_SLAB_VERIFY{1, 1, true, true};  // ed25519_verify_kernel
constexpr EdSlabDesc ED_SLAB_MUL2{2, 1, true, true};    // ed25519_mul2_kernel: a table for P and one for Q
constexpr EdSlabDesc ED_SLAB_DLEQ{2, 2, true, true};    // ed25519_dleq_kernel: both sides rewrite the two tables, park a and b
constexpr EdSlabDesc ED_SLAB_THETA{2, 1, true, true};   // ed25519_theta_kernel: a table for A + U and one for B + W
// ed25519_ring_chain_kernel: the tag's table and the ring member's; five parked slots (600 B) hold PG's (X, Y, Z) at
// byte 0 and the hash midstate (ed25519_ring.cuh EdRingMid, 368 B) at byte 128; the status stays in a register
constexpr EdSlabDesc ED_SLAB_RING{2, 5, false, true};
constexpr EdSlabDesc ED_SLAB_RING_CHALLENGE{0, 5, false, false};  // ed25519_ring_challenge_kernel: the midstate alone
constexpr size_t ED_RING_MID_OFFSET = 128;
// ed25519_ecies_seal_kernel: the table of pub, r B and r pub parked; ed25519_ecies_open_kernel: the table of R, x R parked.
// Their lanes past n leave before the table, and the encoder writes the points' bytes over the front of each table.
constexpr EdSlabDesc ED_SLAB_ECIES_SEAL{1, 2, true, false};
constexpr EdSlabDesc ED_SLAB_ECIES_OPEN{1, 1, true, false};
// ed25519.hip's multiplications run a whole call of n lanes at once, and their lanes past n leave before the table
constexpr EdSlabDesc ED_SLAB_MUL_BASE{0, 1, false, false};
constexpr EdSlabDesc ed_slab_mul(bool status) { return EdSlabDesc{1, 1, status, false}; }
// ed25519_lincomb_kernel: a table for each of the lane's ko own points and the digits of all k = ko + ks scalars.  Its
// pieces shrink with ko so that no shape's slab exceeds ED_SLAB_MUL2's at ED_PIECE.
constexpr EdSlabDesc ed_slab_lincomb(size_t ko, size_t k) { return EdSlabDesc{ko, 1, true, true, k}; }
constexpr size_t ed_lincomb_piece(size_t ko) {
    return ko <= 1 ? ED_PIECE : ko == 2 ? ED_PIECE / 8 * 7 : ko == 3 ? ED_PIECE / 2 : ED_PIECE / 16 * 7;
}
// ed25519_cosi_aggregate_kernel parks the aggregate key and its status; its lanes past n store nothing.  A verification
// (ed25519_cosi_check_kernel) adds one window table and, in the digits field's 32 B per lane, lane-contiguous, the
// aggregate's bytes that the hash reads; the table's lanes past n write theirs, hence whole blocks.
constexpr EdSlabDesc ED_SLAB_COSI_AGGREGATE{0, 1, true, false};
constexpr EdSlabDesc ED_SLAB_COSI_VERIFY{1, 1, true, true, 1};
// ed25519_schnorr_points_kernel parks R = k B and A = x B; the digits field's 64 B per element, element-contiguous, take
// their encodings for ed25519_schnorr_sign_kernel; no table and no status.  ed25519_vss_seal_kernel: the table of the
// verifier's key, DHKey, R and pre parked; ed25519_vss_open_kernel: the table of DHKey, pre parked.  As with the ECIES
// calls the lanes past n leave before the table and the encoder writes the points' bytes over the front of each table.
constexpr EdSlabDesc ED_SLAB_SCHNORR_SIGN{0, 2, false, false, 2};
constexpr EdSlabDesc ED_SLAB_VSS_SEAL{1, 3, true, false};
constexpr EdSlabDesc ED_SLAB_VSS_OPEN{1, 1, true, false};
// ed25519_eddsa_nonce_kernel parks R = r B; the digits field's 64 B per element, element-contiguous, take R's encoding
// (from the encoder) and r (from the nonce pass) for ed25519_eddsa_sign_kernel; no table and no status.  A key expansion
// (ed25519_eddsa_expand_kernel) parks one point per seed and nothing else: ED_SLAB_MUL_BASE, in pieces.
constexpr EdSlabDesc ED_SLAB_EDDSA_SIGN{0, 1, false, false, 2};
// sign/anon's seal and open (ed25519_anonenc.hip): an element of `ring` keys is ring + 1 lanes -- its head and one per
// member -- each with a parked point and 64 B in the digits field (the point's encoding, a head's xb); one status byte an
// element; a window table per lane unless a seal reads the call's shared tables (an open's head always builds one).  A
// piece is whole elements: ed_anon_piece(ring) of them, at most ED_PIECE lanes, and ED_ANON_SLAB_MAX_RING -- the
// KYB_ANON_MAX_RING of include/kyber_hip.h -- is what lets one element fit a piece.
constexpr size_t ED_ANON_SLAB_MAX_RING = 4096;
constexpr EdSlabDesc ed_slab_anon(size_t ring, bool tables) { return EdSlabDesc{tables ? ring + 1 : 0, ring + 1, true, false, 2 * (ring + 1)}; }
constexpr size_t ed_anon_piece(size_t ring) { return ED_PIECE / (ring + 1); }
static_assert(ed_slab_bytes(ED_SLAB_VERIFY, ED_PIECE) == ED_PIECE * (1280 + 120 + 1) + 256, "367 MB per stream");
static_assert(ed_anon_piece(ED_ANON_SLAB_MAX_RING) == 63 && ed_anon_piece(1) == ED_PIECE / 2, "whole elements, at least one");
static_assert(ed_slab_bytes(ed_slab_anon(1, true), ed_anon_piece(1)) == ED_PIECE / 2 * (2 * (1280 + 64 + 120) + 1) + 256 &&
                  ed_slab_bytes(ed_slab_anon(16, false), ed_anon_piece(16)) == 15420 * (17 * (64 + 120) + 1) + 256 &&
                  ed_slab_bytes(ed_slab_anon(ED_ANON_SLAB_MAX_RING, true), ed_anon_piece(ED_ANON_SLAB_MAX_RING)) <=
                      ed_slab_bytes(ed_slab_anon(1, true), ed_anon_piece(1)) &&
                  ed_slab_bytes(ed_slab_anon(1, true), ed_anon_piece(1)) < ed_slab_bytes(ED_SLAB_MUL2, ED_PIECE),
              "384 MB per stream at most (48 MB for a seal over shared tables), below a * P + b * Q's");
static_assert(ed_slab_bytes(ED_SLAB_SCHNORR_SIGN, ED_PIECE) == ED_PIECE * (64 + 240) + 256, "80 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_EDDSA_SIGN, ED_PIECE) == ED_PIECE * (64 + 120) + 256, "48 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_VSS_SEAL, ED_PIECE) == ED_PIECE * (1280 + 360 + 1) + 256 &&
                  ed_slab_bytes(ED_SLAB_VSS_SEAL, ED_PIECE) < ed_slab_bytes(ED_SLAB_MUL2, ED_PIECE),
              "430 MB per stream, below a * P + b * Q's");
static_assert(ed_slab_bytes(ED_SLAB_VSS_OPEN, ED_PIECE) == ED_PIECE * (1280 + 120 + 1) + 256, "367 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_COSI_AGGREGATE, ED_PIECE) == ED_PIECE * (120 + 1) + 256, "32 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_COSI_VERIFY, ED_PIECE) == ED_PIECE * (1280 + 32 + 120 + 1) + 256 &&
                  ed_slab_bytes(ED_SLAB_COSI_VERIFY, ED_PIECE) < ed_slab_bytes(ED_SLAB_MUL2, ED_PIECE),
              "376 MB per stream, below a * P + b * Q's");
static_assert(ed_slab_bytes(ED_SLAB_MUL2, ED_PIECE) == ED_PIECE * (2560 + 120 + 1) + 256, "703 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_DLEQ, ED_PIECE) == ED_PIECE * (2560 + 240 + 1) + 256, "734 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_THETA, ED_PIECE) == ED_PIECE * (2560 + 120 + 1) + 256, "703 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_RING, ED_PIECE) == ED_PIECE * (2560 + 600) + 256, "828 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_ECIES_SEAL, ED_PIECE) == ED_PIECE * (1280 + 240 + 1) + 256, "399 MB per stream");
static_assert(ed_slab_bytes(ED_SLAB_ECIES_OPEN, ED_PIECE) == ED_PIECE * (1280 + 120 + 1) + 256, "367 MB per stream");
static_assert(ed_slab_bytes(ed_slab_lincomb(1, 3), ed_lincomb_piece(1)) == ED_PIECE * (1280 + 96 + 120 + 1) + 256,
              "392 MB per stream");
static_assert(ed_slab_bytes(ed_slab_lincomb(1, 5), ed_lincomb_piece(1)) == ED_PIECE * (1280 + 160 + 120 + 1) + 256,
              "409 MB per stream");
static_assert(ed_slab_bytes(ed_slab_lincomb(2, 6), ed_lincomb_piece(2)) == 229376 * (2560 + 192 + 120 + 1) + 256,
              "659 MB per stream");
static_assert(ed_slab_bytes(ed_slab_lincomb(3, 7), ed_lincomb_piece(3)) == 131072 * (3840 + 224 + 120 + 1) + 256,
              "549 MB per stream");
static_assert(ed_slab_bytes(ed_slab_lincomb(4, 8), ed_lincomb_piece(4)) == 114688 * (5120 + 256 + 120 + 1) + 256,
              "630 MB per stream");
static_assert(ed_slab_bytes(ed_slab_lincomb(2, 6), ed_lincomb_piece(2)) <= ed_slab_bytes(ED_SLAB_MUL2, ED_PIECE) &&
                  ed_slab_bytes(ed_slab_lincomb(4, 8), ed_lincomb_piece(4)) <= ed_slab_bytes(ED_SLAB_MUL2, ED_PIECE) &&
                  ed_lincomb_piece(2) % ED_TAB_BLOCK == 0 && ed_lincomb_piece(4) % ED_TAB_BLOCK == 0,
              "the largest shapes of each piece size stay below a * P + b * Q's slab; pieces are whole blocks");
static_assert(ED_RING_MID_OFFSET >= ED_PROJ_LIMBS * sizeof(int32_t) && ED_RING_MID_OFFSET % 8 == 0 &&
                  ED_RING_MID_OFFSET + 368 <= ED_SLAB_RING.parked * ED_PROJ_LIMBS * sizeof(int32_t),
              "the parked point, then the midstate, inside the lane's five slots");
static_assert(ed_slab_bytes(ED_SLAB_VERIFY, 1) == ED_TAB_BLOCK * 1401 + 256 && ed_slab_lanes(ED_SLAB_DLEQ, 129) == 256, "whole blocks");
static_assert(ed_slab_bytes(ed_slab_mul(false), 4099) == 4099 * 1400 + 256 && ed_slab_bytes(ed_slab_mul(true), 4099) == 4099 * 1401 + 256 &&
                  ed_slab_bytes(ED_SLAB_MUL_BASE, 4099) == 4099 * 120 + 256,
              "unrounded");

// Grows (never shrinks) the stream's WS_ED workspace to the slab of `lanes` lanes and carves it.  The caller holds enq_mu
// until the kernels that use the slab are enqueued (context.h).
inline int ed_slab(DeviceCtx* ctx, hipStream_t st, const EdSlabDesc& d, size_t lanes, EdSlab* s) {
    void* base;
    if (int rc = ctx_workspace(ctx, WS_ED, st, ed_slab_bytes(d, lanes), &base)) return rc;
    lanes = ed_slab_lanes(d, lanes);
    const size_t tab_bytes = lanes * d.tabs * ED_TAB_BYTES, digit_bytes = lanes * d.digits * 32,
                 proj_bytes = lanes * d.parked * ED_PROJ_LIMBS * sizeof(int32_t);
    s->gtab = (int4*)base;
    s->digits = (uint32_t*)((uint8_t*)base + tab_bytes);
    s->proj = (int32_t*)((uint8_t*)base + tab_bytes + digit_bytes);
    s->status = d.status ? (uint8_t*)base + tab_bytes + digit_bytes + proj_bytes : nullptr;
    return KYB_OK;
}

// A batch of n in pieces of `piece` lanes, under enq_mu (the slab and its kernels as one unit): the slab is sized by
// the first piece and serves every piece; enqueue(ctx, lo, cnt, slab) launches the kernels of elements [lo, lo + cnt).
template <class F>
int ed_for_pieces(size_t n, hipStream_t st, const EdSlabDesc& d, F&& enqueue, size_t piece = ED_PIECE) {
    DeviceCtx* ctx;
    int rc = get_ctx(&ctx);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> enq_lock(ctx->enq_mu);
    for (size_t lo = 0; lo < n; lo += piece) {
        EdSlab slab;
        if ((rc = ed_slab(ctx, st, d, std::min(piece, n), &slab))) return rc;
        enqueue(ctx, lo, std::min(piece, n - lo), slab);
        KYB_HIP_CHECK(hipGetLastError());
    }
    return KYB_OK;
}

// Launch geometry of the shared-inversion encoder (ed_encode_chunk): a block of ED_ENC_BLOCK lanes owns
// ED_ENC_BLOCK * ENC_CHUNK consecutive parked points, interleaved over its lanes; the last block may have lanes with
// fewer points than the others, or none.
constexpr unsigned ED_ENC_BLOCK = 64;
constexpr size_t ED_ENC_SPAN = size_t(ED_ENC_BLOCK) * ENC_CHUNK;  // points per block
inline dim3 ed_encode_grid(size_t points) { return dim3((unsigned)((points + ED_ENC_SPAN - 1) / ED_ENC_SPAN)); }
// The grid of a launch with one lane per element (or per whatever `lanes` counts) in blocks of `block`
inline dim3 ed_grid(size_t lanes, size_t block) { return dim3((unsigned)((lanes + block - 1) / block)); }

// The group order l, as the kernels that reduce mod l take it
inline const sf::Mod& ed_order() {
    static const sf::Mod m = sf::make_mod(sf::Q_ED25519, false);
    return m;
}
// a byte stride between the elements' keys: 32, or 0 for one key that serves the whole batch
inline bool stride_bad(size_t s) { return s != 0 && s != 32; }

// How every kyb_ed25519_* entry opens: a refused call leaves `refusal` ("<entry>: bad argument ...") as the thread's
// error and ends with KYB_E_ARG, an empty batch ends with KYB_OK.  True: the entry is over and returns *rc.
inline bool ed_entry_done(int* rc, size_t n, bool bad, const char* refusal) {
    if (bad) set_error(refusal);
    *rc = bad ? KYB_E_ARG : KYB_OK;
    return bad || n == 0;
}
}  // namespace kyb
