// The MSM's host arithmetic (msm.cuh run): everything about a call that is decided before the first launch -- the
// window plan, the environment switches, the split tail's schedule and the workspace layout.  Plain C++, nothing from
// HIP: tests/msm_plan_harness.cpp compiles it for the host and tests/test_msm_plan_host.py checks that every launch of
// the tail fits the buffer the layout gave it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace kyb {
namespace msm {

struct Plan {
    size_t n;
    int c;        // window bits
    int nwin;     // number of windows (incl. the carry window)
    int nb;       // buckets per window = 2^(c-1)
    int chunk;    // buckets per reduce lane
    int nchunks;  // chunks per window
    uint32_t flags;  // the call's KYB_F_* flags (input format / trusted operands), read by the adapter's decode
    int bits;        // scalar bits that count (KYB_F_SCALAR_BITS: bdn's 128-bit coefficients); higher bits are ignored
};

// Environment switches, read once per process at first use; for experiments and A/B runs only.  A word counts by its
// first letter.
struct Switches {
    int chunk;       // KYB_MSM_CHUNK=2|4|..|64  buckets per reduce chain at least (a power of two in range, else 8)
    bool sort;       // KYB_MSM_SORT=single      the counting sort in one pass at every size
    int sort_tiles;  // KYB_MSM_SORT_TILES=N     tiles per window of the one-pass sort (N > 0)
    int sort_xcd;    // KYB_MSM_SORT_XCD=0       tile-minor workgroup order of the one-pass scatter (1 otherwise)
    int sub;         // KYB_MSM_SUB=N            points per bucket piece (N > 0; experiments: profiles/r03_msm_knobs.json)
    bool decode;     // KYB_MSM_DECODE=full      the one decode kernel for every calling convention, never the light one
    bool join;       // KYB_MSM_JOIN=lane        buckets of several pieces joined by one lane each
    bool tail;       // KYB_MSM_TAIL=lane        the one-lane reduce / fold kernels instead of the cooperative ones
    char reduce;     // KYB_MSM_REDUCE=mul       'm': no split tail, every chunk multiplies its own lo * run (rounds 3-5)
                     // KYB_MSM_REDUCE=nofuse    'n': the split tail's whole tree in the fold launches; 0 otherwise
    bool final_;     // KYB_MSM_FINAL=lanes      the three-lane final kernel, not the limb-per-lane rows; no split tail either
    bool split() const { return reduce != 'm' && !final_; }
    bool fuse() const { return reduce != 'n'; }
};
inline const Switches& switches() {
    static const Switches sw = [] {
        const auto is = [](const char* name, char first) {
            const char* e = getenv(name);
            return e && e[0] == first;
        };
        const auto num = [](const char* name) {
            const char* e = getenv(name);
            return e ? atoi(e) : 0;
        };
        Switches s;
        const int v = num("KYB_MSM_CHUNK");
        s.chunk = v >= 2 && v <= 64 && (v & (v - 1)) == 0 ? v : 8;
        s.sort = is("KYB_MSM_SORT", 's');
        s.sort_tiles = num("KYB_MSM_SORT_TILES");
        s.sort_xcd = is("KYB_MSM_SORT_XCD", '0') ? 0 : 1;
        s.sub = num("KYB_MSM_SUB");
        s.decode = is("KYB_MSM_DECODE", 'f');
        s.join = is("KYB_MSM_JOIN", 'l');
        s.tail = is("KYB_MSM_TAIL", 'l');
        s.reduce = is("KYB_MSM_REDUCE", 'm') ? 'm' : is("KYB_MSM_REDUCE", 'n') ? 'n' : 0;
        s.final_ = is("KYB_MSM_FINAL", 'l');
        return s;
    }();
    return sw;
}

inline Plan make_plan(size_t n, int scalar_bits = 256, int cmax = 16, const Switches& sw = switches()) {
    Plan p;
    p.n = n;
    p.flags = 0;
    p.bits = scalar_bits;
    int lg = 0;
    while ((size_t(1) << (lg + 1)) <= n) lg++;
    int c = lg - 3;
    if (c < 3) c = 3;  // at most 86 windows: final_kernel gives each window up to 4 lanes of its 512
    if (c > cmax) c = cmax;
    p.c = c;
    p.nwin = (scalar_bits + c) / c;  // ceil((bits + 1) / c): the scalar bits + the recoding carry
    p.nb = 1 << (c - 1);
    // buckets per reduce lane: the running-sum chain of a lane is latency-bound (2 dependent additions per bucket, and
    // a lone wave already saturates its SIMD's issue rate), so take the shortest chains that still leave every wave
    // a SIMD of its own: at most 1024 waves = 65536 lanes, between 8 and 64 buckets each
    int chunk = sw.chunk;
    while (chunk < 64 && (size_t)p.nwin * (p.nb / chunk) > 65536) chunk <<= 1;
    p.chunk = p.nb < chunk ? p.nb : chunk;
    p.nchunks = p.nb / p.chunk;
    return p;
}

constexpr int SCAN_T = 256, SCAN_E = 16, SCAN_TILE = SCAN_T * SCAN_E;  // launch_scan: threads, entries per thread
constexpr int HIST_MAX_NB = 1 << 15;  // bucket counters of a window in LDS (hist_lds_kernel)

#ifndef KYB_MSM_P2_T1
#define KYB_MSM_P2_T1 8192
#endif
#ifndef KYB_MSM_P2_LMAX
#define KYB_MSM_P2_LMAX 18432
#endif
// the two-pass sort (msm.cuh coarse_hist_kernel ff.)
// (tile and staging sizes that leave two workgroups per CU: fine_sort 76 -> 65 us, coarse_scatter 45 -> 38 us against 2^14 / 24 576;
// a bin of the halves' top window where the density doubles goes the direct way)
constexpr int P2_GIANT = 131072, P2_GS = 64;  // giant bins (giant_*_kernel): entries from which, slices per bin
constexpr int P2_FB = 256, P2_T1 = KYB_MSM_P2_T1, P2_MAXCB = 128, P2_LMAX = KYB_MSM_P2_LMAX, P2_T = 1024;

// the plan takes the two passes: whole bins of 256 buckets, an index that fits 23 bits
inline bool sort_two_pass(const Plan& p, size_t ne, const Switches& sw = switches()) {
    // (below 2^19 entries per window the one pass is ahead: 1.70 against 1.85 ms for 2^16 points, 1.78 against 2.00 for 2^17)
    return !sw.sort && p.nb >= 8192 && p.nb / P2_FB <= P2_MAXCB && ne >= (size_t(1) << 19) && ne <= (size_t(1) << 23);
}

// Tiles per window of the one-pass sort: at most ONE round of the chip's CUs in all (a workgroup holds 128 KB of LDS;
// rounds 1-5 aimed at "about two per CU" and, for 17 windows of Ed25519 scalars, got 272 workgroups: a full round and a
// sixteenth of one, i.e. two), a tile of at least two points per bucket (the per-tile flush is per bucket).
// A forced count: 14 .. 56 tiles all within 1 % for the 2^20-point BLS12-381 G1 MSM.
inline int sort_tiles(int num_cu, int nwin, size_t ne, int nb, const Switches& sw = switches()) {
    int tiles = sw.sort_tiles > 0 ? sw.sort_tiles : num_cu / nwin;
    if (tiles < 1) tiles = 1;
    while (tiles > 1 && (ne ? ne : 1) / tiles < 2 * (size_t)nb) tiles--;
    return tiles;
}

constexpr int MAXSUB = 256;
// Points per accumulate lane: a longer bucket is cut into pieces that are joined afterwards (one full addition per
// extra piece, bucket_kernel).  Twice the mean bucket length, so that only skewed digits split a bucket -- with a fixed
// 64 every second bucket of the 2^20-point BLS12-381 G1 MSM (mean 64) had a second, tiny piece: 6.10 -> 5.94 ms --
// between 64 and MAXSUB.
inline uint32_t piece_len(size_t ne, int nb, const Switches& sw = switches()) {
    size_t v = sw.sub > 0 ? (size_t)sw.sub : 2 * (ne / (size_t)nb + 1);
    v = (v + 31) / 32 * 32;
    return (uint32_t)(v < 64 ? 64 : (v > MAXSUB ? MAXSUB : v));
}

constexpr int REDUCE_FUSED_BITS = 4;  // log2 of reduce_coop_kernel's 16 groups

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// What the layout has to know about an adapter (msm.cuh traits_of<A>)
struct Traits {
    size_t aff, acc;              // sizeof(A::Aff), sizeof(A::Acc)
    int split, bits, cmax;        // Split<A>
    bool coop_slots, split_tail;  // HasCoopSlots<A>, split_tail<A>()
    int fold_groups, fold_bits;   // partials per output of the cooperative folds and their log2 (32 / 5 without slots)
};

// The launches that fold a row of n entries `per` at a time until at most `last` are left (rows of at most 2^15
// entries, 32 or more per output: three launches)
struct Folds {
    struct Level {
        int nin, nout;
    };
    int n;
    Level level[4];
    int nlast;  // entries left
};
inline Folds fold_levels(int n, int per, int last = 1) {
    Folds f = {};
    while (n > last && f.n < 4) {
        const int nout = (n + per - 1) / per;
        f.level[f.n++] = {n, nout};
        n = nout;
    }
    f.nlast = n;
    return f;
}

// The split tail (msm.cuh tree_fold_bits_coop_kernel): the launches of the bit tree, then the doubling chains, then the
// fold over the shifted terms.  Computed ONCE per call: the layout sizes partial / folded / shift / shift2 from it and
// tail_split launches from it, so a fold cannot be launched over more rows than its buffer was given.
struct TailSchedule {
    struct Level {
        int nplain, ncur, nout, lb_out;  // plain rows and entries per row that go in, entries per row and bits that come out
    };
    bool on;         // the call takes the split tail
    int fuse, lb0;   // reduce_coop_kernel runs the first REDUCE_FUSED_BITS levels itself
    int chbits, tz;  // log2 of the chunks per window and of the chunk
    int nlevels;
    Level level[4];  // as many as a fold by fold_groups has
    int nchains;     // terms left: nwin * (1 + chbits), each with a doubling chain of its own
    Folds shifted;   // the fold over the shifted terms: 2 * fold_groups per output, down to one or two for final_kernel's tree
};
inline TailSchedule tail_schedule(const Plan& p, const Traits& t, const Switches& sw = switches()) {
    TailSchedule s = {};
    s.on = t.split_tail && !sw.tail && sw.split() && p.nwin > 1;
    if (!s.on) return s;
    while ((1 << s.chbits) < p.nchunks) s.chbits++;
    while ((1 << s.tz) < p.chunk) s.tz++;
    s.fuse = sw.fuse() && p.nchunks >= 16 ? 1 : 0;
    s.lb0 = s.fuse ? REDUCE_FUSED_BITS : 0;
    int nplain = p.nwin * (1 + s.lb0), done = s.lb0;
    const Folds f = fold_levels(s.fuse ? p.nchunks / 16 : p.nchunks, t.fold_groups);
    for (s.nlevels = 0; s.nlevels < f.n; s.nlevels++) {
        const int lb_out = s.chbits - done < t.fold_bits ? s.chbits - done : t.fold_bits;
        s.level[s.nlevels] = {nplain, f.level[s.nlevels].nin, f.level[s.nlevels].nout, lb_out};
        nplain += p.nwin * lb_out;
        done += lb_out;
    }
    s.nchains = nplain;  // the W sums and every D_k
    s.shifted = fold_levels(s.nchains, 2 * t.fold_groups, 2);
    return s;
}
// rows x entries a launch of the bit tree writes: the plain rows, lb_out D rows and the A row of every window
inline size_t tail_level_out(const Plan& p, const TailSchedule::Level& l) {
    return ((size_t)l.nplain + (size_t)p.nwin * (l.lb_out + 1)) * l.nout;
}
// entries reduce_coop_kernel writes for the split tail: W and T rows, or with its own levels W, four D rows and A
inline size_t tail_reduce_out(const Plan& p, const TailSchedule& s) {
    return s.fuse ? (size_t)p.nwin * (2 + REDUCE_FUSED_BITS) * (p.nchunks / 16) : 2 * (size_t)p.nwin * p.nchunks;
}

// The workspace: name, element, count -- in the order they lie in memory.  lenhist .. bad are zeroed together by one
// memset; a buffer whose count is 0 takes no room.  Counts are written over the locals of layout() below.
// (Elements: Aff / Acc are the adapter's, U32 / I32 four bytes.)
#define KYB_MSM_WORKSPACE(X)                                                                                          \
    X(aff, Aff, n1)                                                                                                   \
    X(digits, I32, n1 * p.nwin)                                                                                       \
    X(sorted, U32, n1 * p.nwin)                                                                                       \
    X(hist, U32, nbk * (size_t)L.tiles)                                                                               \
    X(total, U32, nbk) /* points per bucket */                                                                        \
    X(mid, U32, L.two_pass ? n1 * p.nwin : 0)                                                                         \
    X(ch, U32, L.m1)                                                                                                  \
    X(offs1, U32, L.m1 + 1)                                                                                           \
    X(giant, U32, max_giant)                                                                                          \
    X(gcnt, U32, max_giant * P2_GS * P2_FB)                                                                           \
    X(lenhist, U32, MAXSUB + 2)                                                                                       \
    X(lencursor, U32, MAXSUB + 2)                                                                                     \
    X(nlong, U32, 64)                                                                                                 \
    X(bad, U32, 64)                                                                                                   \
    X(offs, U32, nbk + 1)                                                                                             \
    X(nsub, U32, nbk)                                                                                                 \
    X(suboffs, U32, nbk + 1)                                                                                          \
    X(pieces, Acc, L.max_pieces)                                                                                      \
    X(plo, U32, L.max_pieces)                                                                                         \
    X(plen, U32, L.max_pieces)                                                                                        \
    X(order, U32, L.max_pieces)                                                                                       \
    X(pdst, U32, L.max_pieces)                                                                                        \
    X(longlist, U32, nbk)                                                                                             \
    X(joinlist, U32, nbk)                                                                                             \
    X(lpart, Acc, t.coop_slots ? L.max_pieces : 0) /* slice sums of long buckets */                                   \
    X(buckets, Acc, nbk)                                                                                              \
    X(partial, Acc, n_partial)                                                                                        \
    X(folded, Acc, n_fold)                                                                                            \
    X(shift, Acc, n_chains)                                                                                           \
    X(shift2, Acc, (n_chains + 63) / 64)                                                                              \
    X(tile, U32, ((nbk > L.m1 ? nbk : L.m1) + SCAN_TILE - 1) / SCAN_TILE + 2)                                         \
    X(winsum, Acc, p.nwin)

// Byte offsets of the buffers and what else of a call is fixed before the first launch
struct Layout {
#define X(name, elem, count) size_t name;
    KYB_MSM_WORKSPACE(X)
#undef X
    size_t bytes;       // of the whole workspace
    size_t nbk;         // buckets of all windows
    int tiles;          // one-pass sort: tiles per window
    bool two_pass;      // sort_two_pass
    int cb, tiles1;     // two-pass sort: coarse bins per window, tiles of P2_T1 entries
    size_t m1;          //   and its counters (0 in one pass)
    uint32_t sub;       // piece_len
    size_t max_pieces;  // a piece per bucket and one more per `sub` entries
    TailSchedule tail;
    size_t n_partial, n_fold, n_chains;  // elements of partial, folded and shift
};
inline Layout layout(const Plan& p, size_t ne, int num_cu, const Traits& t, const Switches& sw = switches()) {
    Layout L = {};
    const size_t n1 = ne ? ne : 1, nbk = (size_t)p.nwin * p.nb, Aff = t.aff, Acc = t.acc, U32 = 4, I32 = 4;
    L.nbk = nbk;
    L.tiles = sort_tiles(num_cu, p.nwin, ne, p.nb, sw);
    L.two_pass = sort_two_pass(p, ne, sw);
    L.cb = p.nb / P2_FB;
    L.tiles1 = (int)((n1 + P2_T1 - 1) / P2_T1);
    L.m1 = L.two_pass ? (size_t)p.nwin * L.cb * L.tiles1 : 0;
    const size_t max_giant = L.two_pass ? n1 * (size_t)p.nwin / P2_GIANT + 1 : 0;  // bins of more than P2_GIANT entries
    L.sub = piece_len(n1, p.nb, sw);
    L.max_pieces = nbk + (n1 * (size_t)p.nwin + L.sub - 1) / L.sub;
    L.tail = tail_schedule(p, t, sw);
    // chunk partials ping-pong between `partial` and `folded`; the first fold level leaves one of 64 (one-lane tail)
    // or of 32 / 64 (cooperative tail) partials
    size_t n_partial = (size_t)p.nwin * p.nchunks, n_fold = (size_t)p.nwin * ((p.nchunks + 31) / 32), n_chains = (size_t)p.nwin;
    if (L.tail.on) {  // the bit tree's rows, for the schedule this call runs: levels 0, 2 write `folded`, level 1 `partial`
        n_partial = tail_reduce_out(p, L.tail);
        for (int i = 0; i < L.tail.nlevels; i++) {
            size_t& dst = i % 2 == 0 ? n_fold : n_partial;
            const size_t need = tail_level_out(p, L.tail.level[i]);
            if (need > dst) dst = need;
        }
        n_chains = (size_t)L.tail.nchains;
    }
    L.n_partial = n_partial, L.n_fold = n_fold, L.n_chains = n_chains;
#define X(name, elem, count) \
    L.name = L.bytes;        \
    L.bytes += align256(elem * (size_t)(count));
    KYB_MSM_WORKSPACE(X)
#undef X
    return L;
}

// The plan of a call of n inputs: KYB_F_SCALAR_BITS(b) -- only the low b bits of every scalar count (proportionally
// fewer windows); adapters that split their scalars through an endomorphism already work on halves and ignore it
inline Plan call_plan(size_t n, uint32_t flags, const Traits& t, const Switches& sw = switches()) {
    const size_t ne = n * t.split;  // points after the adapter's endomorphism split
    int bits = t.bits;
    const int want = (int)((flags >> 16) & 0x1ffu);
    if (t.split == 1 && want && want < bits) bits = want;
    return make_plan(ne ? ne : 1, bits, t.cmax, sw);
}

}  // namespace msm
}  // namespace kyb
