// kyber_amd/csrc/msm_plan.h compiled for the CPU (test infrastructure, never linked into libkyberhip.so):
// tests/test_msm_plan_host.py reads the plan, the split tail's schedule and the workspace layout of a call through
// these entry points.
#include "../kyber_amd/csrc/msm_plan.h"

using namespace kyb::msm;

extern "C" {
// the workspace's buffers in the order they lie in memory, comma-separated
const char* mph_names() {
#define X(name, elem, count) #name ","
    return KYB_MSM_WORKSPACE(X);
#undef X
}
// reads the environment switches (once per process); returns how many differ from their defaults
int mph_switches_set() {
    const Switches& s = switches();
    return (s.chunk != 8) + s.sort + (s.sort_tiles != 0) + (s.sort_xcd != 1) + (s.sub != 0) + s.decode + s.join + s.tail +
           (s.reduce != 0) + s.final_;
}
// traits: aff, acc, split, bits, cmax, coop_slots, split_tail, fold_groups, fold_bits
// plan: c, nwin, nb, chunk, nchunks, bits
// offs: one byte offset per buffer, then the total
// misc: nbk, tiles, two_pass, cb, tiles1, m1, sub, max_pieces, n_partial, n_fold, n_chains
// tail: on, fuse, lb0, chbits, tz, nchains, reduce_out, nlevels, 4 x (nplain, ncur, nout, lb_out, rows_out),
//       nfolds, 4 x (nin, nout), nlast
void mph_call(uint64_t n, uint32_t flags, int num_cu, const int64_t* traits, int fuse_ok, int64_t* plan, uint64_t* offs,
              int64_t* misc, int64_t* tail) {
    const Traits t = {(size_t)traits[0], (size_t)traits[1], (int)traits[2], (int)traits[3], (int)traits[4],
                      traits[5] != 0,    traits[6] != 0,    (int)traits[7], (int)traits[8]};
    Switches sw = switches();
    if (!fuse_ok) sw.reduce = 'n';
    const Plan p = call_plan(n, flags, t, sw);
    const Layout L = layout(p, n * t.split, num_cu, t, sw);
    const int64_t pl[] = {p.c, p.nwin, p.nb, p.chunk, p.nchunks, p.bits};
    for (int i = 0; i < 6; i++) plan[i] = pl[i];
#define X(name, elem, count) *offs++ = L.name;
    KYB_MSM_WORKSPACE(X)
#undef X
    *offs = L.bytes;
    const int64_t m[] = {(int64_t)L.nbk, L.tiles,          L.two_pass,          L.cb,
                         L.tiles1,       (int64_t)L.m1,    L.sub,               (int64_t)L.max_pieces,
                         (int64_t)L.n_partial, (int64_t)L.n_fold, (int64_t)L.n_chains};
    for (int i = 0; i < 11; i++) misc[i] = m[i];
    const TailSchedule& s = L.tail;
    int64_t* o = tail;
    const int64_t head[] = {s.on, s.fuse, s.lb0, s.chbits, s.tz, s.nchains, s.on ? (int64_t)tail_reduce_out(p, s) : 0, s.nlevels};
    for (int64_t v : head) *o++ = v;
    for (int i = 0; i < 4; i++) {
        const TailSchedule::Level& l = s.level[i];
        const int64_t lv[] = {l.nplain, l.ncur, l.nout, l.lb_out, i < s.nlevels ? (int64_t)tail_level_out(p, l) : 0};
        for (int64_t v : lv) *o++ = v;
    }
    *o++ = s.shifted.n;
    for (int i = 0; i < 4; i++) {
        *o++ = s.shifted.level[i].nin;
        *o++ = s.shifted.level[i].nout;
    }
    *o++ = s.shifted.nlast;
}
}
