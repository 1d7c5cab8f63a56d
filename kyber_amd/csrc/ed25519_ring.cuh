// Ed25519 ring signatures (sign/anon), one signature per lane: the hash chain of Verify and of Sign's open ring.
//
// Replaces, in the reference:
//   sign/anon Verify, the ring loop      sig.go:231-237   -> ed_ring_lane (steps = ring, start = 0)
//   sign/anon Sign, the ring loop        sig.go:159-166   -> ed_ring_lane (steps = ring - 1, start = mine + 1)
//   sign/anon signH1pre                  sig.go:23-32     -> ed_ring_absorb_prefix (m, then L and ~y when linkable)
//   sign/anon signH1                     sig.go:34-43     -> ed_ring_finish (PG, PH, then Scalar.Pick)
//   xof/blake2xb New(seed) + Write       blake.go:19-41   -> blake2xb_root_iv_keyed + the midstate below
// One step computes PG = s_i G + c X_i and, for a linkable signature, PH = s_i linkBase + c tag as two Straus-Shamir
// chains over window tables that live in memory, encodes both with ONE field inversion, and draws the next challenge
// c = Pick(XOF(m || [scope || tag]) || PG || [PH]).
//
// Scalars are the 32 wire bytes, never reduced.  s_i G is geScalarMultBase's value whatever the flag (point.go:243:
// Mul(s, nil) never takes the variable-time path), so under KYB_F_VARTIME the G chain drops a top digit above 8 that
// the linkBase chain keeps; the other three products follow kyb_ed25519_mul under the same flag.  The digits of s_i and
// of c are recoded once per step and serve both chains.
//
// The hash: suite.XOF(message) keys BLAKE2b with the first <= 64 message bytes (a zero-padded block of its own) and
// writes the rest; an empty message is a keyless root.  The step-invariant prefix is absorbed once per signature; its
// midstate (chaining value, byte count, pending partial block) is parked in the lane's slab, and a step finishes from
// it with 32 or 64 more bytes: the pending block is completed in memory, where an arbitrary byte offset costs nothing,
// and read back as words.  BLAKE2b compresses a block only when more input follows, so a last block that is exactly
// full is the final one and no empty block follows it.
// Compiles with g++ too (tests/ring_harness.cpp runs these programs on the CPU against the oracle).
#pragma once
#include "ed25519_dleq.cuh"

namespace kyb {

// Root of blake2b.NewXOF(OutputLengthUnknown, key) for a key of keylen bytes, 0..64: digest 64, fanout 1, depth 1,
// xof length 0xFFFFFFFF in the upper half of the node offset (blake2xb_root_iv is the keylen = 32 case).
KYB_HD void blake2xb_root_iv_keyed(uint64_t (&h)[8], uint32_t keylen) {
    constexpr uint64_t IV[8] = KYB_BLAKE2B_IV;
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= 0x01010040ull | ((uint64_t)keylen << 8);
    h[1] ^= 0xffffffff00000000ull;
}

// The parked hash state of one signature and the lane's other words of memory.  buf holds the pending block (r bytes,
// zero beyond) and a second block for the step's bytes to run over into: r <= 127 and a step adds at most 64.
struct EdRingMid {
    uint64_t h[8];       // chaining value after the prefix's full blocks
    uint64_t t;          // bytes compressed so far
    uint64_t r;          // bytes pending in buf
    uint32_t czero[8];   // the challenge that entered position 0
    uint64_t buf[32];
};
static_assert(sizeof(EdRingMid) == 368, "ed25519_launch.h: ED_SLAB_RING parks 5 x 120 B per lane, this at byte 128");

// Byte p of the stream suite.XOF(msg) has absorbed after Write(scope), Write(tag): the key block, the message past its
// first 64 bytes, the scope, the tag's canonical bytes.  Zero past the end.
struct EdRingPrefix {
    const uint8_t* msg;
    size_t len;
    const uint8_t* scope;  // nullptr: unlinkable, neither scope nor tag is written
    size_t scope_len;
    const uint8_t* tag;    // 32 canonical bytes in memory (linkable)
    KYB_HD size_t keylen() const { return len < 64 ? len : 64; }
    KYB_HD size_t bytes() const { return (len ? 128 : 0) + (len - keylen()) + (scope ? scope_len + 32 : 0); }
    KYB_HD uint32_t at(size_t p) const {
        const size_t kb = len ? 128 : 0, tail = len - keylen();
        if (p < kb) return p < keylen() ? msg[p] : 0u;
        p -= kb;
        if (p < tail) return msg[64 + p];
        p -= tail;
        if (!scope) return 0u;
        if (p < scope_len) return scope[p];
        p -= scope_len;
        return p < 32 ? tag[p] : 0u;
    }
};

// signH1pre: every full block of the prefix is compressed (more input always follows: a step writes at least PG), the
// rest is left pending.  One compression site serves all blocks.
KYB_HD void ed_ring_absorb_prefix(EdRingMid* mid, const EdRingPrefix& pre) {
    uint64_t h[8], m[16];
    blake2xb_root_iv_keyed(h, (uint32_t)pre.keylen());
    const size_t total = pre.bytes(), nfull = total / 128;
#pragma unroll 1
    for (size_t b = 0; b <= nfull; b++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint64_t v = 0;
#pragma unroll
            for (int k = 7; k >= 0; k--) v = (v << 8) | pre.at(128 * b + 8 * i + k);
            m[i] = v;
        }
        if (b < nfull) {
            blake2b_compress_regs(h, m, 128 * (b + 1), false);
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                mid->buf[i] = m[i];
                mid->buf[16 + i] = 0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) mid->h[i] = h[i];
    mid->t = 128 * nfull;
    mid->r = total - 128 * nfull;
}

// signH1: c = Pick(H1pre.Clone() after Write(PG) [, Write(PH)]).  Returns the draws taken, 0 when ED_PICK_MAX_NODES
// output nodes held no scalar below l (c is then zero).  The midstate is left as it was found: the next step writes
// the same bytes of buf.  One compression site serves the one or two last blocks of the root and every output node.
KYB_HD int ed_ring_finish(uint32_t (&c)[8], EdRingMid* mid, const uint32_t pg[8], const uint32_t ph[8], bool linkable) {
    uint8_t* b = reinterpret_cast<uint8_t*>(mid->buf);
    const size_t r = (size_t)mid->r;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) b[r + 4 * i + k] = (uint8_t)(pg[i] >> (8 * k));
    if (linkable) {
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) b[r + 32 + 4 * i + k] = (uint8_t)(ph[i] >> (8 * k));
    }
    const size_t len = r + (linkable ? 64 : 32);
    const int nblk = len > 128 ? 2 : 1;
    uint64_t h[8], m[16];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = mid->h[i];
    uint64_t t = mid->t;
    bool last = false, done = false;
    int draws = 0;
#pragma unroll 1
    for (int it = 0; it < nblk + ED_PICK_MAX_NODES && !done; it++) {
        if (it < nblk) {
            const uint64_t* src = reinterpret_cast<const uint64_t*>(b + 128 * it);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                uint64_t v;
                __builtin_memcpy(&v, src + i, 8);  // the bytes stored above, read back as words
                m[i] = v;
            }
            last = it == nblk - 1;
            t = last ? mid->t + len : mid->t + 128;
        }
        blake2b_compress_regs(h, m, t, last);
        const int node = it - nblk;  // -1: the root hash is ready
        if (node == -1) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                m[i] = h[i];  // every output node's message
                m[8 + i] = 0;
            }
            t = 64;
        } else if (node >= 0) {
            done = ed_pick_draw(c, h[0], h[1], h[2], h[3]);
            draws = 2 * node + 1;
            if (!done) {
                done = ed_pick_draw(c, h[4], h[5], h[6], h[7]);
                draws = 2 * node + 2;
            }
        }
        if (node >= -1) blake2xb_node_iv(h, (uint32_t)(node + 1));
    }
    if (!done) {
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = 0;
        return 0;
    }
    return draws;
}

// What one call shares: window tables nobody writes during the chain.  Table 0 is the standard base's, table 1
// linkBase's, tables 2 .. 2 + ring - 1 the ring members' when the batch shares one ring; bad[k] != 0 where table k's
// point did not decode.
constexpr int ED_RING_TAB_G = 0, ED_RING_TAB_LINK = 1, ED_RING_TAB_KEYS = 2;
struct EdRingShared {
    const int4* tabs;  // table k: tabs + 80 k
    const uint8_t* bad;
};
// One lane's memory: room for the tag's table (built once per signature), for the current ring member's (one ring per
// signature: rebuilt each step), for PG's parked (X, Y, Z) while the second chain runs, and the midstate.
struct EdRingLaneMem {
    int4* tag_tab;
    int4* key_tab;
    int32_t* park;
    EdRingMid* mid;
};

// tab = the window table of the point w encodes; false when w does not decode (the table is then of no point)
KYB_DEV bool ed_ring_table(int4* tab, const uint32_t w[8]) {
    ge_p3 A;
    const bool ok = ge_p3_fromwords(A, w);
    TabGlobal t{tab};
    ge_window_table(t, A);
    return ok;
}

// One ring position, sig.go:232-236: c <- signH1(s G + c X, [s linkBase + c tag]).  tx: the ring member's table.
// Returns ed_ring_finish's draw count.
KYB_DEV int ed_ring_step(uint32_t (&c)[8], const uint32_t sw[8], bool full, bool linkable, const EdRingShared& sh,
                         const int4* tx, const EdRingLaneMem& mem) {
    int8_t es[65], ec[65];
    recode16(es, sw, full);
    recode16(ec, c, full);
    int vt_top = 63;
    if (full) {
        const int ta = wave_top_digit(sw), tb = wave_top_digit(c);
        vt_top = ta > tb ? ta : tb;
    }
    // geScalarMultBase drops a top digit above 8 whatever the flag (recode16 has done so already without `full`)
    const int8_t l63 = es[63], l64 = es[64];
    const bool drop = (int)l63 + 16 * (int)l64 > 8;
    ge_p3 h;
    const int sides = linkable ? 2 : 1;
#pragma unroll 1
    for (int side = 0; side < sides; side++) {  // one copy of the chain's code serves both
        es[63] = (side == 0 && drop) ? (int8_t)0 : l63;
        es[64] = (side == 0 && drop) ? (int8_t)0 : l64;
        // the sides are told apart by address, never by selecting between register arrays
        TabGlobal tp{const_cast<int4*>(sh.tabs + (side ? ED_RING_TAB_LINK : ED_RING_TAB_G) * 80)};
        TabGlobal tq{const_cast<int4*>(side ? mem.tag_tab : tx)};
        ge_double_scalarmult_w4(h, es, ec, full, tp, tq, vt_top);
        if (side + 1 < sides) store_proj(mem.park, 0, h);
    }
    // both encodings from one inversion: 1 / (Z_G Z_H), times the other's Z
    uint32_t pg[8], ph[8];
    if (linkable) {
        fe zg, zz, inv, zi;
        load_fe(zg, mem.park + 20);
        fe_mul(zz, zg, h.Z);
        fe_invert(inv, zz);
        fe_mul(zi, inv, zg);
        ge_encode_with_zinv(ph, h.X, h.Y, zi);
        fe_mul(zi, inv, h.Z);
        load_fe(h.X, mem.park);
        load_fe(h.Y, mem.park + 10);
        ge_encode_with_zinv(pg, h.X, h.Y, zi);
    } else {
        ge_p3_towords(pg, h);
#pragma unroll
        for (int i = 0; i < 8; i++) ph[i] = 0;
    }
    return ed_ring_finish(c, mem.mid, pg, ph, linkable);
}

// What the chain reads of one signature.  keys: the signature's own ring (32-byte encodings), or nullptr when the call
// shares one ring and sh holds its tables.  sig: c || s_0 .. s_{ring-1} || [tag], 16-byte aligned.
struct EdRingSig {
    size_t ring;
    const uint32_t* keys;
    const uint32_t* sig;
    const uint8_t* msg;
    size_t len;
    const uint8_t* scope;
    size_t scope_len;
};

// The whole chain of one signature: `steps` positions from `start`, wrapping modulo ring, entered with the challenge in
// slot 0.  c: the last challenge; mem.mid->czero: the challenge that entered position 0 (the input challenge when
// start == 0, zero if position ring - 1 was never run).  Status: ED_ST_PICK_EXHAUSTED, else ED_ST_BAD_POINT when
// linkBase, the tag or a ring member that the chain visited does not decode.  Every lane of a wave runs the same
// number of steps (the variable-time chain's wave reductions want every lane).
KYB_DEV int ed_ring_lane(uint32_t (&c)[8], const EdRingSig& s, size_t start, size_t steps, bool full, const EdRingShared& sh,
                         const EdRingLaneMem& mem) {
    const bool linkable = s.scope != nullptr;
    bool bad = false, exhausted = false;
    {  // first: the hash's working set and a point's never meet in the registers
        uint32_t tw[8], tc[8];
        if (linkable) {
            load_words8(tw, s.sig + 8 * (1 + s.ring));
            ed_canon_point_bytes(tc, tw);
#pragma unroll
            for (int i = 0; i < 8; i++) reinterpret_cast<uint32_t*>(mem.park)[i] = tc[i];  // read byte by byte below
        }
        EdRingPrefix pre{s.msg, s.len, s.scope, s.scope_len, reinterpret_cast<const uint8_t*>(mem.park)};
        ed_ring_absorb_prefix(mem.mid, pre);
        if (linkable) {
            bad |= !ed_ring_table(mem.tag_tab, tw);
            bad |= sh.bad[ED_RING_TAB_LINK] != 0;
        }
    }
    load_words8(c, s.sig);
    size_t pos = start;
#pragma unroll
    for (int i = 0; i < 8; i++) mem.mid->czero[i] = pos == 0 ? c[i] : 0u;
#pragma unroll 1
    for (size_t k = 0; k < steps; k++) {
        uint32_t sw[8];
        const int4* tx;
        if (s.keys) {
            load_words8(sw, s.keys + 8 * pos);
            bad |= !ed_ring_table(mem.key_tab, sw);
            tx = mem.key_tab;
        } else {
            bad |= sh.bad[ED_RING_TAB_KEYS + pos] != 0;
            tx = sh.tabs + (ED_RING_TAB_KEYS + pos) * 80;
        }
        load_words8(sw, s.sig + 8 * (1 + pos));
        exhausted |= ed_ring_step(c, sw, full, linkable, sh, tx, mem) == 0;
        pos = pos + 1 == s.ring ? 0 : pos + 1;
        if (pos == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) mem.mid->czero[i] = c[i];
        }
    }
    return exhausted ? ED_ST_PICK_EXHAUSTED : (bad ? ED_ST_BAD_POINT : ED_ST_OK);
}

// signH1 alone (sig.go:34-43 over sig.go:23-32): c = Pick(XOF(m || [scope || canon(tag)]) || PG || [PH]).  pg, ph: the
// bytes MarshalBinary wrote, hashed as they are.  mid: scratch memory of the lane; tagmem: 32 bytes of it.
KYB_DEV int ed_ring_challenge_lane(uint32_t (&c)[8], const uint8_t* msg, size_t len, const uint8_t* scope, size_t scope_len,
                                   const uint32_t tag[8], const uint32_t pg[8], const uint32_t ph[8], EdRingMid* mid,
                                   uint32_t* tagmem) {
    const bool linkable = scope != nullptr;
    if (linkable) {
        uint32_t tc[8];
        ed_canon_point_bytes(tc, tag);
#pragma unroll
        for (int i = 0; i < 8; i++) tagmem[i] = tc[i];
    }
    EdRingPrefix pre{msg, len, scope, scope_len, reinterpret_cast<const uint8_t*>(tagmem)};
    ed_ring_absorb_prefix(mid, pre);
    return ed_ring_finish(c, mid, pg, ph, linkable) ? ED_ST_OK : ED_ST_PICK_EXHAUSTED;
}

}  // namespace kyb
