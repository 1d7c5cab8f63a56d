"""The table of sharded host entries: every public call that reaches an `md_active(` site of kyber_amd/csrc, as rows
built on the oracles alone (no GPU, no engine), shared by tests/test_shard_sites.py (the table held to the sources and to
itself, on the CPU) and tests/test_gpu_sharded_entries.py (every row run with a device set against the single-device
call and against the expectations below).

A row's builder make(n, world) returns a Case: the arguments of the C ABI call (numpy arrays for the inputs, Out() for
the outputs, Dst() for a domain separation tag, integers and None as they are), the expected status byte of EVERY
element, the expected verdict (`ok`) of every element where the entry has one, and the expected bytes of every output
at the CHECK rows: the boundary rows lo - 1, lo, hi - 1 of every shard (kyber_amd.devices.shard_range), 0 and n - 1,
and the planted rows.  Planted rows are the ones the single-device path answers with a status or with ok = 0; they sit
on the boundary rows of the MIDDLE shard and on the last row, so a slice that reads its neighbour's operand flips a
byte the table knows.  Any two adjacent rows differ in every per-element operand.

Expectations are the existing restatements': tests/_ed_verify_oracle.py, mul2_oracle of tests/test_ed_verify_host.py,
tests/_pvss_oracle.py, tests/_anon_oracle.py, tests/_shuffle_cases.py, tests/_ibe_oracle.py, tests/_oracle_c.py (bulk
Ed25519 products and the BLS12-381 / bn256 pairings) and the decoding rules of oracle/*.py.  Points of the pairing groups
are links of chains of oracle additions (tests/_add_cases.py), so a row costs a few dozen big-integer multiplications.
Where only the engine can make bulk filler (a few hundred BLS signatures or IBE ciphertexts) the Case carries fill(): the
GPU test runs it with the device set cleared, and it writes the rows the table holds no expectation of output bytes
for; their verdicts (valid by construction) are still the table's."""
import functools
import hashlib
import random
from collections import namedtuple

import numpy as np

from kyber_amd.devices import shard_range
from kyber_amd.util import blake2xb
from oracle import bls12381 as OB, bn254 as ON4, bn256 as ON, ed25519 as O
from tests import _add_cases as AC
from tests import _anon_oracle as A
from tests import _ed_verify_oracle as V
from tests import _ibe_oracle as IO
from tests import _oracle_c as OC
from tests import _pvss_oracle as PO
from tests import _shuffle_cases as SC
from tests._dkg_cases import ORDER8, UNDECODABLE
from tests.test_ed_verify_host import mul2_oracle

# (source file, enclosing function) of every `md_active(` outside context.h
SITES = frozenset({
    ("ed25519.hip", "kyb_ed25519_mul_base"), ("ed25519.hip", "kyb_ed25519_mul"), ("ed25519.hip", "kyb_ed25519_mul_same_base"),
    ("ed25519_verify.hip", "kyb_ed25519_verify"), ("ed25519_verify.hip", "kyb_ed25519_mul2"),
    ("ed25519_dleq.hip", "kyb_ed25519_dleq_challenge"), ("ed25519_dleq.hip", "kyb_ed25519_dleq_verify"),
    ("ed25519_ring.hip", "kyb_ed25519_ring_chain"), ("ed25519_ring.hip", "kyb_ed25519_ring_challenge"),
    ("ed25519_shuffle.hip", "kyb_ed25519_theta_check"),
    ("pairing_abi.cuh", "mul_host"), ("pairing_abi.cuh", "pair_host"), ("pairing_abi.cuh", "pair_check_host"),
    ("bls12381_h2c.hip", "kyb_bls12381_verify_g1"), ("bls12381_h2c.hip", "kyb_bls12381_verify_g1_same_key"),
    ("bls12381_h2c.hip", "kyb_bls12381_verify_g1_same_msg"), ("bls12381_h2c.hip", "kyb_bls12381_verify_g2"),
    ("bls12381_ibe.hip", "encrypt_host"), ("bls12381_ibe.hip", "decrypt_host"),
    ("msm.cuh", "run_host"),
})

F_VARTIME, F_UNIFORM, F_DLEQ_FS, F_UNC, F_UNC_OUT, F_TRUSTED0 = 1, 8, 16, 2, 4, 0x100  # include/kyber_hip.h
# the status codes a row may expect (include/kyber_hip.h)
ST_OK, ST_BAD_POINT, ST_NOT_IN_SUBGROUP, ST_IBE_CHECK, ST_SIG_NONCANONICAL, ST_SIG_SMALL_ORDER, ST_DLEQ_CHALLENGE = 0, 1, 2, 3, 5, 6, 7
DOCUMENTED = {ST_OK, ST_BAD_POINT, ST_NOT_IN_SUBGROUP, ST_IBE_CHECK, ST_SIG_NONCANONICAL, ST_SIG_SMALL_ORDER, ST_DLEQ_CHALLENGE}
MSG_CYCLE = (0, 1, 31, 32, 33, 63, 64, 65, 111, 112, 113, 127, 128, 129)  # both SHA-512 block edges behind R || A

Out = namedtuple("Out", "name shape null", defaults=(False,))  # null: the call gets NULL; the array must keep its canary
Dst = namedtuple("Dst", "tag")
Plant = namedtuple("Plant", "label status ok")  # ok None: the entry has no verdict array


class Case:
    """entry(*args) and what must come back.  status: (n,) uint8 or None (no status array); ok: (n,) uint8 or None;
    expect: {output name: {row: bytes}}; planted: {row: Plant}; whole: {output name: bytes} for an output that is not
    per element (an MSM's sum)."""

    def __init__(self, entry, args, n, world, status=None, ok=None, expect=None, planted=None, whole=None, fill=None, notes=None):
        self.entry, self.args, self.n, self.world = entry, args, n, world
        self.status, self.ok, self.expect, self.planted = status, ok, expect or {}, planted or {}
        self.whole, self.fill, self.notes = whole or {}, fill, notes or {}

    def outs(self):
        return [a for a in self.args if isinstance(a, Out)]


Row = namedtuple("Row", "name site make cheap")
ROWS = {}


def _row(name, site, make, cheap=False):
    assert site in SITES and name not in ROWS, name
    ROWS[name] = Row(name, site, make, cheap)


# --------------------------------------------------------------------------------------------------- the partition
def bounds(n, world):
    return [shard_range(n, r, world) for r in range(world)]


def boundary_rows(n, world):
    rows = {0, n - 1}
    for lo, hi in bounds(n, world):
        if hi > lo:
            rows |= {lo - 1, lo, hi - 1}
    return sorted(r for r in rows if 0 <= r < n)


def plant_rows(n, world):
    """where planted rows go, in the order they are handed out: the middle shard's first and last row, the batch's last
    row, then the rows that touch the middle shard from outside"""
    lo, hi = bounds(n, world)[world // 2]
    out = []
    for r in (lo, hi - 1, n - 1, lo - 1, hi):
        if 0 <= r < n and r not in out:
            out.append(r)
    return out


def _check_rows(n, world, planted=()):
    return sorted(set(boundary_rows(n, world)) | set(planted))


def _shake(label, nbytes):
    return np.frombuffer(hashlib.shake_256(b"shard cases/" + label).digest(nbytes), dtype=np.uint8).copy()


def _rows32(label, n, top=0x0F):
    """n distinct little-endian scalars below 2^(248 + bits of top)"""
    s = _shake(label, n * 32).reshape(n, 32)
    s[:, 31] &= top
    return s


def _arr(rows, width):
    return np.frombuffer(b"".join(bytes(r) for r in rows), dtype=np.uint8).reshape(len(rows), width).copy()


def _le(b):
    return int.from_bytes(bytes(b), "little")


def _sc(v):
    return (v % O.L).to_bytes(32, "little")


def _plant(kinds, n, world):
    """{row: kind} for as many of the kinds as there are places"""
    return dict(zip(plant_rows(n, world), kinds))


def msg_lengths(n, world):
    """lengths cycling through MSG_CYCLE, the first message of every shard empty, an odd byte count in front of every
    shard but the first (where a shard has a row to spare for the parity)"""
    ln = [MSG_CYCLE[i % len(MSG_CYCLE)] for i in range(n)]
    bs = bounds(n, world)
    for lo, hi in bs:
        if hi > lo:
            ln[lo] = 0
    for r in range(1, world):
        (plo, phi), (lo, hi) = bs[r - 1], bs[r]
        if hi > lo and phi - plo >= 3 and sum(ln[:lo]) % 2 == 0:
            ln[plo + 1] += 1
    return ln


def _messages(label, n, world):
    ln = msg_lengths(n, world)
    blob = _shake(label, sum(ln) + 1)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(ln, out=off[1:])
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(n)], blob[:max(1, int(off[n]))].copy(), off


# ======================================================================================================== Ed25519
@functools.lru_cache(maxsize=None)
def _ed_points(label, n):
    """n distinct points of the prime-order subgroup and their discrete logarithms"""
    k = _rows32(label, n)
    return k, OC.ed_mul_base(k, OC.host_threads())


def _make_mul_base(flags):
    def make(n, world):
        s = _rows32(b"mul_base/s", n, 0x7F)
        rows = _check_rows(n, world)
        return Case("kyb_ed25519_mul_base", [n, s, Out("out", (n, 32)), flags], n, world,
                    expect={"out": {i: O.mul_base(bytes(s[i])) for i in rows}})
    return make


def _make_mul(flags):
    def make(n, world):
        s = _rows32(b"mul/s", n, 0x7F)
        P = _ed_points(b"mul/P", n)[1].copy()
        planted = _plant(["undecodable point"] * 3, n, world)
        for r in planted:
            P[r] = np.frombuffer(UNDECODABLE, dtype=np.uint8)
        status, exp = np.zeros(n, dtype=np.uint8), {}
        for i in _check_rows(n, world, planted):
            v = O.mul(bytes(s[i]), bytes(P[i]), bool(flags & F_VARTIME))
            status[i] = ST_OK if v is not None else ST_BAD_POINT
            exp[i] = v or bytes(32)
        return Case("kyb_ed25519_mul", [n, s, P, Out("out", (n, 32)), Out("status", (n,)), flags], n, world, status=status,
                    expect={"out": exp}, planted={r: Plant(k, ST_BAD_POINT, None) for r, k in planted.items()})
    return make


def _make_mul_same_base(flags, bad_base=False):
    def make(n, world):
        s = _rows32(b"same_base/s", n, 0x7F)
        base = UNDECODABLE if bad_base else bytes(_ed_points(b"same_base/P", 8)[1][5])
        status = np.full(n, ST_BAD_POINT if bad_base else ST_OK, dtype=np.uint8)
        exp = {i: bytes(32) if bad_base else O.mul(bytes(s[i]), base, bool(flags & F_VARTIME)) for i in _check_rows(n, world)}
        return Case("kyb_ed25519_mul_same_base", [n, s, _arr([base], 32), Out("out", (n, 32)), Out("status", (n,)), flags], n, world,
                    status=status, expect={"out": exp})
    return make


def _make_verify(variant):
    """variant: "messages", "empty" (every message empty, msgs NULL) or "no status" (status NULL)"""
    def make(n, world):
        a, pubs = _ed_points(b"verify/a", n)
        r, R = _ed_points(b"verify/r", n)
        pubs = pubs.copy()
        if variant == "empty":
            msgs, blob, off = [b""] * n, None, np.zeros(n + 1, dtype=np.uint64)
        else:
            msgs, blob, off = _messages(b"verify/m", n, world)
        sigs = np.zeros((n, 64), dtype=np.uint8)
        for i in range(n):
            h = _le(hashlib.sha512(bytes(R[i]) + bytes(pubs[i]) + msgs[i]).digest()) % O.L
            sigs[i] = np.frombuffer(bytes(R[i]) + _sc(_le(r[i]) + h * _le(a[i])), dtype=np.uint8)
        kinds = {"undecodable key": ST_BAD_POINT, "small-order key": ST_SIG_SMALL_ORDER, "non-canonical S": ST_SIG_NONCANONICAL,
                 "forged": ST_OK}
        planted = _plant(list(kinds), n, world)
        for row, kind in planted.items():
            if kind == "undecodable key":
                pubs[row] = np.frombuffer(UNDECODABLE, dtype=np.uint8)
            elif kind == "small-order key":
                pubs[row] = np.frombuffer(ORDER8, dtype=np.uint8)
            elif kind == "non-canonical S":
                sigs[row, 32:] = np.frombuffer((_le(sigs[row, 32:]) + O.L).to_bytes(32, "little"), dtype=np.uint8)
            else:
                sigs[row, 32:] = np.frombuffer(_sc(_le(sigs[row, 32:]) + 1), dtype=np.uint8)
        ok, status = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for i in _check_rows(n, world, planted):  # the restatement's word at every check row, planted or not
            c = (bytes(pubs[i]), msgs[i], bytes(sigs[i]))
            ok[i], status[i] = int(V.verify_with_checks(*c)[0]), V.abi_status(*c)
            assert (ok[i], status[i]) == ((0, kinds[planted[i]]) if i in planted else (1, 0)), (i, planted.get(i))
        st = Out("status", (n,), variant == "no status")
        return Case("kyb_ed25519_verify", [n, pubs, blob, off, sigs, Out("ok", (n,)), st, 0], n, world,
                    status=None if st.null else status, ok=ok, planted={r: Plant(k, kinds[k], 0) for r, k in planted.items()},
                    notes={"off": off, "lengths": [len(m) for m in msgs]})
    return make


def _make_mul2(flags):
    def make(n, world):
        a, b = _rows32(b"mul2/a", n, 0x7F), _rows32(b"mul2/b", n, 0x7F)
        P, Q = _ed_points(b"mul2/P", n)[1].copy(), _ed_points(b"mul2/Q", n)[1].copy()
        planted = _plant(["undecodable P", "undecodable Q", "both undecodable"], n, world)
        bad = np.frombuffer(UNDECODABLE, dtype=np.uint8)
        for row, kind in planted.items():
            if kind != "undecodable Q":
                P[row] = bad
            if kind != "undecodable P":
                Q[row] = bad
        status, exp = np.zeros(n, dtype=np.uint8), {}
        for i in _check_rows(n, world, planted):
            v = mul2_oracle(bytes(a[i]), bytes(P[i]), bytes(b[i]), bytes(Q[i]), bool(flags & F_VARTIME))
            status[i] = ST_OK if v is not None else ST_BAD_POINT
            exp[i] = v or bytes(32)
        return Case("kyb_ed25519_mul2", [n, a, P, b, Q, Out("out", (n, 32)), Out("status", (n,)), flags], n, world, status=status,
                    expect={"out": exp}, planted={r: Plant(k, ST_BAD_POINT, None) for r, k in planted.items()})
    return make


def _make_dleq_challenge(n, world):
    cols = [_shake(b"dleq_challenge/%d" % k, n * 32).reshape(n, 32) for k in range(4)]
    special = [(O.P + 1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little"), (2**256 - 1).to_bytes(32, "little")]
    for k, row in enumerate(plant_rows(n, world)[:3]):  # non-canonical encodings: the challenge is defined on every input
        cols[k][row] = np.frombuffer(special[k], dtype=np.uint8)
    exp = {i: PO.device_challenge(*(bytes(c[i]) for c in cols)) for i in _check_rows(n, world)}
    return Case("kyb_ed25519_dleq_challenge", [n] + cols + [Out("c", (n, 32)), Out("status", (n,))], n, world,
                status=np.zeros(n, dtype=np.uint8), expect={"c": exp})


def _make_dleq_verify(g_stride, h_stride, mode):
    """mode: "expect" (expect_c given), "fs" (KYB_F_DLEQ_FS) or "free" (neither)"""
    def make(n, world):
        G, H = _ed_points(b"dleq/G", n)[1].copy(), _ed_points(b"dleq/H", n)[1].copy()
        if not g_stride:
            G[:] = G[7 % n]
        if not h_stride:
            H[:] = H[11 % n]
        x, v = _rows32(b"dleq/x", n), _rows32(b"dleq/v", n)
        th = OC.host_threads()
        xG, xH, vG, vH = (OC.ed_mul(k, p, False, th)[0] for k, p in ((x, G), (x, H), (v, G), (v, H)))
        C = _rows32(b"dleq/c", n)
        expect_c = None
        if mode == "expect":
            expect_c = C[3 % n].copy()
            C[:] = expect_c
        elif mode == "fs":
            for i in range(n):
                C[i] = np.frombuffer(PO.device_challenge(bytes(xG[i]), bytes(xH[i]), bytes(vG[i]), bytes(vH[i])), dtype=np.uint8)
        R = _arr([_sc(_le(v[i]) - _le(C[i]) * _le(x[i])) for i in range(n)], 32)
        kinds = {"challenge altered": ST_OK if mode == "free" else ST_DLEQ_CHALLENGE, "undecodable xG": ST_BAD_POINT,
                 "response altered": ST_OK}
        if g_stride:
            kinds["undecodable G"] = ST_BAD_POINT
        planted = _plant(list(kinds), n, world)
        bad = np.frombuffer(UNDECODABLE, dtype=np.uint8)
        for row, kind in planted.items():
            if kind == "challenge altered":
                C[row, 0] ^= 1
            elif kind == "response altered":
                R[row, 0] ^= 1
            elif kind == "undecodable G":
                G[row] = bad
            else:
                xG[row] = bad
                if mode == "fs":  # the challenge of the row as it now is: the point's status is what is left to find
                    C[row] = np.frombuffer(PO.device_challenge(bytes(xG[row]), bytes(xH[row]), bytes(vG[row]), bytes(vH[row])), dtype=np.uint8)
        ok, status = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for i in _check_rows(n, world, planted):
            f = [bytes(c[i]) for c in (G, H, xG, xH, C, R, vG, vH)]
            status[i] = PO.abi_status(*f[:5], expect_c=None if expect_c is None else bytes(expect_c), fs_with=(f[6], f[7]) if mode == "fs" else None)
            ok[i] = int(status[i] == 0 and PO.dleq_verify(*f))
            assert (ok[i], status[i]) == ((0, kinds[planted[i]]) if i in planted else (1, 0)), (i, planted.get(i))
        Ga, Ha = (G if g_stride else G[:1].copy()), (H if h_stride else H[:1].copy())
        args = [n, Ga, g_stride, Ha, h_stride, xG, xH, C, R, vG, vH, None if expect_c is None else expect_c.reshape(1, 32),
                Out("ok", (n,)), Out("status", (n,)), F_DLEQ_FS if mode == "fs" else 0]
        return Case("kyb_ed25519_dleq_verify", args, n, world, status=status, ok=ok,
                    planted={r: Plant(k, kinds[k], 0) for r, k in planted.items()}, notes={"one value": [C] if mode == "expect" else []})
    return make


RING = 2
RING_SCOPE = b"shard cases scope"


@functools.lru_cache(maxsize=None)
def _ring_signed(n, world, shared, linkable):
    """(keys (n or 1, RING, 32), messages, blob, off, sigs (n, slots * 32), planted): random signature bytes everywhere,
    the oracle's signatures at the check rows (signer RING - 1), then the planted alterations"""
    slots = RING + (2 if linkable else 1)
    scope = RING_SCOPE if linkable else None
    tag_of = lambda i: "%d/%d/%d/%d" % (n, world, shared, linkable) + "/%d" % i
    msgs, blob, off = _messages(b"ring/m", n, world)
    nk = 1 if shared else n
    xs = _rows32(b"ring/x", nk)
    keys = OC.ed_mul_base(_rows32(b"ring/k", nk * RING), OC.host_threads()).reshape(nk, RING, 32).copy()
    keys[:, RING - 1] = OC.ed_mul_base(xs, OC.host_threads())
    sigs = _rows32(b"ring/sig", n * slots).reshape(n, slots * 32)
    if linkable:  # a tag is a point: somebody's x times the link base
        sigs[:, 32 * (RING + 1):] = _ed_points(b"ring/tag", n)[1]
    kinds = ["s altered"] + ([] if shared else ["key undecodable"]) + (["tag undecodable"] if linkable else [])
    planted = _plant(kinds, n, world)
    for i in _check_rows(n, world, planted):
        k = i if not shared else 0
        sig = A.sign(msgs[i], [bytes(p) for p in keys[k]], scope, RING - 1, bytes(xs[k]), blake2xb.New(tag_of(i).encode()))
        sigs[i] = np.frombuffer(sig, dtype=np.uint8)
    bad = np.frombuffer(UNDECODABLE, dtype=np.uint8)
    for row, kind in planted.items():
        if kind == "s altered":
            sigs[row, 32] ^= 1
        elif kind == "key undecodable":
            keys[row, 0] = bad
        else:
            sigs[row, 32 * (RING + 1):] = bad
    return keys, msgs, blob, off, sigs, planted


def _make_ring_chain(shared, with_start, with_c_zero, linkable):
    def make(n, world):
        keys, msgs, blob, off, sigs, planted = _ring_signed(n, world, shared, linkable)
        slots = RING + (2 if linkable else 1)
        scope = RING_SCOPE if linkable else None
        start = (np.arange(n, dtype=np.uint32) * 7 + 1) % RING if with_start else None
        ok, status = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        exp = {"c_zero": {}, "c_out": {}}
        for i in _check_rows(n, world, planted):
            cz, co, ok[i], status[i] = A.chain(msgs[i], [bytes(p) for p in keys[0 if shared else i]], scope, bytes(sigs[i]),
                                               start=int(start[i]) if with_start else 0, steps=RING)
            exp["c_zero"][i], exp["c_out"][i] = cz, co
            valid = i not in planted and not (with_start and start[i])
            assert (ok[i], status[i]) == ((1, 0) if valid else (0, status[i])), i
        plants = {r: Plant(k, ST_OK if k == "s altered" else ST_BAD_POINT, 0) for r, k in planted.items()}
        assert all(status[r] == p.status and not ok[r] for r, p in plants.items())
        if not with_c_zero:
            del exp["c_zero"]
        args = [n, RING, keys.reshape(-1, 32 * RING), 0 if shared else 32 * RING, blob, off,
                None if scope is None else np.frombuffer(scope, dtype=np.uint8).copy(), len(scope or b""),
                None if scope is None else _arr([A.link_base(scope)], 32), sigs, 32 * slots, start, RING,
                Out("c_zero", (n, 32), not with_c_zero), Out("c_out", (n, 32)), Out("ok", (n,)), Out("status", (n,)), 0]
        # (a filler row is random bytes under a ring's keys: no signature, ok = 0 by all but a 2^-252 chance)
        return Case("kyb_ed25519_ring_chain", args, n, world, status=status, ok=ok, expect=exp, planted=plants,
                    notes={"off": off, "lengths": [len(m) for m in msgs]})
    return make


def _make_ring_challenge(linkable):
    def make(n, world):
        msgs, blob, off = _messages(b"ring_challenge/m", n, world)
        PG = _shake(b"ring_challenge/PG", n * 32).reshape(n, 32)
        tags = PH = scope = None
        if linkable:
            scope = RING_SCOPE
            tags, PH = _ed_points(b"ring_challenge/tag", n)[1].copy(), _shake(b"ring_challenge/PH", n * 32).reshape(n, 32)
            for k, row in enumerate(plant_rows(n, world)[:2]):  # a tag is hashed through its canonical bytes
                tags[row] = np.frombuffer([(O.P + 1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little")][k], dtype=np.uint8)
        exp = {i: A.h1(msgs[i], scope, A.canon_bytes(bytes(tags[i])) if linkable else None, bytes(PG[i]),
                       bytes(PH[i]) if linkable else None) for i in _check_rows(n, world)}
        args = [n, blob, off, None if scope is None else np.frombuffer(scope, dtype=np.uint8).copy(), len(scope or b""), tags, PG, PH,
                Out("c", (n, 32)), Out("status", (n,))]
        return Case("kyb_ed25519_ring_challenge", args, n, world, status=np.zeros(n, dtype=np.uint8), expect={"c": exp},
                    notes={"off": off, "lengths": [len(m) for m in msgs]})
    return make


def _make_theta(flags):
    def make(n, world):
        a, b = _rows32(b"theta/a", n, 0x7F), _rows32(b"theta/b", n, 0x7F)
        A_, B = _ed_points(b"theta/A", n)[1].copy(), _ed_points(b"theta/B", n)[1].copy()
        U, W = SC._pt(0xABCDEF0123), SC._pt(0x9876543210FF)
        add = lambda p, q: O.encode(O.add(O.decode(bytes(p)), O.decode(bytes(q))))
        xhat, yhat = _arr([add(p, U) for p in A_], 32), _arr([add(p, W) for p in B], 32)
        nb = _arr([_sc(-_le(x)) for x in b], 32)
        th = OC.host_threads()
        vt = bool(flags & F_VARTIME)
        T = _arr([add(p, q) for p, q in zip(OC.ed_mul(a, xhat, vt, th)[0], OC.ed_mul(nb, yhat, vt, th)[0])], 32)
        kinds = {"undecodable A": ST_BAD_POINT, "T moved": ST_OK, "undecodable B": ST_BAD_POINT}
        planted = _plant(list(kinds), n, world)
        bad = np.frombuffer(UNDECODABLE, dtype=np.uint8)
        for row, kind in planted.items():
            if kind == "undecodable A":
                A_[row] = bad
            elif kind == "undecodable B":
                B[row] = bad
            else:
                T[row] = np.frombuffer(add(T[row], SC._pt(1)), dtype=np.uint8)
        ok, status = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for i in _check_rows(n, world, planted):
            ok[i], status[i] = SC.expect(bytes(a[i]), bytes(A_[i]), U, bytes(b[i]), bytes(B[i]), W, bytes(T[i]), vt)
            assert (ok[i], status[i]) == ((0, kinds[planted[i]]) if i in planted else (1, 0)), (i, planted.get(i))
        args = [n, a, A_, _arr([U], 32), b, B, _arr([W], 32), T, Out("ok", (n,)), Out("status", (n,)), flags]
        return Case("kyb_ed25519_theta_check", args, n, world, status=status, ok=ok,
                    planted={r: Plant(k, kinds[k], 0) for r, k in planted.items()})
    return make


def _make_ed_msm(with_reject):
    def make(n, world):
        s = _rows32(b"msm/s", n, 0x7F)
        P = _ed_points(b"msm/P", n)[1].copy()
        status = np.zeros(n, dtype=np.uint8)
        planted = _plant(["undecodable point"] * 2, n, world) if with_reject else {}
        for r in planted:
            P[r] = np.frombuffer(UNDECODABLE, dtype=np.uint8)
            status[r] = ST_BAD_POINT
        total = bytes(32) if with_reject else O.msm([bytes(x) for x in s], [bytes(p) for p in P])
        return Case("kyb_ed25519_msm", [n, s, P, Out("out", (32,)), Out("status", (n,))], n, world, status=status,
                    whole={"out": total}, planted={r: Plant(k, ST_BAD_POINT, None) for r, k in planted.items()})
    return make


_ED, _EDV, _EDD, _EDR, _EDS = "ed25519.hip", "ed25519_verify.hip", "ed25519_dleq.hip", "ed25519_ring.hip", "ed25519_shuffle.hip"
for _name, _f in (("", 0), ("/uniform", F_UNIFORM)):
    _row("ed25519/mul_base" + _name, (_ED, "kyb_ed25519_mul_base"), _make_mul_base(_f), cheap=not _f)
for _name, _f in (("", 0), ("/uniform", F_UNIFORM), ("/vartime", F_VARTIME)):
    _row("ed25519/mul" + _name, (_ED, "kyb_ed25519_mul"), _make_mul(_f))
    _row("ed25519/mul_same_base" + _name, (_ED, "kyb_ed25519_mul_same_base"), _make_mul_same_base(_f))
_row("ed25519/mul_same_base/undecodable base", (_ED, "kyb_ed25519_mul_same_base"), _make_mul_same_base(0, True))
for _v in ("messages", "empty", "no status"):
    _row("ed25519/verify/" + _v, (_EDV, "kyb_ed25519_verify"), _make_verify(_v), cheap=_v == "messages")
for _name, _f in (("", 0), ("/vartime", F_VARTIME)):
    _row("ed25519/mul2" + _name, (_EDV, "kyb_ed25519_mul2"), _make_mul2(_f))
    _row("ed25519/theta_check" + _name, (_EDS, "kyb_ed25519_theta_check"), _make_theta(_f), cheap=not _f)
_row("ed25519/dleq_challenge", (_EDD, "kyb_ed25519_dleq_challenge"), _make_dleq_challenge, cheap=True)
for _g in (0, 32):
    for _h in (0, 32):
        for _m in ("expect", "fs", "free"):
            _row("ed25519/dleq_verify/g%d/h%d/%s" % (_g, _h, _m), (_EDD, "kyb_ed25519_dleq_verify"), _make_dleq_verify(_g, _h, _m))
for _sh in (True, False):
    for _st in (False, True):
        for _cz in (True, False):
            for _lk in (False, True):
                _row("ed25519/ring_chain/%s/%s/%s/%s" % ("one ring" if _sh else "ring each", "start" if _st else "no start",
                                                       "c_zero" if _cz else "no c_zero", "linkable" if _lk else "unlinkable"),
                     (_EDR, "kyb_ed25519_ring_chain"), _make_ring_chain(_sh, _st, _cz, _lk))
for _lk in (False, True):
    _row("ed25519/ring_challenge/" + ("linkable" if _lk else "unlinkable"), (_EDR, "kyb_ed25519_ring_challenge"),
         _make_ring_challenge(_lk), cheap=not _lk)
_row("ed25519/msm", ("msm.cuh", "run_host"), _make_ed_msm(False), cheap=True)
_row("ed25519/msm/rejects", ("msm.cuh", "run_host"), _make_ed_msm(True))


# ================================================================================================ pairing suites
class Suite:
    """one pairing suite's oracle: encodings under the flags, decoding statuses, scalar multiplications and pairings"""

    def __init__(self, name):
        self.name, self.bls = name, name == "bls12381"
        self.M = {"bls12381": OB, "bn256": ON, "bn254": ON4}[name]
        self.G = {1: AC.group(name + "-g1"), 2: AC.group(name + "-g2")}
        self.order = OB.R if self.bls else self.M.ORDER
        self.gt_size = 576 if self.bls else 384
        self._mul, self._pair = {}, {}

    def width(self, g, unc):
        return self.G[g].width * (2 if self.bls and unc else 1)

    def enc(self, g, pt, unc):
        if self.bls and unc:
            return (OB.g1_serialize_unc if g == 1 else OB.g2_serialize_unc)(pt)
        return self.G[g]._enc(pt)

    def status(self, g, buf, unc):
        """UnmarshalBinary's verdict on an encoding, from the oracle's decoders"""
        if not self.bls:
            try:
                (self.M.g1_unmarshal if g == 1 else self.M.g2_unmarshal)(bytes(buf))
                return ST_OK
            except self.M.DecodeError:
                return ST_BAD_POINT
        try:
            if unc:
                pt = (OB.g1_deserialize_unc if g == 1 else OB.g2_deserialize_unc)(bytes(buf), validate=False)
                if pt is not None and not (OB.g1_on_curve if g == 1 else OB.g2_on_curve)(pt):
                    return ST_BAD_POINT
            else:
                pt = (OB.g1_decompress if g == 1 else OB.g2_decompress)(bytes(buf), subgroup_check=False)
        except OB.DecodeError:
            return ST_BAD_POINT
        return ST_OK if pt is None or (OB.g1_in_subgroup if g == 1 else OB.g2_in_subgroup)(pt) else ST_NOT_IN_SUBGROUP

    def mul(self, g, k, pt):
        key = (g, k, pt)
        if key not in self._mul:
            self._mul[key] = None if pt is None else self.G[g].mul(k % self.order, pt)
        return self._mul[key]

    def pair(self, p, q):
        """the GT bytes of e(p, q), p and q valid finite points"""
        if (p, q) not in self._pair:
            a, b = self.G[1]._enc(p), self.G[2]._enc(q)
            if self.name == "bls12381":
                gt, st = OC.bls12381_pair_compressed(a, b, 1)
            elif self.name == "bn256":
                gt, st = OC.bn256_pair(a, b, 1)
            else:
                gt, st = [ON4.pair_bytes(a, b)], [0]
            assert not st[0]
            self._pair[(p, q)] = bytes(gt[0])
        return self._pair[(p, q)]

    def scalar(self, label):
        return int.from_bytes(hashlib.shake_256(b"shard cases/" + self.name.encode() + label).digest(40), "big") % (self.order - 1) + 1

    @functools.lru_cache(maxsize=None)
    def line(self, g, label, n):
        """(scalars, points): k_i = a + i d and k_i * generator, by a chain of additions"""
        G, a, d = self.G[g], self.scalar(label + b"/a"), self.scalar(label + b"/d")
        p, step, ks, pts = G.mul(a, G.gen), G.mul(d, G.gen), [], []
        for i in range(n):
            ks.append((a + i * d) % self.order)
            pts.append(p)
            p = G.add(p, step)
        return ks, pts

    @functools.lru_cache(maxsize=None)
    def product_line(self, g, label1, label2, n):
        """(k1_i k2_i) * generator for two lines: second differences are constant, two additions a row"""
        G = self.G[g]
        a, b = self.scalar(label1 + b"/a"), self.scalar(label1 + b"/d")
        c, d = self.scalar(label2 + b"/a"), self.scalar(label2 + b"/d")
        p, delta, dd = G.mul(a * c % self.order, G.gen), G.mul((a * d + b * c + b * d) % self.order, G.gen), G.mul(2 * b * d % self.order, G.gen)
        pts = []
        for _ in range(n):
            pts.append(p)
            p, delta = G.add(p, delta), G.add(delta, dd)
        return pts

    @functools.lru_cache(maxsize=None)
    def rejects(self, g, unc):
        """{kind: encoding}: a break of the encoding's flag rule (BN: a point off the curve), a curve point outside the
        subgroup (BLS12-381), and infinity, which is no reject"""
        G, rng = self.G[g], random.Random("shard cases/%s/%d" % (self.name, g))
        good = self.enc(g, self.line(g, b"rejects", 4)[1][2], unc)
        out = {"infinity": self.enc(g, None, unc)}
        if self.bls:
            out["flag rule"] = bytes([good[0] | 0x80]) + good[1:] if unc else bytes([good[0] & 0x7F]) + good[1:]
            while True:
                pt = AC._on_curve_x(G, OB, rng)
                if self.status(g, self.enc(g, pt, unc), unc) == ST_NOT_IN_SUBGROUP:
                    break
            out["off subgroup"] = self.enc(g, pt, unc)
        else:
            w = len(good)
            out["off curve"] = good[:w - 32] + ((int.from_bytes(good[w - 32:], "big") + 1) % self.M.P).to_bytes(32, "big")
        for k, v in out.items():
            want = {"infinity": ST_OK, "off subgroup": ST_NOT_IN_SUBGROUP}.get(k, ST_BAD_POINT)
            assert self.status(g, v, unc) == want, (self.name, g, k)
        return out


@functools.lru_cache(maxsize=None)
def suite(name):
    return Suite(name)


def _be_scalars(ks):
    return _arr([k.to_bytes(32, "big") for k in ks], 32)


def _reject_kinds(S):
    return ["flag rule", "off subgroup", "infinity"] if S.bls else ["off curve", "infinity"]


def _make_group_mul(name, g, flags, same_base=False, bad_base=False):
    def make(n, world):
        S = suite(name)
        unc, unc_out, trusted = bool(flags & F_UNC), bool(flags & F_UNC_OUT), bool(flags & F_TRUSTED0)
        ks = S.line(g, b"mul/k", n)[0]
        pts = S.line(g, b"mul/P", n)[1]
        wi, wo = S.width(g, unc), S.width(g, unc_out)
        status, exp, plants = np.zeros(n, dtype=np.uint8), {}, {}
        if same_base:
            base_pt = pts[5 % n]
            base = S.rejects(g, unc)["flag rule" if S.bls else "off curve"] if bad_base else S.enc(g, base_pt, unc)
            P = _arr([base], wi)
            if bad_base:
                status[:] = ST_BAD_POINT
            for i in _check_rows(n, world):
                exp[i] = bytes(wo) if bad_base else S.enc(g, S.mul(g, ks[i], base_pt), unc_out)
        else:
            P = _arr([S.enc(g, p, unc) for p in pts], wi)
            # (a trusted operand is vouched for: nothing the decoder would reject may stand in its place)
            planted = {} if trusted else _plant(_reject_kinds(S), n, world)
            for row, kind in planted.items():
                P[row] = np.frombuffer(S.rejects(g, unc)[kind], dtype=np.uint8)
                status[row] = S.status(g, bytes(P[row]), unc)
                plants[row] = Plant(kind, int(status[row]), None)
            for i in _check_rows(n, world, planted):
                if status[i]:
                    exp[i] = bytes(wo)
                else:
                    exp[i] = S.enc(g, None if planted.get(i) == "infinity" else S.mul(g, ks[i], pts[i]), unc_out)
        entry = "kyb_%s_g%d_mul%s" % (name, g, "_same_base" if same_base else "")
        return Case(entry, [n, _be_scalars(ks), P, Out("out", (n, wo)), Out("status", (n,)), flags], n, world, status=status,
                    expect={"out": exp}, planted=plants)
    return make


def _make_pair(name, flags):
    def make(n, world):
        S = suite(name)
        unc = bool(flags & F_UNC)
        ps, qs = S.line(1, b"pair/P", n)[1], S.line(2, b"pair/Q", n)[1]
        g1 = _arr([S.enc(1, p, unc) for p in ps], S.width(1, unc))
        g2 = _arr([S.enc(2, q, unc) for q in qs], S.width(2, unc))
        kinds = [k for k in _reject_kinds(S) if k != "infinity"]
        planted = _plant([(1, kinds[0]), (2, kinds[-1]), (2, kinds[0])], n, world)
        status, exp, plants = np.zeros(n, dtype=np.uint8), {}, {}
        for row, (g, kind) in planted.items():
            (g1 if g == 1 else g2)[row] = np.frombuffer(S.rejects(g, unc)[kind], dtype=np.uint8)
            status[row] = S.status(g, S.rejects(g, unc)[kind], unc)
            plants[row] = Plant("G%d %s" % (g, kind), int(status[row]), None)
        for i in _check_rows(n, world, planted):
            exp[i] = bytes(S.gt_size) if status[i] else S.pair(ps[i], qs[i])
        return Case("kyb_%s_pair" % name, [n, g1, g2, Out("gt", (n, S.gt_size)), Out("status", (n,)), flags], n, world, status=status,
                    expect={"gt": exp}, planted=plants)
    return make


def _make_pair_check(name, flags):
    """e(p G1, q r G2) == e(p q G1, r G2): four operands that all change from row to row, equal by construction
    (tests/test_shard_sites.py puts the oracle's own pairings to a few rows of these lines)"""
    def make(n, world):
        S = suite(name)
        unc = bool(flags & F_UNC)
        a1 = S.line(1, b"check/p", n)[1]
        a2 = S.product_line(2, b"check/q", b"check/r", n)
        b1 = S.product_line(1, b"check/p", b"check/q", n)
        b2 = S.line(2, b"check/r", n)[1]
        cols = [_arr([S.enc(g, p, unc) for p in pts], S.width(g, unc)) for g, pts in ((1, a1), (2, a2), (1, b1), (2, b2))]
        bad = [k for k in _reject_kinds(S) if k != "infinity"]
        planted = _plant(["forged", "p1 " + bad[0], "inv2 " + bad[-1], "forged"], n, world)
        ok, status, plants = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), {}
        for row, kind in planted.items():
            ok[row] = 0
            if kind == "forged":  # another valid point, nobody's product
                cols[2][row] = np.frombuffer(S.enc(1, S.line(1, b"check/forged", n)[1][row], unc), dtype=np.uint8)
            else:
                slot, g = (0, 1) if kind.startswith("p1") else (3, 2)
                cols[slot][row] = np.frombuffer(S.rejects(g, unc)[kind.split(" ", 1)[1]], dtype=np.uint8)
                status[row] = S.status(g, bytes(cols[slot][row]), unc)
            plants[row] = Plant(kind, int(status[row]), 0)
        return Case("kyb_%s_pair_check" % name, [n] + cols + [Out("ok", (n,)), Out("status", (n,)), flags], n, world, status=status,
                    ok=ok, planted=plants)
    return make


def _make_suite_msm(name):
    def make(n, world):
        S = suite(name)
        ks, pts = S.line(1, b"msm/P", n)
        small = [S.scalar(b"msm/s%d" % i) % 2**32 for i in range(n)]  # 32-bit scalars: the sum's discrete logarithm is at hand
        total = S.G[1].mul(sum(s * k for s, k in zip(small, ks)) % S.order, S.G[1].gen)
        P = _arr([S.enc(1, p, False) for p in pts], S.width(1, False))
        w = S.width(1, False)
        return Case("kyb_%s_g1_msm" % name, [n, _be_scalars(small), P, Out("out", (w,)), Out("status", (n,)), 0], n, world,
                    status=np.zeros(n, dtype=np.uint8), whole={"out": S.enc(1, total, False)})
    return make


_PA = "pairing_abi.cuh"
_BLS_MUL_FLAGS = (("", 0), ("/uncompressed", F_UNC), ("/uncompressed out", F_UNC_OUT), ("/uncompressed trusted both", F_UNC | F_TRUSTED0 | F_UNC_OUT))
for _s in ("bls12381", "bn256", "bn254"):
    for _g in (1, 2):
        for _name, _f in _BLS_MUL_FLAGS if _s == "bls12381" else (("", 0),) + ((("/uncompressed", F_UNC),) if _g == 1 else ()):
            _row("%s/g%d_mul%s" % (_s, _g, _name), (_PA, "mul_host"), _make_group_mul(_s, _g, _f), cheap=_s == "bn256" and _g == 1 and not _f)
            _row("%s/g%d_commit%s" % (_s, _g, _name), (_PA, "mul_host"), _make_group_mul(_s, _g, _f, same_base=True))
        _row("%s/g%d_commit/rejected base" % (_s, _g), (_PA, "mul_host"), _make_group_mul(_s, _g, 0, same_base=True, bad_base=True))
    for _name, _f in (("", 0), ("/uncompressed", F_UNC)):
        _row("%s/pair%s" % (_s, _name), (_PA, "pair_host"), _make_pair(_s, _f))
        _row("%s/pair_check%s" % (_s, _name), (_PA, "pair_check_host"), _make_pair_check(_s, _f))
    _row("%s/g1_msm" % _s, ("msm.cuh", "run_host"), _make_suite_msm(_s))


# ============================================================================================= BLS verifications
def _bls_sign_rows(scheme_g, msgs, rows, xs, dst):
    """{row: x_row * H(m_row)} as points of the signature group"""
    S = suite("bls12381")
    h = {}
    out = {}
    for i in rows:
        m = bytes(msgs[i])
        if m not in h:
            h[m] = (OB.hash_to_g1 if scheme_g == 1 else OB.hash_to_g2)(m, dst)
        out[i] = S.mul(scheme_g, xs[i], h[m])
    return out


def _make_bls_verify(entry, msg_len, flags, key="a"):
    """entry: verify_g1 / verify_g2 (a message each), verify_g1_same_msg, verify_g1_same_key.  key (same_key): "a", "b" or
    "bad" (one that fails UnmarshalBinary)"""
    sig_g = 2 if entry == "verify_g2" else 1
    key_g = 3 - sig_g
    dst = IO.DOMAIN_G1 if sig_g == 1 else IO.DOMAIN_G2
    one_msg, one_key = entry == "verify_g1_same_msg", entry == "verify_g1_same_key"

    def make(n, world):
        S = suite("bls12381")
        unc = bool(flags & F_UNC)
        xs, Xs = S.line(key_g, b"verify/x/" + key.encode(), n)
        if one_key:
            xs, Xs = [xs[0]] * n, [Xs[0]]
        if one_msg:
            msg = bytes(_shake(b"verify/one msg", msg_len))
            msgs = [msg] * n
            marr = np.frombuffer(msg, dtype=np.uint8).copy() if msg_len else None
        else:
            marr = _shake(b"verify/m%d" % msg_len, n * msg_len).reshape(n, msg_len) if msg_len else None
            msgs = [bytes(marr[i]) if msg_len else b"" for i in range(n)]
        ws, wk = S.width(sig_g, unc), S.width(key_g, unc)
        keys = _arr([S.enc(key_g, X, unc) for X in Xs], wk)
        if key == "bad":
            keys[0] = np.frombuffer(S.rejects(key_g, unc)["flag rule"], dtype=np.uint8)
        rej = S.rejects(sig_g, unc)
        kinds = {"forged": ST_OK, "signature off subgroup": ST_NOT_IN_SUBGROUP, "signature flag rule": ST_BAD_POINT}
        if not one_key:
            kinds["undecodable key"] = ST_BAD_POINT
        planted = _plant(list(kinds), n, world)
        rows = _check_rows(n, world, planted)
        signed = _bls_sign_rows(sig_g, msgs, rows, xs, dst)
        other = S.line(sig_g, b"verify/forged", n)[1]  # valid points that are nobody's signature
        sigs = _arr([S.enc(sig_g, signed.get(i, other[i]), unc) for i in range(n)], ws)
        ok, status = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for row, kind in planted.items():
            ok[row], status[row] = 0, kinds[kind]
            if kind == "forged":
                sigs[row] = np.frombuffer(S.enc(sig_g, other[row], unc), dtype=np.uint8)
            elif kind == "undecodable key":
                keys[row] = np.frombuffer(S.rejects(key_g, unc)["flag rule"], dtype=np.uint8)
            else:
                sigs[row] = np.frombuffer(rej[kind.split(" ", 1)[1]], dtype=np.uint8)
                assert S.status(sig_g, bytes(sigs[row]), unc) == kinds[kind]
        if key == "bad":  # the key's verdict comes first, for every element of every shard
            ok[:], status[:] = 0, ST_BAD_POINT
        filler = [i for i in range(n) if i not in signed]
        xs_be = _be_scalars(xs)

        def fill(bls):
            """the engine signs the rows the oracle did not: x_i * H(m_i), device set cleared by the caller"""
            if not filler:
                return
            hash_ = bls.batch_hash_g1 if sig_g == 1 else bls.batch_hash_g2
            mul = bls.g1_batch_mul if sig_g == 1 else bls.g2_batch_mul
            m = np.zeros((len(filler), msg_len), dtype=np.uint8)
            for k, i in enumerate(filler):
                m[k] = np.frombuffer(msgs[i], dtype=np.uint8)
            hm, st = hash_(m, dst)
            assert not np.asarray(st).any()
            out, st = mul(xs_be[filler], np.asarray(hm), F_UNC_OUT if unc else 0)
            assert not np.asarray(st).any()
            sigs[filler] = np.asarray(out)

        args = [n, keys, marr, msg_len, Dst(dst), len(dst), sigs, Out("ok", (n,)), Out("status", (n,)), flags]
        plants = {} if key == "bad" else {r: Plant(k, kinds[k], 0) for r, k in planted.items()}
        return Case("kyb_bls12381_" + entry, args, n, world, status=status, ok=ok, planted=plants, fill=fill)
    return make


_H2C = "bls12381_h2c.hip"
for _e in ("verify_g1", "verify_g2", "verify_g1_same_msg"):
    for _ln in (0, 32, 33):
        for _name, _f in (("", 0), ("/uncompressed", F_UNC)):
            _row("bls12381/%s/len %d%s" % (_e, _ln, _name), (_H2C, "kyb_bls12381_" + _e), _make_bls_verify(_e, _ln, _f),
                 cheap=_e == "verify_g1_same_msg" and _ln == 32 and not _f)
for _k in ("a", "b", "bad"):
    _row("bls12381/verify_g1_same_key/key " + _k, (_H2C, "kyb_bls12381_verify_g1_same_key"), _make_bls_verify("verify_g1_same_key", 32, 0, _k))
_row("bls12381/verify_g1_same_key/key a/uncompressed", (_H2C, "kyb_bls12381_verify_g1_same_key"),
     _make_bls_verify("verify_g1_same_key", 33, F_UNC, "a"))


# ================================================================================================================ IBE
IBE_ID, IBE_LEN, IBE_SECRET = b"shard cases round", 16, 0x1B3C5D7E9F


def _make_ibe_encrypt(n, world):
    """EncryptCCAonG2 (drand quicknet): U and W at every check row, V (a GT exponentiation each) at the planted places"""
    master, _ = IO.keys(True, IBE_SECRET, IBE_ID)
    sig, msg = _shake(b"ibe/sigma", n * IBE_LEN).reshape(n, IBE_LEN), _shake(b"ibe/msg", n * IBE_LEN).reshape(n, IBE_LEN)
    g = IO.gid(True, master, IBE_ID)
    exp = {"u": {}, "v": {}, "w": {}}
    for i in _check_rows(n, world):
        s, m = bytes(sig[i]), bytes(msg[i])
        exp["u"][i] = OB.g2_compress(OB.g2_mul(IO.h3(s, m), OB.G2_GEN))
        exp["w"][i] = IO._xor(m, IO.h4(s, IBE_LEN))
    for i in plant_rows(n, world)[:3]:
        exp["v"][i] = IO.encrypt(True, master, IBE_ID, bytes(msg[i]), bytes(sig[i]), g=g)[1]
    args = [n, _arr([master], 96), np.frombuffer(IBE_ID, dtype=np.uint8).copy(), len(IBE_ID), Dst(IO.DOMAIN_G1), len(IO.DOMAIN_G1), sig, msg,
            IBE_LEN, Out("u", (n, 96)), Out("v", (n, IBE_LEN)), Out("w", (n, IBE_LEN)), Out("status", (n,)), 0]
    return Case("kyb_bls12381_ibe_encrypt_g2", args, n, world, status=np.zeros(n, dtype=np.uint8), expect=exp)


def _make_ibe_decrypt(n, world):
    """DecryptCCAonG2 under one private key: the oracle's ciphertexts at the planted places (one with V altered: the rP
    check fails), the engine's everywhere else; every message is the table's own plaintext"""
    master, private = IO.keys(True, IBE_SECRET, IBE_ID)
    sig, msg = _shake(b"ibe/sigma", n * IBE_LEN).reshape(n, IBE_LEN), _shake(b"ibe/msg", n * IBE_LEN).reshape(n, IBE_LEN)
    g = IO.gid(True, master, IBE_ID)
    U, Vv, W = np.zeros((n, 96), dtype=np.uint8), np.zeros((n, IBE_LEN), dtype=np.uint8), np.zeros((n, IBE_LEN), dtype=np.uint8)
    places = plant_rows(n, world)[:3]
    for i in places:
        u, v, w = IO.encrypt(True, master, IBE_ID, bytes(msg[i]), bytes(sig[i]), g=g)
        U[i], Vv[i], W[i] = (np.frombuffer(x, dtype=np.uint8) for x in (u, v, w))
    status = np.zeros(n, dtype=np.uint8)
    Vv[places[0], 0] ^= 1
    status[places[0]] = ST_IBE_CHECK
    exp = {i: bytes(IBE_LEN) if status[i] else bytes(msg[i]) for i in _check_rows(n, world, places)}
    filler = [i for i in range(n) if i not in places]

    def fill(bls):
        if filler:
            u, v, w, st = bls.batch_ibe_encrypt_g2(master, IBE_ID, msg[filler], sigmas=sig[filler], dst=IO.DOMAIN_G1)
            assert not np.asarray(st).any()
            U[filler], Vv[filler], W[filler] = np.asarray(u), np.asarray(v), np.asarray(w)

    args = [n, _arr([private], 48), 0, U, Vv, W, IBE_LEN, Out("msgs", (n, IBE_LEN)), Out("status", (n,)), 0]
    return Case("kyb_bls12381_ibe_decrypt_g2", args, n, world, status=status, expect={"msgs": exp},
                planted={places[0]: Plant("V altered", ST_IBE_CHECK, None)}, fill=fill)


_row("bls12381/ibe_encrypt_g2", ("bls12381_ibe.hip", "encrypt_host"), _make_ibe_encrypt, cheap=True)
_row("bls12381/ibe_decrypt_g2", ("bls12381_ibe.hip", "decrypt_host"), _make_ibe_decrypt)


@functools.lru_cache(maxsize=256)
def build(name, n, world):
    return ROWS[name].make(n, world)
