"""sign/anon without a GPU: kyber_amd/csrc/ed25519_ring.cuh compiled for the CPU (tests/ring_harness.cpp) against the
sign/anon oracle on the table of tests/_ring_cases.py, and the challenge at the boundaries of the key / data split and of
the 128-byte block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _anon_oracle as A
from tests import _ring_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build", "libringharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "ring_harness.cpp")])
    return C.CDLL(out)


def _aligned(b: bytes) -> np.ndarray:
    """a 16-byte aligned copy (the lane program loads 32-byte items as two 16-byte words)"""
    raw = np.zeros(len(b) + 32, dtype=np.uint8)
    o = (-raw.ctypes.data) % 16
    a = raw[o:o + max(len(b), 1)]
    a[:len(b)] = np.frombuffer(b, dtype=np.uint8)
    return a


def run_chain(h, rows, scope, shared, vartime, start=None, steps=None, link_base=None):
    n, ring = len(rows), rows[0].ring
    keys = _aligned(b"".join(rows[0].keys) if shared else b"".join(b"".join(r.keys) for r in rows))
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(r.message) for r in rows], out=off[1:])
    msgs = _aligned(b"".join(r.message for r in rows))
    sigs = _aligned(b"".join(r.sig for r in rows))
    base = _aligned(link_base or A.link_base(scope)) if scope is not None else None
    sc = np.frombuffer(scope or b"\0", dtype=np.uint8) if scope is not None else None
    st = np.ascontiguousarray(np.asarray(start, dtype=np.uint32)) if start is not None else None
    cz, co = _aligned(bytes(32 * n)), _aligned(bytes(32 * n))
    ok, status = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    h.rng_chain(C.c_size_t(n), C.c_size_t(ring), p(keys), C.c_size_t(0 if shared else 32 * ring), p(msgs), p(off), p(sc),
                C.c_size_t(len(scope) if scope is not None else 0), p(base), p(sigs), C.c_size_t(len(rows[0].sig)), p(st),
                C.c_size_t(ring if steps is None else steps), C.c_int(int(vartime)), p(cz), p(co), p(ok), p(status))
    return [(bytes(cz[32 * i:32 * i + 32]), bytes(co[32 * i:32 * i + 32]), int(ok[i]), int(status[i])) for i in range(n)]


def test_table_holds_every_label_at_every_ring_size():
    for (ring, linkable), idx in RC.groups().items():
        have = {RC.rows()[i].label for i in idx}
        want = set(RC.LABELS) - (set() if linkable else set(RC.LINKABLE_ONLY)) - ({"identity intermediate"} if ring == 1 else set())
        assert have == want, (ring, linkable)
    exp = RC.expected(False)
    labels = [r.label for r in RC.rows()]
    assert all(exp[i][2] == 1 for i, l in enumerate(labels) if l in ("valid", "s + l", "identity intermediate"))
    assert all(exp[i][3] == 1 for i, l in enumerate(labels) if l in ("tag undecodable",))
    assert any(exp[i][3] == 1 for i, l in enumerate(labels) if l == "key undecodable")
    assert all(exp[i][2] == 0 for i, l in enumerate(labels) if l in ("c0 altered", "message altered", "c0 + l", "c0 + 8 l", "c0 + 15 l", "c0 = 0", "scope altered"))


@pytest.mark.parametrize("vartime", [False, True])
def test_lane_program_agrees_with_the_oracle_on_every_row(harness, vartime):
    exp = RC.expected(vartime)
    for (ring, linkable), idx in RC.groups().items():
        rows = [RC.rows()[i] for i in idx]
        got = run_chain(harness, rows, RC.SCOPE if linkable else None, False, vartime)
        for i, g in zip(idx, got):
            assert g == exp[i], (ring, linkable, RC.rows()[i].label, vartime)
    shared_labels = set()
    for (ring, linkable, _), idx in RC.shared_groups().items():  # every row again with its ring shared by the call
        idx = idx if len(idx) > 1 else idx * 2
        shared_labels |= {RC.rows()[i].label for i in idx}
        got = run_chain(harness, [RC.rows()[i] for i in idx], RC.SCOPE if linkable else None, True, vartime)
        for i, g in zip(idx, got):
            assert g == exp[i], (ring, linkable, RC.rows()[i].label, "shared ring")
    assert shared_labels == set(RC.LABELS)


def test_undecodable_link_base_is_a_bad_point_for_every_signature(harness):
    rows = [r for r in RC.rows() if r.ring == 3 and r.linkable and r.label in ("valid", "s altered")]
    for shared in (False, True):
        got = run_chain(harness, rows, RC.SCOPE, shared, False, link_base=RC.UNDECODABLE)
        assert got == [(bytes(32), bytes(32), 0, 1)] * len(rows)


def test_rotated_chain_agrees_with_the_oracle(harness):
    for linkable in (False, True):
        rows = [r for r in RC.rows() if r.ring == 3 and r.linkable == linkable and r.label in ("valid", "s altered", "s + 8 l")]
        scope = RC.SCOPE if linkable else None
        for start, steps in ((1, 2), (2, 2), (2, 1), (0, 2), (1, 5)):
            got = run_chain(harness, rows, scope, False, False, [start] * len(rows), steps)
            want = [A.chain(r.message, list(r.keys), scope, r.sig, start, steps) for r in rows]
            assert got == want, (linkable, start, steps)


MSG_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193)
SCOPE_LENS = (None, 0, 16, 31, 32, 33, 95, 96, 97)


def challenge_cases():
    """(msg, scope, tag, PG, PH) at every boundary of the key / data split and of the 128-byte block; tags include an
    undecodable one and non-canonical ones (y >= p, and "-0")"""
    import hashlib

    from oracle import ed25519 as O

    pt = lambda s: O.mul_base(hashlib.sha256(s).digest())
    odd_tags = [RC.UNDECODABLE, (O.P + 1).to_bytes(32, "little"), bytes([1]) + bytes(30) + bytes([0x80]),
                (2**255 - 1).to_bytes(32, "little")]
    out = []
    for ml in MSG_LENS:
        msg = bytes((7 * i + ml) & 255 for i in range(ml))
        for k, sl in enumerate(SCOPE_LENS):
            scope = None if sl is None else bytes((3 * i + sl) & 255 for i in range(sl))
            tag = None if sl is None else (odd_tags[(ml + k) % 4] if (ml + k) % 3 == 0 else pt(b"tag%d" % ml))
            out.append((msg, scope, tag, pt(b"pg%d.%d" % (ml, k)), None if sl is None else pt(b"ph%d.%d" % (ml, k))))
    return out


def test_challenge_at_every_block_and_key_boundary(harness):
    by_scope = {}
    for c in challenge_cases():
        by_scope.setdefault(c[1], []).append(c)
    seen_odd = 0
    for scope, cs in by_scope.items():
        n = len(cs)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(c[0]) for c in cs], out=off[1:])
        msgs = _aligned(b"".join(c[0] for c in cs))
        pg = _aligned(b"".join(c[3] for c in cs))
        tags = _aligned(b"".join(c[2] for c in cs)) if scope is not None else None
        ph = _aligned(b"".join(c[4] for c in cs)) if scope is not None else None
        sc = np.frombuffer(scope or b"\0", dtype=np.uint8) if scope is not None else None
        out, st = _aligned(bytes(32 * n)), np.zeros(n, dtype=np.uint8)
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        harness.rng_challenge(C.c_size_t(n), p(msgs), p(off), p(sc), C.c_size_t(len(scope or b"")), p(tags), p(pg), p(ph), p(out), p(st))
        for i, c in enumerate(cs):
            want = A.h1(c[0], scope, A.canon_bytes(c[2]) if scope is not None else None, c[3], c[4])
            assert bytes(out[32 * i:32 * i + 32]) == want and st[i] == 0, (len(c[0]), None if scope is None else len(scope))
            seen_odd += scope is not None and A.canon_bytes(c[2]) != c[2] or (scope is not None and c[2] == RC.UNDECODABLE)
    assert seen_odd >= 8
