"""tests/_add_cases.py checked on the CPU: every group's table builds from the oracles alone, carries every required
label, agrees with itself (the expectation of (a, b) is that of (b, a) wherever both operands decode; every expected
encoding decodes, from scratch, to the oracle's sum of the operands decoded from scratch), and builds quickly enough to
be shared by the host-harness tests and the GPU tests."""
import time
from collections import Counter

import pytest

from tests import _add_cases as A

BUILD_SECONDS = 120  # all seven tables on one core; they take a few seconds (the build time is printed below)


def test_tables_build_within_budget():
    A.table.cache_clear()
    for name in A.GROUPS:
        A.group(name).memo.clear()
    t0 = time.time()
    sizes = {name: len(A.table(name).labels) for name in A.GROUPS}
    dt = time.time() - t0
    print("add case tables: %s rows in %.1f s" % (sizes, dt))
    assert dt < BUILD_SECONDS, dt
    assert all(n >= A.FILLER + 50 for n in sizes.values())


@pytest.mark.parametrize("name", A.GROUPS)
def test_label_census(name):
    t = A.table(name)
    census = Counter(t.labels)
    for label in A.required_labels(name):
        assert census[label] >= 1, label
    assert census["generic"] == A.FILLER
    rejected = [l for l, s in zip(t.labels, t.status) if s]
    assert rejected and all(l.startswith(("reject", "coord-ge-p")) for l in rejected)
    if name.startswith("bls"):
        # status 2 alone, status 2 before 1 and 1 before 2: which operand's status wins is visible
        both = [(int(A.group(name).decode(a)[0]), int(A.group(name).decode(b)[0]), int(s))
                for a, b, s, l in zip(t.a, t.b, t.status, t.labels) if l.startswith("reject-both")]
        assert {(1, 2, 1), (2, 1, 2)} <= set(both)
    if name in ("bn256-g1", "bn256-g2"):
        assert not any(s for l, s in zip(t.labels, t.status) if l.startswith("coord-ge-p"))   # reduced, as point.go does
    if name in ("bn254-g1", "bn254-g2"):
        assert all(s == 1 for l, s in zip(t.labels, t.status) if l.startswith("coord-ge-p"))  # rejected, as gfp.go does


@pytest.mark.parametrize("name", A.GROUPS)
def test_tables_agree_with_themselves(name):
    t, G = A.table(name), A.group(name)
    for i, label in enumerate(t.labels):
        a, b, out = bytes(t.a[i]), bytes(t.b[i]), bytes(t.out[i])
        sa, pa = G._dec(a) if label != "generic" else G.decode(a)  # (the labelled operands from scratch, not from the memo)
        sb, pb = G._dec(b) if label != "generic" else G.decode(b)
        assert int(t.status[i]) == (sa if sa else sb), (i, label)
        if t.status[i]:
            assert out == bytes(G.width), (i, label)
            continue
        so, po = G._dec(out) if label != "generic" else G.decode(out)
        assert so == 0 and po == G.add(pa, pb) == G.add(pb, pa), (i, label)
        assert G._enc(po) == out, (i, label)  # results are canonical encodings
        assert G.expect(b, a) == (0, out), (i, label)


def test_chain_and_tiling():
    for name in ("ed25519", "bn256-g1"):
        G = A.group(name)
        a, b, out = A.chain(name, 130)
        for i in (0, 1, 64, 127, 128, 129):
            assert G.expect(bytes(a[i]), bytes(b[i])) == (0, bytes(out[i]))
        assert bytes(a[127]) == bytes(b[127])  # the tail: P + P, P + (-P), inf + P
        t = A.table(name)
        tt = A.tiled(t, 3)
        assert len(tt.labels) == 3 * len(t.labels) and Counter(tt.labels) == Counter(t.labels * 3)
        assert sorted(set(t.labels)) == sorted(t.labels[i] for i in A.one_per_label(t))
