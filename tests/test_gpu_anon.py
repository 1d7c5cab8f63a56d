"""sign/anon on the GPU: the golden signatures of the reference, the challenge at every block boundary, the ring chain
on the table of tests/_ring_cases.py, launch and piece edges, and the sharded host call -- all against the sign/anon
oracle (tests/_anon_oracle.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _anon_oracle as A
from tests import _ring_cases as RC
from tests.test_ring_host import challenge_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "anon.json")))


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


@pytest.fixture(scope="module")
def anon():
    from kyber_amd.sign import anon

    return anon


def _rows(x):
    return [bytes(r) for r in np.asarray(x)]


@pytest.mark.parametrize("name", A.GOLDEN_EXAMPLES)
def test_golden_signatures_verify_and_are_reproduced(anon, name):
    keys, scope, mines, xs, rand = A.golden_keys(name)
    sigs = [bytes.fromhex(h) for h in GOLDEN["examples"][name]["signatures"]]
    n = len(sigs)
    want_tags = [bytes.fromhex(t) for t in GOLDEN["examples"][name]["tags"]] or [b""] * n
    for sig, tag in zip(sigs, want_tags):
        assert anon.Verify(A.GOLDEN_MESSAGE, keys, scope, sig) == tag
        with pytest.raises(anon.AnonError):
            anon.Verify(A.GOLDEN_BAD_MESSAGE, keys, scope, sig)
        with pytest.raises(anon.AnonError):
            anon.Verify(A.GOLDEN_MESSAGE, keys, scope, sig[:-1])
    tags, ok, st = anon.VerifyBatch([A.GOLDEN_MESSAGE] * n + [A.GOLDEN_BAD_MESSAGE] * n, keys, scope, sigs + sigs)
    assert list(ok) == [1] * n + [0] * n and not st.any() and tags == want_tags + [None] * n
    assert anon.SignBatch([A.GOLDEN_MESSAGE] * n, keys, scope, mines, xs, rand) == sigs
    if scope is not None:
        assert anon.link_base(scope) == A.link_base(scope)


def test_challenge_at_every_block_and_key_boundary(ed):
    by_scope = {}
    for c in challenge_cases():
        by_scope.setdefault(c[1], []).append(c)
    assert len(by_scope) == 9
    for scope, cs in by_scope.items():
        linkable = scope is not None
        c, st = ed.batch_ring_challenge([x[0] for x in cs], scope, b"".join(x[2] for x in cs) if linkable else None,
                                        b"".join(x[3] for x in cs), b"".join(x[4] for x in cs) if linkable else None)
        want = [A.h1(x[0], scope, A.canon_bytes(x[2]) if linkable else None, x[3], x[4]) for x in cs]
        assert _rows(c) == want and not st.any(), None if scope is None else len(scope)


def _chain(ed, rows, scope, shared, vartime, link_base=None, **kw):
    keys = b"".join(rows[0].keys) if shared else b"".join(b"".join(r.keys) for r in rows)
    keys = np.frombuffer(keys, dtype=np.uint8).reshape(1 if shared else len(rows), -1)
    base = (link_base or A.link_base(scope)) if scope is not None else None
    cz, co, ok, st = ed.batch_ring_chain(keys, [r.message for r in rows], scope, base, b"".join(r.sig for r in rows),
                                         rows[0].ring, vartime=vartime, **kw)
    return list(zip(_rows(cz), _rows(co), [int(v) for v in ok], [int(v) for v in st]))


@pytest.mark.parametrize("vartime", [False, True])
def test_chain_agrees_with_the_oracle_on_every_row(ed, vartime):
    exp = RC.expected(vartime)
    labels = set()
    for (ring, linkable), idx in RC.groups().items():
        rows = [RC.rows()[i] for i in idx]
        labels |= {r.label for r in rows}
        scope = RC.SCOPE if linkable else None
        got = _chain(ed, rows, scope, False, vartime)
        for i, g in zip(idx, got):
            assert g == exp[i], (ring, linkable, RC.rows()[i].label)
    assert labels == set(RC.LABELS)
    shared_labels = set()
    for (ring, linkable, _), idx in RC.shared_groups().items():  # every row again with its ring shared by the call:
        for reps in (2, 1):                                       # the tables kernel's tables and its bad-key flags
            rows = [RC.rows()[i] for i in idx] * reps
            shared_labels |= {r.label for r in rows}
            got = _chain(ed, rows, RC.SCOPE if linkable else None, True, vartime)
            for i, g in zip(idx * reps, got):
                assert g == exp[i], (ring, linkable, RC.rows()[i].label, "shared ring", len(rows))
    assert shared_labels == set(RC.LABELS)
    assert {r.ring for r in RC.rows()} == {1, 2, 3, 5}


def test_undecodable_link_base_is_a_bad_point_for_every_signature(ed):
    rows = [r for r in RC.rows() if r.ring == 3 and r.linkable and r.label in ("valid", "s altered")]
    for shared in (False, True):
        assert _chain(ed, rows, RC.SCOPE, shared, False, link_base=RC.UNDECODABLE) == [(bytes(32), bytes(32), 0, 1)] * len(rows)


def test_embed_and_data_follow_the_reference(ed):
    """Point.Embed / Data (point.go:125-193) against their restatement on the oracle, on the same stream"""
    from kyber_amd.util import blake2xb
    from oracle import ed25519 as O

    def oracle_embed(data, rand):
        dl = min(29, len(data))
        while True:
            b = bytearray(rand.XORKeyStream(bytes(32)))
            b[0] = dl
            b[1:1 + dl] = data[:dl]
            pt = O.decode(bytes(b))
            if pt is not None and O.mul_int(O.L, pt) == O.IDENTITY:
                return O.encode(pt)

    assert ed.Point().EmbedLen() == 29
    # Embed(nil, rand) under blake2xb.New(nil): the first key of the reference's ExampleSign_anonSet, whose printed
    # signature pins it (tests/test_anon_oracle.py)
    assert ed.Point().Embed(None, blake2xb.New(b"")).MarshalBinary() == A.golden_keys("ExampleSign_anonSet")[0][0]
    for data in (b"", b"x", b"twenty-nine bytes of data, yes", bytes(range(29)), bytes(range(40))):
        p = ed.Point().Embed(data, blake2xb.New(b"embed"))
        enc = p.MarshalBinary()
        assert enc == oracle_embed(data, blake2xb.New(b"embed"))
        assert enc[0] == min(29, len(data)) and p.Data() == data[:29]
    with pytest.raises(ValueError):
        ed.Point(bytes([30]) + bytes(31)).Data()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_launch_edges_host_and_device_entries_agree(ed, n):
    import torch

    for linkable in (False, True):
        pool = [r for r in RC.rows() if r.ring == 3 and r.linkable == linkable and r.keys == RC.base_keys(3, linkable)[0]]
        rows = [pool[i % len(pool)] for i in range(n)]
        scope = RC.SCOPE if linkable else None
        start = [i % 3 for i in range(n)]
        steps = 2
        uniq = {}
        exp = []
        for r, s in zip(rows, start):
            k = (r.label, s)
            if k not in uniq:
                uniq[k] = A.chain(r.message, list(r.keys), scope, r.sig, s, steps)
            exp.append(uniq[k])
        host = _chain(ed, rows, scope, True, False, start=start, steps=steps)
        assert host == exp
        dev = "cuda"
        t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r.message) for r in rows], out=off[1:])
        keys = b"".join(rows[0].keys)
        out = ed.batch_ring_chain(t(keys).view(1, -1), (t(b"".join(r.message for r in rows)), torch.from_numpy(off).to(dev)),
                                  t(scope) if linkable else None, t(A.link_base(scope)) if linkable else None,
                                  t(b"".join(r.sig for r in rows)).view(n, -1), 3,
                                  start=torch.tensor(start, dtype=torch.int32, device=dev), steps=steps)
        torch.cuda.synchronize()
        cz, co, ok, st = [x.cpu().numpy() for x in out]
        assert list(zip(_rows(cz), _rows(co), [int(v) for v in ok], [int(v) for v in st])) == exp
        if n == 1:
            continue
        full_host = _chain(ed, rows, scope, True, False)
        c_dev, s_dev = ed.batch_ring_challenge((t(b"".join(r.message for r in rows)), torch.from_numpy(off).to(dev)),
                                               t(scope) if linkable else None,
                                               t(b"".join(r.sig[-32:] for r in rows)).view(n, 32) if linkable else None,
                                               t(b"".join(g[1] if g[3] == 0 else bytes(32) for g in full_host)).view(n, 32),
                                               t(b"".join(g[0] for g in full_host)).view(n, 32) if linkable else None)
        c_host, s_host = ed.batch_ring_challenge([r.message for r in rows], scope,
                                                 b"".join(r.sig[-32:] for r in rows) if linkable else None,
                                                 b"".join(g[1] if g[3] == 0 else bytes(32) for g in full_host),
                                                 b"".join(g[0] for g in full_host) if linkable else None)
        torch.cuda.synchronize()
        assert _rows(c_dev.cpu().numpy()) == _rows(c_host) and list(s_dev.cpu().numpy()) == list(s_host)


def test_piece_edge_sign_batch_then_verify_batch(anon):
    from kyber_amd.util import blake2xb

    n = (1 << 18) + 5
    r = blake2xb.New(b"piece edge keys")
    x = [A.scalar_pick(r), A.scalar_pick(r)]
    from oracle import ed25519 as O

    keys = [O.mul_base(x[0]), O.mul_base(x[1])]
    scope = b"piece edge"
    msgs = [b"ballot %d" % i for i in range(n)]
    mine = [i & 1 for i in range(n)]

    class Fast:  # a cheap deterministic stream: the draws only have to be scalars
        def __init__(self):
            self.rng = np.random.default_rng(7)

        def Read(self, k):
            return self.rng.bytes(k)

    sigs = anon.SignBatch(msgs, keys, scope, mine, [x[m] for m in mine], Fast())
    bad = [0, 1, 63, 64, 1000, 131071, 131072, (1 << 18) - 2, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 18) + 2, (1 << 18) + 3,
           (1 << 18) + 4, 200000, 77]
    assert len(set(bad)) == 16
    for k, i in enumerate(bad):
        slot = k % 4  # c0, s_0, s_1 or the tag
        b = bytearray(sigs[i])
        b[32 * slot + (k % 31)] ^= 1 << (k % 7)
        sigs[i] = bytes(b)
    tags, ok, st = anon.VerifyBatch(msgs, keys, scope, sigs)
    rejected = [i for i in range(n) if not ok[i]]
    assert sorted(rejected) == sorted(bad)
    rng = np.random.default_rng(11)
    sample = sorted(set(bad) | set(int(i) for i in rng.integers(0, n, 48)))[:64]
    assert len(sample) == 64
    for i in sample:
        want = A.chain(msgs[i], keys, scope, sigs[i])
        assert (int(ok[i]), int(st[i])) == (want[2], want[3]), i
        assert tags[i] == (A.canon(sigs[i][-32:]) if want[2] else None)


SHARD_SCRIPT = r"""
import numpy as np
from kyber_amd import devices
from kyber_amd.group import edwards25519 as ed
from tests import _anon_oracle as A, _ring_cases as RC
rows = [r for r in RC.rows() if r.ring == 3 and r.linkable and r.keys == RC.base_keys(3, True)[0]]
rows = [rows[i % len(rows)] for i in range(37)]
args = (b"".join(rows[0].keys), [r.message for r in rows], RC.SCOPE, A.link_base(RC.SCOPE), b"".join(r.sig for r in rows), 3)
start = [i % 3 for i in range(37)]
one = ed.batch_ring_chain(*args, start=start, steps=3)
per = ed.batch_ring_chain(b"".join(b"".join(r.keys) for r in rows), *args[1:])
ch1 = ed.batch_ring_challenge(args[1], RC.SCOPE, b"".join(r.sig[-32:] for r in rows), one[1], one[0])
devices.set_devices([0, 0])
devices.set_shard_threshold(1)
two = ed.batch_ring_chain(*args, start=start, steps=3)
per2 = ed.batch_ring_chain(b"".join(b"".join(r.keys) for r in rows), *args[1:])
ch2 = ed.batch_ring_challenge(args[1], RC.SCOPE, b"".join(r.sig[-32:] for r in rows), one[1], one[0])
devices.set_devices([])
for a, b in zip(one + per + ch1, two + per2 + ch2):
    assert np.array_equal(np.asarray(a), np.asarray(b))
assert one[2].any() and not one[2].all()
print("SHARDED == UNSHARDED")
"""


def test_sharded_call_equals_unsharded_call():
    r = subprocess.run([sys.executable, "-c", SHARD_SCRIPT], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SHARDED == UNSHARDED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
