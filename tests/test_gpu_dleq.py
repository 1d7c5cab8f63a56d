"""kyb_ed25519_dleq_challenge and kyb_ed25519_dleq_verify on the GPU against the Python restatement (hashlib + the host
BLAKE2Xb + the big-integer oracle) and against the composed five-call path the fused call replaces."""
import collections
import ctypes as C
import random

import numpy as np
import pytest

from tests import _dleq_cases as DC
from tests import _ed_verify_oracle as V
from tests import _pvss_oracle as PO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _rows4(rows):
    return [np.frombuffer(b"".join(r[k] for r in rows), dtype=np.uint8).reshape(len(rows), 32).copy() for k in range(4)]


def test_challenge_matches_the_python_restatement_byte_for_byte(ed):
    rows = DC.challenge_inputs(4096 + 77)
    # real proofs as well: there the device's canonical-bytes rule must give exactly NewDLEQProof's challenge
    proofs = [r[2:4] + r[6:8] for r in DC.cases(fs=True)[0] if all(PO.canon(p) is not None for p in r[2:4] + r[6:8])]
    rows += proofs
    c, st = ed.batch_dleq_challenge(*_rows4(rows))
    assert not st.any()
    draws = collections.Counter()
    from kyber_amd.util import blake2xb as X
    import hashlib

    for i, r in enumerate(rows):
        assert c[i].tobytes() == PO.device_challenge(*r), i
        draws[X.pick_int(X.New(hashlib.sha256(b"".join(PO.canon_bytes_rule(p) for p in r)).digest()).Read)[1]] += 1
    for i, r in enumerate(proofs):
        assert c[len(rows) - len(proofs) + i].tobytes() == PO.dleq_challenge(*r)
    # the multi-draw seeds' preimages are in the batch: lanes of one wave leave the rejection loop at different trips
    assert all(draws[k] for k in (1, 2, 3, 4)) and max(draws) >= 8, draws
    noncanon = sum(any(PO.canon_bytes_rule(p) != p for p in r) for r in rows)
    assert noncanon >= 500


def test_challenge_across_pieces_and_on_a_side_stream(ed):
    import torch

    n = (1 << 18) + 5  # crosses ED_PIECE
    rng = np.random.default_rng(5)
    a = [torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda() for _ in range(4)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c, st = ed.batch_dleq_challenge(*a)
    s.synchronize()
    assert not st.any().item()
    c = c.cpu().numpy()
    host = [x.cpu().numpy() for x in a]
    for i in list(range(0, n, 4099)) + [(1 << 18) - 1, 1 << 18, n - 1]:
        assert c[i].tobytes() == PO.device_challenge(*[h[i].tobytes() for h in host]), i
    c2, _ = ed.batch_dleq_challenge(*[h[-300:] for h in host])  # host buffers, another batch size: the same bytes
    assert (c2 == c[-300:]).all()


def _all_rows(vartime, fs=False):
    rows, labels = DC.cases(fs=fs)
    extra = [DC.commitments_from_equations(r, vartime) for r, l in zip(rows, labels) if l == "edge-scalars"]
    return rows + extra, labels + ["edge-valid"] * len(extra)


@pytest.mark.parametrize("vartime", [False, True])
def test_verify_matches_the_oracle_and_the_composed_path(ed, vartime):
    from kyber_amd.proof import dleq

    rows, labels = _all_rows(vartime)
    a = DC.pack(rows)
    ok, st = ed.batch_dleq_verify(*a, vartime=vartime)
    want = DC.oracle_ok(rows, vartime)
    composed = dleq.batch_verify_composed(*a, vartime=vartime)
    for i, r in enumerate(rows):
        assert bool(ok[i]) == want[i] == composed[i], (i, labels[i], ok[i], want[i], composed[i])
        assert st[i] == PO.abi_status(*r[:5]), (i, labels[i])
    by = collections.defaultdict(list)
    for l, o in zip(labels, ok):
        by[l].append(bool(o))
    for l in ("valid", "edge-valid", "vG-plus-p", "vH-plus-p", "vG-minus-zero", "both-minus-zero-noncanonical"):
        assert by[l] and all(by[l]), l
    assert not any(o for l, v in by.items() if l.startswith(("tampered", "undecodable")) or l.endswith("wrong") for o in v)
    assert sum(l.startswith("tampered") for l in labels) == 16 and sum(l.startswith("undecodable") for l in labels) == 6
    if not vartime:
        assert (dleq.batch_verify(*a) == want).all()  # the public entry rides the fused call


def test_fiat_shamir_flag_expected_challenge_and_precedence(ed):
    rows, labels = DC.cases(seed=4, fs=True)
    a = DC.pack(rows)
    ok, st = ed.batch_dleq_verify(*a, fiat_shamir=True)
    want = DC.oracle_ok(rows)
    for i, r in enumerate(rows):
        s = PO.abi_status(*r[:5], fs_with=r[6:8])
        assert st[i] == s and bool(ok[i]) == (want[i] and s == 0), (i, labels[i])
    assert all(ok[i] for i, l in enumerate(labels) if l == "valid")
    assert {int(st[i]) for i, l in enumerate(labels) if l in ("C-plus-l", "tampered-C", "tampered-VG", "tampered-xH")} == {7}
    ok_v, st_v = ed.batch_dleq_verify(*a, fiat_shamir=True, vartime=True)  # both flags together
    assert (st_v == st).all() and (ok_v == ok).all()
    # precedence: a wrong challenge and an undecodable G report the challenge; without the flag, the point
    both = [list(rows[0])]
    both[0][0], both[0][4] = V._not_on_curve(), bytes(32)
    assert ed.batch_dleq_verify(*DC.pack(both), fiat_shamir=True)[1][0] == 7
    assert ed.batch_dleq_verify(*DC.pack(both))[1][0] == 1
    assert ed.batch_dleq_verify(*DC.pack(both), expect_c=bytes(31) + b"\x02")[1][0] == 7
    # expect_c right and wrong, on proofs that share one challenge
    rng = random.Random(8)
    rows2 = [DC.valid_proof(rng) for _ in range(200)]
    c0 = rows2[0][4]
    rows2 = [DC.commitments_from_equations(r[:4] + [c0] + r[5:], False) for r in rows2]
    rows2[7][4] = PO.sc(PO.le(c0) + 1)
    ok, st = ed.batch_dleq_verify(*DC.pack(rows2), expect_c=c0)
    assert list(np.flatnonzero(ok == 0)) == [7] and list(np.flatnonzero(st)) == [7] and st[7] == 7
    ok, st = ed.batch_dleq_verify(*DC.pack(rows2), expect_c=PO.sc(PO.le(c0) + PO.O.L - 1))
    assert not ok.any() and set(st) == {7}
    # stride 0 against the same base replicated
    rows3 = [DC.commitments_from_equations([rows2[0][0], rows2[1][1]] + r[2:], False) for r in rows2]
    rows3[11][6] = rows3[12][6]
    p = DC.pack(rows3)
    full = ed.batch_dleq_verify(*p)
    shared = ed.batch_dleq_verify(p[0][:1], p[1][:1], *p[2:])
    mixed = ed.batch_dleq_verify(p[0], p[1][:1], *p[2:])
    for got in (shared, mixed):
        assert (got[0] == full[0]).all() and (got[1] == full[1]).all()
    assert list(np.flatnonzero(full[0] == 0)) == [11]


def test_dev_twin_on_a_side_stream_and_two_shards_of_one_device(ed):
    import torch

    from kyber_amd import devices

    rows, labels = _all_rows(False, fs=True)
    rows = rows * 12  # several waves, a chunk boundary of the encoder inside
    a = DC.pack(rows)
    ref_ok, ref_st = ed.batch_dleq_verify(*a, fiat_shamir=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = [torch.from_numpy(x).cuda() for x in a]
        ok, st = ed.batch_dleq_verify(*d, fiat_shamir=True)
        ok2, st2 = ed.batch_dleq_verify(d[0][:1].clone(), *d[1:], expect_c=d[4][0].clone())
    s.synchronize()
    assert (ok.cpu().numpy() == ref_ok).all() and (st.cpu().numpy() == ref_st).all()
    h_ok2, h_st2 = ed.batch_dleq_verify(a[0][:1], *a[1:], expect_c=a[4][0])
    assert (ok2.cpu().numpy() == h_ok2).all() and (st2.cpu().numpy() == h_st2).all()
    devices.set_devices([0, 0])
    devices.set_shard_threshold(1)
    try:
        ok, st = ed.batch_dleq_verify(*a, fiat_shamir=True)
        assert (ok == ref_ok).all() and (st == ref_st).all()
        ok, st = ed.batch_dleq_verify(a[0][:1], *a[1:], expect_c=a[4][0])  # a shared base goes to every shard
        assert (ok == h_ok2).all() and (st == h_st2).all()
        c, _ = ed.batch_dleq_challenge(a[2], a[3], a[6], a[7])
    finally:
        devices.set_devices([])
        devices.set_shard_threshold(16384)
    c1, _ = ed.batch_dleq_challenge(a[2], a[3], a[6], a[7])
    assert (c == c1).all()


def test_null_status_and_large_batch_across_pieces(ed):
    from kyber_amd import _lib

    lib = _lib.load()
    rng = random.Random(21)
    base = [DC.valid_proof(rng, fs=True) for _ in range(64)]
    bad = list(base[5])
    bad[5] = PO.sc(PO.le(bad[5]) + 1)
    n = (1 << 18) + 5
    idx = np.arange(n) % 64
    a = [x[idx] for x in DC.pack(base)]
    a[5][n - 2] = np.frombuffer(bad[5], dtype=np.uint8)
    a[5][1 << 18] = np.frombuffer(bad[5], dtype=np.uint8)
    ok, st = np.full(n, 9, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)
    _lib.check(lib.kyb_ed25519_dleq_verify(n, a[0].ctypes.data, 32, a[1].ctypes.data, 32, *[x.ctypes.data for x in a[2:]], None,
                                           ok.ctypes.data, None, _lib.KYB_F_DLEQ_FS), "kyb_ed25519_dleq_verify")
    want = np.ones(n, dtype=np.uint8)
    want[[n - 2, 1 << 18]] = 0  # a foreign response on either side of the piece boundary
    assert (ok == want).all() and (st == 255).all()
