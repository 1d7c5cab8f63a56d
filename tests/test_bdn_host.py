"""sign/bdn on the pairing suites without a GPU: kyber_amd/csrc/blake2xs.cuh and bdn.cuh compiled for the CPU
(tests/bdn_harness.cpp) against the oracle's labelled table (tests/_bdn_cases.py) for all six (suite, group) pairs --
the roster, coefficient and term lanes, the table build at both widths, the slice lanes at S in {1, 2, groups} in both
polarities, the fold and the finish -- the oracle itself against the bytes the reference prints for bn256, BLAKE2Xs at
the block edges, the plan against a restatement, and the C ABI's argument checks through the built library."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from kyber_amd import _lib
from kyber_amd.util.blake2xs import blake2xs
from tests import _bdn_cases as BC
from tests import _bdn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libbdnharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "bdn_harness.cpp")])
    h = C.CDLL(out)
    h.bdh_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p]
    h.bdh_plan.restype = None
    h.bdh_additions.argtypes = [C.c_size_t, C.c_size_t, C.c_int]
    h.bdh_additions.restype = C.c_size_t
    h.bdh_blake2xs.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    h.bdh_blake2xs.restype = None
    h.bdh_terms.argtypes = [C.c_int, C.c_size_t] + [C.c_void_p] * 4 + [C.c_uint32]
    h.bdh_terms.restype = None
    h.bdh_aggregate.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_uint32]
    h.bdh_aggregate.restype = None
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def ptr(a):
    return None if a is None else a.ctypes.data


def run_terms(h, G, roster, flags=0, want=True):
    m = len(roster)
    r = BC.pack(roster, G.POINT)
    coefs, tm, st = np.full((m, 16), 7, np.uint8), np.full((m, G.POINT), 7, np.uint8), np.full(m, 7, np.uint8)
    h.bdh_terms(G.which, m, ptr(r), ptr(coefs) if want else None, ptr(tm), ptr(st) if want else None, flags)
    return [c.tobytes() for c in coefs], [t.tobytes() for t in tm], list(st)


def run_aggregate(h, G, pts, ms, g, S, stride, flags=0, want=True):
    m, n = len(pts), len(ms)
    p, flat = BC.pack(pts, G.POINT), BC.pack_masks(ms, m, stride)
    out, cnt, st = np.full((n, G.POINT), 7, np.uint8), np.zeros(n, np.uint32), np.full(n, 7, np.uint8)
    h.bdh_aggregate(G.which, n, m, g, S, ptr(p), ptr(flat), stride, ptr(out), ptr(cnt) if want else None, ptr(st) if want else None, flags)
    return [(o.tobytes(), int(c), int(s)) for o, c, s in zip(out, cnt, st)]


# ---- the oracle against the reference's printed bytes (bn256 only: the reference prints no others)
@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "bn256.json")))


def test_oracle_matches_the_reference_fixtures(golden):
    from oracle import bn256 as ON

    G2, G1 = O.BY_NAME["bn256_g2"], O.BY_NAME["bn256_g1"]
    # TestBDN_HashPointToR_BN256 (bdn_vartime_test.go:24-48): P, 2 P, 3 P, every bit set
    pubs = [ON.g2_marshal(ON.g2_mul(i, ON.G2_GEN)) for i in (1, 2, 3)]
    coefs, terms, st = O.new_mask(G2, pubs)
    assert st == [0, 0, 0] and [c[::-1].hex() for c in coefs] == golden["bdn_coefs"]
    assert O.aggregate(G2, terms, b"\x07")[0].hex() == golden["bdn_agg_key"]
    # TestBDNFixtures (bdn_vartime_test.go:104-146): mask 101
    pubs = [bytes.fromhex(p) for p in golden["bdn_pubs"]]
    sigs = [bytes.fromhex(s) for s in golden["bdn_sigs"]]
    coefs, terms, st = O.new_mask(G2, pubs)
    assert O.aggregate(G2, terms, b"\x05") == (bytes.fromhex(golden["bdn_fixture_agg_key_mask101"]), 2, 0)
    ints = [int.from_bytes(c, "little") for c in coefs]
    assert O.aggregate_signatures(G1, [sigs[0], sigs[2]], ints, b"\x05", 3).hex() == golden["bdn_fixture_agg_sig_mask101"]
    # TestBDN_AggregateSignatures' length errors and an undecodable signature, in the loop's order (bdn.go:128-158)
    for bad in ([sigs[0]], [sigs[0], sigs[2], sigs[1]]):
        with pytest.raises(ValueError, match="length of signatures and public keys must match"):
            O.aggregate_signatures(G1, bad, ints, b"\x05", 3)
    with pytest.raises(ValueError, match="invalid signature"):
        O.aggregate_signatures(G1, [bytes(63) + b"\x05", sigs[2], sigs[1]], ints, b"\x05", 3)


# ---- BLAKE2Xs
@pytest.mark.parametrize("length", [0, 63, 64, 65, 128, 200])
def test_blake2xs_matches_the_python_mirror_at_the_block_edges(harness, length):
    data = np.frombuffer(bytes((7 * i + length) & 0xFF for i in range(length)) + b"\0", dtype=np.uint8).copy()[:max(length, 1)]
    for ncoef in (1, 2, 5):  # an odd count ends in half an output node
        out = np.zeros(16 * ncoef, np.uint8)
        harness.bdh_blake2xs(ptr(data), length, ncoef, ptr(out))
        assert out.tobytes() == blake2xs(data.tobytes()[:length], 16 * ncoef), (length, ncoef)


# ---- the lane programs over the table
def slice_counts(m, g):
    nb = (m + g - 1) // g
    return sorted({1, min(2, nb), nb})


@pytest.mark.parametrize("G", O.GROUPS, ids=lambda G: G.name)
def test_lane_programs_match_the_oracle_on_the_labelled_table(harness, G):
    for name in BC.names(G):
        roster = BC.roster(G.name, name)
        m = len(roster)
        want = BC.terms(G.name, name)
        assert run_terms(harness, G, roster) == (list(want[0]), list(want[1]), list(want[2])), (G.name, name)
        assert run_terms(harness, G, roster, want=False)[1] == list(want[1]), (G.name, name)  # coefs and status left out
        pts, ms, ex = BC.points(G.name, name), [mk for _, mk in BC.masks(m)], list(BC.expected(G.name, name))
        for g in (4, 8):
            stride = O.mask_len(m) + (3 if g == 8 else 0)  # an odd stride at one width, the exact one at the other
            for S in slice_counts(m, g):
                got = run_aggregate(harness, G, pts, ms, g, S, stride)
                for (label, _), a, b in zip(BC.masks(m), got, ex):
                    assert a == b, (G.name, name, g, S, label)
            got = run_aggregate(harness, G, pts, ms, g, 1, stride, want=False)
            assert [o for o, _, _ in got] == [o for o, _, _ in ex], (G.name, name, g)


def test_special_rosters_say_what_their_names_say():
    for G in O.GROUPS:
        coefs, terms, st = BC.terms(G.name, "undecodable")
        assert st == [0, 0, 0, O.ST_BAD_POINT, 0] and set(coefs) == {bytes(16)} and set(terms) == {bytes(G.POINT)}
        assert all(e[2] == O.ST_BAD_POINT and e[0] == bytes(G.POINT) for e in BC.expected(G.name, "undecodable"))
        assert BC.terms(G.name, "identity")[1][1] == G.marshal(None)  # (c + 1) O = O
        full = dict(zip([l for l, _ in BC.masks(5)], BC.expected(G.name, "opposite")))["full"]
        assert full[1] == 5 and full[2] == 0
    for g in ("g1", "g2"):
        a, b = BC.terms(f"bn256_{g}", "xplusp"), BC.terms(f"bn256_{g}", "m3")
        assert BC.roster(f"bn256_{g}", "xplusp") != BC.roster(f"bn256_{g}", "m3") and a == b
    assert BC.terms("bls12381_g1", "offsub")[2] == [0, O.ST_NOT_IN_SUBGROUP, 0]


def test_off_subgroup_key_with_and_without_the_trusted_flag(harness):
    """Unvouched, the key is rejected and nothing is defined.  Vouched for, the statuses are clean and the coefficients
    are the hash of the canonical bytes; the ladder's value on a point off the subgroup is the caller's, as with
    kyb_bls12381_g1_mul, but the masked SUM over such points is plain additions and has one value."""
    G = O.BY_NAME["bls12381_g1"]
    roster = BC.roster(G.name, "offsub")
    coefs, terms, st = run_terms(harness, G, roster)
    assert st == [0, O.ST_NOT_IN_SUBGROUP, 0] and set(coefs) == {bytes(16)} and set(terms) == {bytes(48)}
    coefs, terms, st = run_terms(harness, G, roster, O.F_TRUSTED)
    want = BC.terms(G.name, "offsub", O.F_TRUSTED)
    assert st == [0, 0, 0] and coefs == list(want[0]) and (terms[0], terms[2]) == (want[1][0], want[1][2])
    ms = [mk for _, mk in BC.masks(3)]
    for flags in (0, O.F_TRUSTED):
        ex = [O.aggregate(G, roster, mk, flags) for mk in ms]
        assert run_aggregate(harness, G, roster, ms, 4, 1, 1, flags) == ex
        assert ex[0][2] == (0 if flags else O.ST_NOT_IN_SUBGROUP)


# ---- the plan
def test_plan_matches_its_restatement_on_both_sides_of_each_edge(harness):
    lib = _lib.load()
    got = (C.c_int * 2)()
    ns = [1, 2, 63, 64, 65, 224, 225, 226, 1000, 21845, 21846, 32767, 32768, 32769, 65535, 65536, 65537, 1 << 20]
    for m in (1, 3, 4, 5, 8, 9, 16, 17, 64, 1000, 3000, 8191, 8192):
        for n in ns:
            want = O.plan(n, m)
            assert lib.kyb_bdn_plan(n, m, got) == 0 and (got[0], got[1]) == want, (n, m)
            mine = (C.c_int * 2)()
            harness.bdh_plan(n, m, C.addressof(mine))
            assert (mine[0], mine[1]) == want
            assert got[0] == lib.kyb_ed25519_cosi_group_width(n, m)  # the width rule is sign/cosi's
            assert 1 <= got[1] <= (m + got[0] - 1) // got[0]
        assert O.plan(65536, m)[1] == 1  # n alone fills the device
    assert [O.plan(n, 64)[0] for n in (224, 225)] == [4, 8]
    assert O.plan(1, 3000) == (4, 750) and O.plan(65535, 3000)[1] == 2
    for args in ((0, 9), (4, 0), (4, 8193)):
        assert lib.kyb_bdn_plan(*args, got) == -1 and b"kyb_bdn_plan:" in lib.kyb_last_error()
    assert lib.kyb_bdn_plan(4, 9, None) == -1
    # the measurement hook overrides what a call does, never what the plan reports
    assert lib.kyb_bdn_debug_set_slices(7) == 0 and lib.kyb_bdn_plan(1, 3000, got) == 0 and (got[0], got[1]) == (4, 750)
    assert lib.kyb_bdn_debug_set_slices(0) == 0


# ---- the C ABI's argument rules, with no device
@pytest.mark.parametrize("G", O.GROUPS, ids=lambda G: G.name)
def test_argument_errors_need_no_device(G):
    lib = _lib.load()
    buf = C.create_string_buffer(1 << 16)
    p = C.addressof(buf)
    terms, agg = f"kyb_{G.suite}_bdn_terms_{G.g}", f"kyb_{G.suite}_mask_aggregate_{G.g}"
    # m, roster, coefs, terms, status, flags
    bad = [(0, p, p, p, p, 0), (8193, p, p, p, p, 0), (9, None, p, p, p, 0), (9, p, p, None, p, 0), (9, p, p, p, p, 1), (9, p, p, p, p, 2),
           (9, p, p, p, p, 0x200), (9, p, p, p, p, 0x104)]
    for args in bad:
        for name, extra in ((terms, ()), (terms + "_dev", (None,))):
            assert getattr(lib, name)(*args, *extra) == -1, (name, args)
            assert name.encode() + b":" in lib.kyb_last_error(), (name, lib.kyb_last_error())
    # n = 0 is KYB_OK and touches nothing
    assert getattr(lib, agg)(0, 9, p, p, 2, p, p, p, 0) == 0
    assert getattr(lib, agg)(0, 9, None, None, 2, None, None, None, 0x100) == 0
    assert getattr(lib, agg + "_dev")(0, 9, None, None, 2, None, None, None, 0, None) == 0
    # n, m, points, masks, mask_stride, out, count, status, flags
    bad = [(4, 9, p, p, 2, p, p, p, 1), (4, 9, p, p, 2, p, p, p, 0x200), (4, 9, p, p, 2, p, p, p, 0x102), (4, 0, p, p, 2, p, p, p, 0),
           (4, 8193, p, p, 1025, p, p, p, 0), (4, 9, p, p, 1, p, p, p, 0), (4, 8, p, p, 0, p, p, p, 0), (4, 9, None, p, 2, p, p, p, 0),
           (4, 9, p, None, 2, p, p, p, 0), (4, 9, p, p, 2, None, p, p, 0), (0, 9, p, p, 1, p, p, p, 0)]
    for args in bad:
        for name, extra in ((agg, ()), (agg + "_dev", (None,))):
            assert getattr(lib, name)(*args, *extra) == -1, (name, args)
            assert name.encode() + b":" in lib.kyb_last_error(), (name, lib.kyb_last_error())
    assert getattr(lib, agg)(4, 8192, None, p, 1024, p, p, p, 0) == -1  # the widest roster is a roster


def test_header_cites_the_reference_lines_and_the_current_device():
    src = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    item = src[src.index("sign/bdn on the pairing suites"):src.index("int kyb_bls12381_bdn_terms_g1(")]
    item = " ".join(item.replace(" * ", " ").split())
    for cite in ("mask.go:51-61", "bdn.go:29-63", "mask.go:59-60", "bdn.go:166-181", "KYB_COSI_MAX_ROSTER", "mask_stride >= L",
                 "kyb_ed25519_mask_aggregate", "run on the current device", "16-byte aligned", "bytes"):
        assert cite in item, cite
    for unit in ("bdn_launch.cuh", "bls12381_bdn.hip", "bn256_bdn.hip", "bn254_bdn.hip", "bdn_plan.hip"):
        hip = open(os.path.join(ROOT, "kyber_amd", "csrc", unit)).read()
        assert "md_active(" not in hip, unit
    for suite in ("bls12381", "bn256", "bn254"):
        for g in ("g1", "g2"):
            for stem in (f"kyb_{suite}_bdn_terms_{g}", f"kyb_{suite}_mask_aggregate_{g}"):
                assert stem in _lib.SIGNATURES and stem + "_dev" in _lib.SIGNATURES
