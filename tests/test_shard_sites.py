"""tests/_shard_cases.py held to the sources and to itself, on the CPU: every `md_active(` site of kyber_amd/csrc is in
SITES and is claimed by a row (a new sharded entry without a row fails here), and every row builds from the oracles alone
at (n, world) = (100, 3) and (67, 8) with its planted rows on the shard boundaries, documented status codes, and, for
the rows with variable-length messages, an empty first message and an odd byte count in front of every shard."""
import glob
import os
import re
import time

import numpy as np
import pytest

from tests import _shard_cases as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kyber_amd", "csrc")
CONFIGS = ((100, 3), (67, 8))
BUILD_SECONDS = 600  # every row at both configurations on one core; the time it does take is printed below
_HEADER = re.compile(r"^(?:static\s+|inline\s+)*int\s+(\w+)\(")  # function definitions start in column 0


def find_sites(root=CSRC):
    found = set()
    for path in sorted(sum((glob.glob(os.path.join(root, "*" + ext)) for ext in (".hip", ".cuh", ".inc")), [])):
        name, func = os.path.basename(path), None
        for line in open(path):
            m = _HEADER.match(line)
            if m and not line.rstrip().endswith(";"):
                func = m.group(1)
            if "md_active(" in line:
                assert func is not None, (name, line)
                found.add((name, func))
    return found


def test_every_sharded_site_is_in_the_table_and_claimed_by_a_row():
    found = find_sites()
    assert found == set(T.SITES), (sorted(found - T.SITES), sorted(T.SITES - found))
    claimed = {r.site for r in T.ROWS.values()}
    assert claimed == set(T.SITES), sorted(T.SITES - claimed)
    # a row's entry point is one that reaches its site: the exported name itself, or the suite's name for a template
    for r in T.ROWS.values():
        entry = T.build(r.name, *CONFIGS[0]).entry
        if r.site[1].startswith("kyb_"):
            assert entry == r.site[1], r.name
        else:
            want = {"mul_host": r"_g[12]_mul(_same_base)?$", "pair_host": r"_pair$", "pair_check_host": r"_pair_check$",
                    "encrypt_host": r"_ibe_encrypt_g[12]$", "decrypt_host": r"_ibe_decrypt_g[12]$", "run_host": r"_msm$"}[r.site[1]]
            assert re.search(want, entry), (r.name, entry)
    # all three suites stand behind the templates, each with every call
    for s in ("bls12381", "bn256", "bn254"):
        entries = {T.build(r.name, *CONFIGS[0]).entry for r in T.ROWS.values() if r.name.startswith(s + "/")}
        assert {"kyb_%s_%s" % (s, e) for e in ("g1_mul", "g2_mul", "g1_mul_same_base", "g2_mul_same_base", "pair", "pair_check", "g1_msm")} <= entries


def required_rows():
    """the roster, restated from the entries' own arguments: every stride, flag and optional array a slice's offsets
    depend on.  A row taken out of tests/_shard_cases.py is missed here."""
    ed = ["mul_base", "mul_base/uniform", "mul_same_base/undecodable base", "dleq_challenge", "msm", "msm/rejects"]
    ed += [e + f for e in ("mul", "mul_same_base") for f in ("", "/uniform", "/vartime")]
    ed += ["verify/" + v for v in ("messages", "empty", "no status")]
    ed += [e + f for e in ("mul2", "theta_check") for f in ("", "/vartime")]
    ed += ["dleq_verify/g%d/h%d/%s" % (g, h, m) for g in (0, 32) for h in (0, 32) for m in ("expect", "fs", "free")]
    ed += ["ring_chain/%s/%s/%s/%s" % (k, s, c, l) for k in ("one ring", "ring each") for s in ("start", "no start")
           for c in ("c_zero", "no c_zero") for l in ("linkable", "unlinkable")]
    ed += ["ring_challenge/linkable", "ring_challenge/unlinkable"]
    rows = ["ed25519/" + r for r in ed]
    bls_flags = ("", "/uncompressed", "/uncompressed out", "/uncompressed trusted both")
    for s in ("bls12381", "bn256", "bn254"):
        for g in (1, 2):
            flags = bls_flags if s == "bls12381" else ("", "/uncompressed") if g == 1 else ("",)
            rows += ["%s/g%d_%s%s" % (s, g, e, f) for e in ("mul", "commit") for f in flags] + ["%s/g%d_commit/rejected base" % (s, g)]
        rows += ["%s/%s%s" % (s, e, f) for e in ("pair", "pair_check") for f in ("", "/uncompressed")] + [s + "/g1_msm"]
    rows += ["bls12381/%s/len %d%s" % (e, ln, f) for e in ("verify_g1", "verify_g2", "verify_g1_same_msg") for ln in (0, 32, 33)
             for f in ("", "/uncompressed")]
    rows += ["bls12381/verify_g1_same_key/key " + k for k in ("a", "b", "bad", "a/uncompressed")]
    return rows + ["bls12381/ibe_encrypt_g2", "bls12381/ibe_decrypt_g2"]


def test_the_table_has_every_row():
    want = required_rows()
    assert len(want) == len(set(want)) == 122
    assert set(T.ROWS) == set(want), (sorted(set(want) - set(T.ROWS)), sorted(set(T.ROWS) - set(want)))
    cheap = [r.site[0] for r in T.ROWS.values() if r.cheap]  # the rows of the degenerate sizes: one per source file
    assert sorted(cheap) == sorted({f for f, _ in T.SITES})


def test_the_site_scan_sees_a_new_site(tmp_path):
    src = tmp_path / "new_call.hip"
    src.write_text("namespace kyb {\nstatic int helper(size_t n);\n}\nint kyb_new_call(size_t n, const uint8_t* a,\n"
                   "                 uint8_t* out) {\n    if (md_active(n))\n        return 0;\n    return 1;\n}\n")
    assert find_sites(str(tmp_path)) == {("new_call.hip", "kyb_new_call")}


def test_every_row_builds_within_budget():
    T.build.cache_clear()
    t0 = time.time()
    slowest = []
    for cfg in CONFIGS:
        for name in T.ROWS:
            t1 = time.time()
            T.build(name, *cfg)
            slowest.append((time.time() - t1, name, cfg))
    dt = time.time() - t0
    print("shard case table: %d rows x %d configurations in %.1f s; slowest: %s"
          % (len(T.ROWS), len(CONFIGS), dt, ", ".join("%s %s %.1f s" % (n, c, s) for s, n, c in sorted(slowest, reverse=True)[:3])))
    assert dt < BUILD_SECONDS, dt


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "n%d-w%d" % c)
def test_partition_and_places(cfg):
    n, world = cfg
    bs = T.bounds(n, world)
    assert bs[0][0] == 0 and bs[-1][1] == n and all(a[1] == b[0] for a, b in zip(bs, bs[1:]))
    sizes = [hi - lo for lo, hi in bs]
    assert max(sizes) - min(sizes) == 1  # uneven, as both configurations are chosen to be
    lo, hi = bs[world // 2]
    places = T.plant_rows(n, world)
    assert places[:3] == [lo, hi - 1, n - 1] and set(places) <= set(T.boundary_rows(n, world))
    assert 0 < lo and hi < n  # a middle shard: neighbours on both sides


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "n%d-w%d" % c)
@pytest.mark.parametrize("name", sorted(T.ROWS))
def test_row_agrees_with_itself(name, cfg):
    n, world = cfg
    c = T.build(name, n, world)
    assert (c.n, c.world) == cfg and c.args[0] == n
    boundary, places = set(T.boundary_rows(n, world)), T.plant_rows(n, world)
    outs = {o.name: o for o in c.outs()}
    assert len(outs) == len(c.outs())
    # planted rows: on the boundaries, the middle shard's first, and with the code they claim
    assert set(c.planted) <= boundary and list(c.planted) == places[:len(c.planted)]
    for row, p in c.planted.items():
        assert p.status in T.DOCUMENTED
        if c.status is not None:
            assert c.status[row] == p.status, (row, p)
        if p.ok is not None:
            assert c.ok[row] == p.ok, (row, p)
        assert p.status != 0 or p.ok == 0 or p.label in ("infinity",), (row, p)  # something a wrong slice would change
    if c.status is not None:
        assert c.status.shape == (n,) and set(int(s) for s in c.status) <= T.DOCUMENTED
        assert {int(s) for s in c.status if s} == {p.status for p in c.planted.values() if p.status} or len(set(c.status)) == 1
    if c.ok is not None:
        assert c.ok.shape == (n,) and "ok" in outs and set(c.ok) <= {0, 1}
        assert all(c.ok[i] == 0 for i in range(n) if c.status is not None and c.status[i])
    # expectations: of declared outputs, of the right width, at every boundary row (where there are any at all)
    for out, rows in c.expect.items():
        assert out in outs and not outs[out].null
        width = int(np.prod(outs[out].shape[1:]))
        assert all(len(v) == width for v in rows.values())
        if out != "v":  # (the IBE's V costs a GT exponentiation a row: at the planted places alone)
            assert boundary | set(c.planted) <= set(rows), (out, sorted(boundary - set(rows)))
        if c.status is not None:
            assert all(v == bytes(width) for i, v in rows.items() if c.status[i] and out != "c_zero")
    for out, v in c.whole.items():
        assert len(v) == int(np.prod(outs[out].shape))
    assert c.expect or c.whole or c.ok is not None, "a row expects something of its outputs"
    # adjacent rows differ in every per-element operand (or the operand is one value for the whole batch)
    for a in c.args:
        if any(a is x for x in c.notes.get("one value", ())):  # (every proof under the one expected challenge)
            continue
        if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[0] == n and a.shape[1] and not (a == a[0]).all():
            # (rows still zero are the ones fill() leaves to the engine)
            same = np.nonzero((a[1:] == a[:-1]).all(axis=1) & (a[1:].any(axis=1) | (c.fill is None)))[0]
            assert not len(same), (name, same[:4])
    # variable-length messages: an empty first message and an odd byte count in front of every shard
    if "lengths" in c.notes and "empty" not in name:
        ln, off = c.notes["lengths"], c.notes["off"]
        assert set(T.MSG_CYCLE) <= set(ln)
        for r, (lo, hi) in enumerate(T.bounds(n, world)):
            assert ln[lo] == 0
            assert r == 0 or int(off[lo]) % 2 == 1, (r, lo, int(off[lo]))
    if name.endswith("verify/empty"):
        assert c.args[2] is None and not c.notes["off"].any()
    if name.endswith("verify/no status"):
        assert c.status is None and outs["status"].null


def test_planted_kinds_cover_what_the_issue_names():
    labels = {}
    for name in T.ROWS:
        for p in T.build(name, *CONFIGS[1]).planted.values():
            labels.setdefault(name.split("/")[0], set()).add((p.label, p.status))
    ed = labels["ed25519"]
    assert {("undecodable key", 1), ("small-order key", 6), ("non-canonical S", 5), ("forged", 0), ("challenge altered", 7)} <= ed
    for s in ("bls12381", "bn256", "bn254"):
        kinds = {l for l, _ in labels[s]}
        assert "infinity" in kinds and "forged" in kinds
        assert ("flag rule" in kinds and "off subgroup" in kinds) if s == "bls12381" else "off curve" in kinds
    assert {st for _, st in labels["bls12381"]} >= {0, 1, 2, 3}


def test_pair_check_rows_are_equal_by_construction():
    """the four lines of a pair_check row under the oracle's own pairings, at a size small enough to afford them"""
    for s in ("bls12381", "bn256"):
        S = T.suite(s)
        a1, a2 = S.line(1, b"check/p", 4)[1], S.product_line(2, b"check/q", b"check/r", 4)
        b1, b2 = S.product_line(1, b"check/p", b"check/q", 4), S.line(2, b"check/r", 4)[1]
        for i in (0, 3):
            assert S.pair(a1[i], a2[i]) == S.pair(b1[i], b2[i])
        assert S.pair(a1[1], a2[1]) != S.pair(b1[2], b2[1])
    S = T.suite("bn254")
    assert S.M.g1_mul(S.scalar(b"check/p/a") * S.scalar(b"check/q/a") % S.order, S.M.G1_GEN) == S.product_line(1, b"check/p", b"check/q", 4)[0]
    p, q = S.line(1, b"check/p", 4)[0][3], S.line(2, b"check/q", 4)[0][3]
    assert S.M.g1_mul(p * q % S.order, S.M.G1_GEN) == S.product_line(1, b"check/p", b"check/q", 4)[3]
