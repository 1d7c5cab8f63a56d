"""sign/bdn on the GPU: the labelled table of tests/_bdn_cases.py through the host and the device entry of
kyb_<suite>_bdn_terms_<g> and kyb_<suite>_mask_aggregate_<g> for all six (suite, group) pairs, byte for byte against
the oracle; n at the wave edges; one n on each side of the width rule and of S = 1, found through kyb_bdn_plan; count
and status present and NULL; the reference's printed fixtures through Mask / Scheme; and VerifyBatch against
AggregatePublicKeys + Verify with a forged signature, a flipped mask bit and a rogue key."""
import json
import os

import numpy as np
import pytest

from tests import _bdn_cases as BC
from tests import _bdn_oracle as O

pytestmark = pytest.mark.gpu


def lib():
    from kyber_amd import _lib

    return _lib.load()


def raw_terms(G, roster, flags, device, want=True):
    import torch

    m = len(roster)
    r = BC.pack(roster, G.POINT)
    name = f"kyb_{G.suite}_bdn_terms_{G.g}"
    if device:
        d_r = torch.from_numpy(r).cuda()
        coefs = torch.full((m, 16), 0xEE, dtype=torch.uint8, device="cuda")
        tm = torch.full((m, G.POINT), 0xEE, dtype=torch.uint8, device="cuda")
        st = torch.full((m,), 0xEE, dtype=torch.uint8, device="cuda")
        rc = getattr(lib(), name + "_dev")(m, d_r.data_ptr(), coefs.data_ptr() if want else None, tm.data_ptr(),
                                           st.data_ptr() if want else None, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        coefs, tm, st = coefs.cpu().numpy(), tm.cpu().numpy(), st.cpu().numpy()
    else:
        coefs, tm, st = np.full((m, 16), 0xEE, np.uint8), np.full((m, G.POINT), 0xEE, np.uint8), np.full(m, 0xEE, np.uint8)
        rc = getattr(lib(), name)(m, r.ctypes.data, coefs.ctypes.data if want else None, tm.ctypes.data, st.ctypes.data if want else None, flags)
    assert rc == 0, lib().kyb_last_error()
    return [c.tobytes() for c in coefs], [t.tobytes() for t in tm], [int(s) for s in st]


def raw_aggregate(G, pts, ms, stride, flags, device, want=True):
    """the C ABI itself, so that count and status can be NULL and the mask buffer ends with the last mask"""
    import torch

    m, n = len(pts), len(ms)
    p, flat = BC.pack(pts, G.POINT), BC.pack_masks(ms, m, stride)
    name = f"kyb_{G.suite}_mask_aggregate_{G.g}"
    if device:
        d_p, d_m = torch.from_numpy(p).cuda(), torch.from_numpy(flat).cuda()
        out = torch.full((n, G.POINT), 0xEE, dtype=torch.uint8, device="cuda")
        cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        rc = getattr(lib(), name + "_dev")(n, m, d_p.data_ptr(), d_m.data_ptr(), stride, out.data_ptr(), cnt.data_ptr() if want else None,
                                           st.data_ptr() if want else None, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out, cnt, st = out.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy()
    else:
        out, cnt, st = np.full((n, G.POINT), 0xEE, np.uint8), np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, 0xEE, np.uint8)
        rc = getattr(lib(), name)(n, m, p.ctypes.data, flat.ctypes.data, stride, out.ctypes.data, cnt.ctypes.data if want else None,
                                  st.ctypes.data if want else None, flags)
    assert rc == 0, lib().kyb_last_error()
    return out, cnt, st


def rows_of(ex, G):
    return (np.frombuffer(b"".join(e[0] for e in ex), dtype=np.uint8).reshape(len(ex), G.POINT), [e[1] for e in ex], [e[2] for e in ex])


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("G", O.GROUPS, ids=lambda G: G.name)
def test_the_labelled_table_through_both_entries(G, device):
    for name in BC.names(G):
        roster = BC.roster(G.name, name)
        m = len(roster)
        want = BC.terms(G.name, name)
        assert raw_terms(G, roster, 0, device) == (list(want[0]), list(want[1]), list(want[2])), (G.name, name)
        pts, ms, ex = BC.points(G.name, name), [mk for _, mk in BC.masks(m)], BC.expected(G.name, name)
        wout, wcnt, wst = rows_of(ex, G)
        stride = O.mask_len(m) + (3 if device else 0)  # an odd stride through one entry, the exact one through the other
        out, cnt, st = raw_aggregate(G, pts, ms, stride, 0, device)
        assert (out == wout).all() and [int(c) for c in cnt] == wcnt and [int(s) for s in st] == wst, (G.name, name)
    # count, coefs and status left out: the same bytes, and the buffers left alone
    roster = BC.roster(G.name, "m9")
    assert raw_terms(G, roster, 0, device, want=False)[1] == list(BC.terms(G.name, "m9")[1])
    out, cnt, st = raw_aggregate(G, BC.points(G.name, "m9"), [mk for _, mk in BC.masks(9)], 2, 0, device, want=False)
    assert (out == rows_of(BC.expected(G.name, "m9"), G)[0]).all() and (st == 0xEE).all()


def tiled(G, name, n):
    """n masks cycling through the table's, with what the oracle expects of each"""
    m = len(BC.roster(G.name, name))
    base, ex = BC.masks(m), BC.expected(G.name, name)
    idx = [(5 * i + i // 7) % len(base) for i in range(n)]
    rows = np.stack([np.frombuffer(e[0], dtype=np.uint8) for e in ex])
    return [base[k][1] for k in idx], rows[idx], np.array([ex[k][1] for k in idx])


@pytest.mark.parametrize("gname", ["bls12381_g1", "bn256_g1", "bn254_g1", "bn256_g2", "bls12381_g2"])
def test_batch_sizes_at_the_wave_edges(gname):
    G = O.BY_NAME[gname]
    name = "m5" if G.g == "g2" else "m9"
    for n in (1, 63, 64, 65, 130):
        ms, wout, wcnt = tiled(G, name, n)
        out, cnt, st = raw_aggregate(G, BC.points(gname, name), ms, O.mask_len(len(BC.roster(gname, name))), O.F_TRUSTED, n & 1 == 0)
        assert (out == wout).all() and (cnt == wcnt).all() and not st.any(), (gname, n)


def plan(n, m):
    from kyber_amd.pairing import bn256

    return bn256.ENGINE.bdn_plan(n, m)


def edge(pred, lo=1, hi=1 << 20):
    """the largest n with pred(n) and the next one; pred(lo) holds, pred(hi) does not"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo, hi


@pytest.mark.parametrize("gname,name", [("bls12381_g1", "m17"), ("bn256_g1", "m9"), ("bn256_g2", "m9")])
def test_each_side_of_the_width_rule_and_of_one_slice(gname, name):
    G = O.BY_NAME[gname]
    m = len(BC.roster(gname, name))
    sizes = list(edge(lambda n: plan(n, m)[1] > 1))  # the last n cut into slices and the first that is not
    assert plan(sizes[0], m)[1] == 2 and plan(sizes[1], m)[1] == 1 and sizes[1] == 65536
    if G.g == "g1":  # the large side of the width rule on G1 only
        sizes += list(edge(lambda n: plan(n, m)[0] == 4))
        assert plan(sizes[2], m)[0] == 4 and plan(sizes[3], m)[0] == 8
    for n in sizes:
        ms, wout, wcnt = tiled(G, name, n)
        out, cnt, st = raw_aggregate(G, BC.points(gname, name), ms, O.mask_len(m), O.F_TRUSTED, True)
        assert (out == wout).all() and (cnt == wcnt).all() and not st.any(), (gname, n, plan(n, m))


def test_off_subgroup_key_on_the_device():
    G = O.BY_NAME["bls12381_g1"]
    roster = BC.roster(G.name, "offsub")
    for device in (False, True):
        coefs, terms, st = raw_terms(G, roster, 0, device)
        assert st == [0, O.ST_NOT_IN_SUBGROUP, 0] and set(coefs) == {bytes(16)} and set(terms) == {bytes(48)}
        coefs, terms, st = raw_terms(G, roster, O.F_TRUSTED, device)
        want = BC.terms(G.name, "offsub", O.F_TRUSTED)
        assert st == [0, 0, 0] and coefs == list(want[0]) and (terms[0], terms[2]) == (want[1][0], want[1][2])
        ms = [mk for _, mk in BC.masks(3)]
        for flags in (0, O.F_TRUSTED):
            wout, wcnt, wst = rows_of([O.aggregate(G, roster, mk, flags) for mk in ms], G)
            out, cnt, st = raw_aggregate(G, roster, ms, 1, flags, device)
            assert (out == wout).all() and [int(s) for s in st] == wst and [int(c) for c in cnt] == wcnt


# ---- the reference's fixtures through Mask / Scheme
@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "bn256.json")))


def test_hash_point_to_r_bn256_fixture(golden):  # TestBDN_HashPointToR_BN256 (bdn_vartime_test.go:24-48)
    from kyber_amd.pairing import bn256
    from kyber_amd.sign import bdn

    suite = bn256.NewSuite()
    pubs = [suite.G2().Point().Mul(bn256.Scalar(i), None) for i in (1, 2, 3)]
    mask = bdn.NewMask(suite.G2(), pubs)
    assert [f"{c:032x}" for c in mask.publicCoefs] == golden["bdn_coefs"]
    assert mask.CountEnabled() == 0 and mask.CountTotal() == 3 and mask.Len() == 1
    for i in range(3):
        mask.SetBit(i, True)
    assert bdn.AggregatePublicKeys(bn256, mask).MarshalBinary().hex() == golden["bdn_agg_key"]
    assert bdn.NewSchemeOnG1(bn256).AggregatePublicKeys(bdn.NewMask(suite.G2(), pubs)).enc == bn256.G2_NULL  # the empty mask


def test_bdn_fixtures_through_mask_and_scheme(golden):  # TestBDNFixtures (bdn_vartime_test.go:104-146)
    from kyber_amd.pairing import bn256
    from kyber_amd.sign import bdn

    sch = bdn.NewSchemeOnG1(bn256)
    msg = golden["bdn_msg"].encode()
    privs = [bn256.Scalar().UnmarshalBinary(bytes.fromhex(p)) for p in golden["bdn_privs"]]
    pubs = [bn256.G2Elt().UnmarshalBinary(bytes.fromhex(p)) for p in golden["bdn_pubs"]]
    sigs = [sch.Sign(x, msg) for x in privs]
    assert [s.hex() for s in sigs] == golden["bdn_sigs"]
    mask = bdn.NewMask(bn256.NewSuite().G2(), pubs)
    mask.SetBit(0, True)
    mask.SetBit(2, True)
    agg_sig = sch.AggregateSignatures([sigs[0], sigs[2]], mask)
    agg_key = sch.AggregatePublicKeys(mask)
    assert agg_sig.MarshalBinary().hex() == golden["bdn_fixture_agg_sig_mask101"]
    assert agg_key.MarshalBinary().hex() == golden["bdn_fixture_agg_key_mask101"]
    sch.Verify(agg_key, msg, agg_sig.MarshalBinary())
    # TestBDN_AggregateSignatures' errors, in the order of the loop of bdn.go:128-158
    for bad in ([sigs[0]], sigs):
        with pytest.raises(ValueError, match="length of signatures and public keys must match"):
            sch.AggregateSignatures(bad, mask)
    with pytest.raises(ValueError, match="malformed point"):
        sch.AggregateSignatures([bytes(63) + b"\x05", sigs[2], sigs[1]], mask)  # the undecodable one is met first
    with pytest.raises(ValueError, match="length of signatures"):
        sch.AggregateSignatures([sigs[0], sigs[2], bytes(63) + b"\x05"], mask)  # the loop never reaches the third
    # a clone shares the terms: the subset signature of TestBDN_SubsetSignature
    sub = mask.Clone()
    sub.SetBit(0, False)
    key2 = sch.AggregatePublicKeys(sub)
    sch.Verify(key2, msg, sch.AggregateSignatures([sigs[2]], sub).MarshalBinary())
    with pytest.raises(ValueError, match="bls: invalid signature"):
        sch.Verify(key2, msg, agg_sig.MarshalBinary())
    assert mask.GetBit(0) and sch.AggregatePublicKeys(mask).Equal(agg_key)


def schemes():
    from kyber_amd.pairing import bls12381, bn256
    from kyber_amd.sign import bdn

    return {"bn256-on-g1": (bn256, bdn.NewSchemeOnG1(bn256)), "bls12381-on-g1": (bls12381, bdn.NewSchemeOnG1(bls12381)),
            "bls12381-on-g2": (bls12381, bdn.NewSchemeOnG2(bls12381))}


@pytest.mark.parametrize("which", ["bn256-on-g1", "bls12381-on-g1", "bls12381-on-g2"])
def test_verify_batch_is_aggregate_then_verify(which):
    from kyber_amd.sign import bdn

    suite, sch = schemes()[which]
    key_group = suite.NewSuite().G2() if sch.key_group == 2 else suite.NewSuite().G1()
    seed = iter(range(1, 1 << 20))
    rand = lambda n: bytes((37 * next(seed) + 11 * k) & 0x7F for k in range(n))
    pairs = [sch.NewKeyPair(rand) for _ in range(4)]
    pubs = [X for _, X in pairs]
    base = bdn.NewMask(key_group, pubs)
    msgs = [b"block %d" % i for i in range(4)]
    bitmasks = [bytes([0b1111]), bytes([0b0101]), bytes([0b1110]), bytes([0b1000])]
    sigs = []
    for msg, bm in zip(msgs, bitmasks):
        mk = base.Clone()
        mk.SetMask(bytearray(bm))
        each = [sch.Sign(x, msg) for i, (x, _) in enumerate(pairs) if bm[0] >> i & 1]
        sigs.append(sch.AggregateSignatures(each, mk).MarshalBinary())
    # element 1 carries element 0's signature (a forgery for its message); element 2's mask has one bit flipped
    rows_m = msgs + [msgs[1], msgs[2]]
    rows_s = sigs + [sigs[0], sigs[2]]
    rows_b = bitmasks + [bitmasks[1], bytes([0b1111])]
    got = sch.VerifyBatch(base, rows_m, rows_s, rows_b)
    assert list(got) == [True, True, True, True, False, False]
    for msg, sig, bm, ok in zip(rows_m, rows_s, rows_b, got):  # per element: AggregatePublicKeys + Verify
        mk = base.Clone()
        mk.SetMask(bytearray(bm))
        key = sch.AggregatePublicKeys(mk)
        if ok:
            sch.Verify(key, msg, sig)
        else:
            with pytest.raises(ValueError, match="invalid signature"):
                sch.Verify(key, msg, sig)
    # TestBDN_RogueAttack: the attacker publishes x2 B - X1, so that the PLAIN sum of the two keys is x2 B and a signature
    # under x2 alone verifies under it; under the coefficients it does not
    (x1, X1), (x2, X2) = pairs[0], pairs[1]
    rogue = X2.Clone().Sub(X2, X1)
    plain = X1.Clone().Add(X1, rogue)
    assert plain.Equal(X2)
    sig = sch.Sign(x2, msgs[0])
    sch.Verify(plain, msgs[0], sig)  # the attack on plain BLS aggregation
    rmask = bdn.NewMask(key_group, [X1, rogue])
    assert list(sch.VerifyBatch(rmask, [msgs[0]], [sig], [bytes([0b11])])) == [False]
    rmask.SetMask(bytearray([0b11]))
    with pytest.raises(ValueError, match="invalid signature"):
        sch.Verify(sch.AggregatePublicKeys(rmask), msgs[0], sig)


def test_forced_slices_change_no_byte():
    """kyb_bdn_debug_set_slices, the probe's hook: every forced S gives the planned call's bytes, and 0 restores the plan"""
    G = O.BY_NAME["bn256_g1"]
    ms, wout, wcnt = tiled(G, "m17", 65)
    try:
        for S in (1, 2, 3, 1000):
            assert lib().kyb_bdn_debug_set_slices(S) == 0
            out, cnt, st = raw_aggregate(G, BC.points(G.name, "m17"), ms, 3, O.F_TRUSTED, True)
            assert (out == wout).all() and (cnt == wcnt).all() and not st.any(), S
    finally:
        lib().kyb_bdn_debug_set_slices(0)
    assert plan(65, 17) == (4, 5)
