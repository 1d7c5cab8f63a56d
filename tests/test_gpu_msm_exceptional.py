"""The MSM on colliding, opposite and cancelling operands (tests/_msm_exceptional.py): one point +-P under random scalars,
pairs (k, P), (k, -P), long and giant buckets of one (k, P), inputs that meet their own endomorphism image, points at
infinity -- on every adapter, host buffers and device tensors, in every BLS12-381 input convention.  Each result must be
(sum k_i h_i mod r) G, computed with big integers and one fixed-base Commit, and for n <= 64 also the oracle's
N x (Mul + Add).  Then the multi-device combine of equal and opposite partials, and batched PubPoly.Eval whose Horner
steps double, cancel or meet the identity."""
import importlib

import numpy as np
import pytest

from tests import _msm_exceptional as X

pytestmark = pytest.mark.gpu


def _lib(ad):
    return importlib.import_module("kyber_amd.group.edwards25519" if ad.suite == "ed25519" else "kyber_amd.pairing." + ad.suite)


def _oracle(ad):
    """(mul(k, P), add(P, Q), encode(P), G, identity) of the oracle of the adapter's group"""
    if ad.suite == "ed25519":
        from oracle import ed25519 as O

        return O.mul_int, O.add, O.encode, O.B, O.IDENTITY
    O = importlib.import_module("oracle." + ad.suite)
    g = "g%d_" % ad.group
    enc = getattr(O, g + ("compress" if ad.suite == "bls12381" else "marshal"))
    return (lambda k, p: getattr(O, g + "mul")(k, p)), getattr(O, g + "add"), enc, getattr(O, "G%d_GEN" % ad.group), None


def _commit(ad, logs, flags=0):
    """rows log * G (0: the point at infinity) through the engine's fixed-base Commit; flags: F_UNCOMPRESSED_OUT"""
    m = _lib(ad)
    sc = X.scalar_bytes(ad, logs)
    if ad.suite == "ed25519":
        return np.asarray(m.batch_mul_base(sc))
    out, st = (m.g1_commit if ad.group == 1 else m.g2_commit)(sc, None, flags)
    assert not np.asarray(st).any()
    return np.asarray(out)


def _points(ad, hs, flags=0):
    """the workload's points: each distinct log committed once, the rows gathered"""
    uniq, inv = np.unique(np.array([str(h) for h in hs]), return_inverse=True)
    rows = _commit(ad, [int(u) for u in uniq], flags)
    return rows[inv.ravel()].copy()


def _msm(ad, sc, pts, flags):
    m = _lib(ad)
    if ad.suite == "ed25519":
        return m.msm(sc, pts)
    return (m.g1_msm if ad.group == 1 else m.g2_msm)(sc, pts, flags)


def _expected(ad, w):
    """(sum k_i h_i mod r) G; for n <= 64 checked against the oracle's N x (Mul + Add) of the same inputs"""
    exp = bytes(_commit(ad, [w.expected])[0])
    mul, add, enc, gen, acc = _oracle(ad)
    if w.expected == 0:
        assert exp == enc(acc)  # the identity encoding: Commit agrees with the oracle
    if len(w.ks) <= 64:
        pts = {}
        for k, h in zip(w.ks, w.hs):
            if h not in pts:
                pts[h] = mul(h, gen)
            acc = add(acc, mul(k, pts[h]))
        assert enc(acc) == exp, w
    return exp


ALL = [w for ad in X.ADAPTERS.values() for w in X.workloads(ad)]


@pytest.mark.parametrize("w", ALL, ids=[repr(w) for w in ALL])
def test_msm_exceptional_operands(w):
    """host buffers with the adapter's flags, then the _dev entry point on device tensors (vouched-for points)"""
    import torch

    ad = w.ad
    m = _lib(ad)
    exp = _expected(ad, w)
    sc, pts = X.scalar_bytes(ad, w.ks), _points(ad, w.hs)
    out, st = _msm(ad, sc, pts, ad.flags)
    assert not np.asarray(st).any() and bytes(np.asarray(out)) == exp, (w, "host")
    trusted = 0 if ad.suite == "ed25519" else m.F_TRUSTED(0)
    out, st = _msm(ad, torch.from_numpy(sc).cuda(), torch.from_numpy(pts).cuda(), ad.flags | trusted)
    torch.cuda.synchronize()
    assert not st.any().item() and bytes(out.cpu().numpy()) == exp, (w, "dev")


BLS_CONV = [w for w in ALL if w.ad.suite == "bls12381" and w.name in ("onepoint", "paired-plain", "paired-extra")
            and len(w.ks) in (17, 40, 41, 1025, 3000, 3001, 65537, (1 << 15) + 2, (1 << 15) + 3, (1 << 15) + 7)]


@pytest.mark.parametrize("w", BLS_CONV, ids=[repr(w) for w in BLS_CONV])
def test_bls12381_msm_exceptional_operands_every_convention(w):
    """checked, F_TRUSTED(0), F_UNCOMPRESSED and both: the full and the light decode kernels feed the pipeline"""
    import torch

    from kyber_amd.pairing import bls12381 as B

    ad = w.ad
    exp = _expected(ad, w)
    sc = X.scalar_bytes(ad, w.ks)
    comp, unc = _points(ad, w.hs), _points(ad, w.hs, B.F_UNCOMPRESSED_OUT)
    for pts, fl in ((comp, 0), (comp, B.F_TRUSTED(0)), (unc, B.F_UNCOMPRESSED), (unc, B.F_UNCOMPRESSED | B.F_TRUSTED(0))):
        out, st = _msm(ad, sc, pts, ad.flags | fl)
        assert not np.asarray(st).any() and bytes(np.asarray(out)) == exp, (w, fl, "host")
        out, st = _msm(ad, torch.from_numpy(sc).cuda(), torch.from_numpy(pts).cuda(), ad.flags | fl)
        torch.cuda.synchronize()
        assert not st.any().item() and bytes(out.cpu().numpy()) == exp, (w, fl, "dev")


# ----------------------------------------------------------------------------------------- the multi-device combine
COMBINE = ["bls12381-g1-split", "bls12381-g2-gls", "bn256-g1-glv", "bn256-g2-plain", "bn254-g1-glv", "ed25519"]


@pytest.mark.parametrize("key", COMBINE)
@pytest.mark.parametrize("mode", ["double", "cancel"])
def test_msm_multi_device_combine_of_equal_and_opposite_partials(key, mode):
    """two shards on device 0: the second shard equal to the first (the combine adds two equal partials) or the first
    with its points negated (the combine adds P and -P: the identity)"""
    import random

    from kyber_amd import devices

    ad = X.ADAPTERS[key]
    r = ad.order
    n = 6000
    rng = random.Random(key + mode)
    half = n // 2
    ks = [rng.randrange(ad.kmax) for _ in range(half)]
    hs = [rng.randrange(1, r) for _ in range(half)]
    ks, hs = ks + ks, hs + (hs if mode == "double" else [r - h for h in hs])
    w = X.Workload("combine-" + mode, ad, ks, hs, mode)
    assert w.expected == (0 if mode == "cancel" else 2 * sum(k * h for k, h in zip(ks[:half], hs[:half])) % r)
    exp = _expected(ad, w)
    sc, pts = X.scalar_bytes(ad, ks), _points(ad, hs)
    devices.set_devices([0, 0])
    devices.set_shard_threshold(1024)
    try:
        assert devices.shard_range(n, 0, 2) == (0, half) and devices.shard_range(n, 1, 2) == (half, n)
        out, st = _msm(ad, sc, pts, ad.flags)
    finally:
        devices.set_devices([])
        devices.set_shard_threshold(16384)
    assert not np.asarray(st).any() and bytes(np.asarray(out)) == exp


# ----------------------------------------------------------------------------------------- batched PubPoly.Eval
POLY = ["bls12381-g1-split", "bls12381-g2-gls", "bn256-g1-glv", "bn256-g2-plain", "bn254-g1-glv", "bn254-g2-plain", "ed25519"]
# the kind of every Horner step from the top: "rand" a random coefficient; at x0, "cancel" c_j = -v_{j+1} x0 (the step
# meets its negation), "double" c_j = v_{j+1} x0 (the step meets itself), "zero" an identity commitment
STEPS = {
    "cancel": ["rand", "cancel", "rand", "rand", "cancel", "cancel", "rand", "cancel", "rand", "rand"],
    "double": ["rand", "double", "double", "rand", "double", "cancel", "double", "rand", "double", "rand"],
    "root": ["rand", "double", "rand", "cancel", "rand", "rand", "double", "rand", "rand", "cancel"],
    "identity": ["zero", "zero", "rand", "rand", "zero", "zero", "rand", "double", "zero", "rand"],
}


def _horner(coeffs, x, r):
    v = 0
    for c in reversed(coeffs):
        v = (v * x + c) % r
    return v


@pytest.mark.parametrize("key", POLY)
@pytest.mark.parametrize("case,x0", [("cancel", 7), ("double", 3), ("root", 1 << 32), ("identity", 12345)])
def test_poly_eval_steps_that_double_cancel_or_meet_the_identity(key, case, x0):
    """poly_eval_kernel: commitments c_j G chosen from the scalar Horner values v_j = v_{j+1} x0 + c_j (mod r) so that at
    x0 the mixed addition of a step gets the accumulator's negation or the accumulator itself, the polynomial has a root
    at x0, or identity commitments sit at the top and in the middle; other indices see ordinary steps"""
    import random

    ad = X.ADAPTERS[key]
    r = ad.order
    m = _lib(ad)
    rng = random.Random("%s/%s" % (key, case))
    top = 0 if STEPS[case][0] == "zero" else rng.randrange(1, r)
    coeffs, v = [top], top
    for kind in STEPS[case][1:]:
        c = {"rand": rng.randrange(1, r), "cancel": -v * x0 % r, "double": v * x0 % r, "zero": 0}[kind]
        coeffs.append(c)
        v = (v * x0 + c) % r
    coeffs = coeffs[::-1]  # coeffs[j] multiplies x^j
    assert (_horner(coeffs, x0, r) == 0) == (case in ("cancel", "root") and STEPS[case][-1] == "cancel")
    idx = [x0 - 1, 0, 1, 6, 1000, (1 << 32) - 1]
    want = _commit(ad, [_horner(coeffs, i + 1, r) for i in idx])
    commits = _commit(ad, coeffs)
    if ad.suite == "ed25519":
        out, st = m.poly_eval(commits, idx)
        sv = m.scalar_poly_eval(X.scalar_bytes(ad, coeffs), idx[:3])
    else:
        out, st = m.ENGINE.poly_eval(ad.group, commits, idx)
        sv = m.ENGINE.scalar_poly_eval(X.scalar_bytes(ad, coeffs), idx[:3])
    assert not np.asarray(st).any()
    assert [bytes(o) for o in np.asarray(out)] == [bytes(o) for o in want], (key, case)
    assert bytes(np.asarray(sv)) == bytes(X.scalar_bytes(ad, [_horner(coeffs, i + 1, r) for i in idx[:3]]))
    if case == "root":
        mul, add, enc, gen, ident = _oracle(ad)
        assert bytes(np.asarray(out)[0]) == enc(ident)
