"""The exceptional-operand MSM workloads of tests/_msm_exceptional.py do what they claim -- no GPU.  A wrong eigenvalue, a
split that does not come out equal or a workload whose buckets hold distinct points would make the GPU tests quietly run
random points: here the endomorphisms are checked against the oracles' coordinates, the adapters' splits and msm.cuh's
plan and recoding are restated, and every workload's buckets are shown to hold the equal or opposite entries it is for."""
import os
import random
import re

import pytest

from tests import _msm_exceptional as X

CSRC = X.CSRC


def _mont(header, name, p, rbits, fp2=False):
    """a constant of a generated params header (gen_consts.py: Montgomery residues x 2^rbits mod p, 32-bit words)"""
    text = open(os.path.join(CSRC, header)).read()
    body = re.search(r"static constexpr uint32_t %s\[[^=]*= \{(.*?)\};" % name, text).group(1)
    rows = re.findall(r"\{([^{}]*)\}", body) if fp2 else [body]
    vals = [sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(r.split(","))) for r in rows]
    inv = pow(2, -rbits, p)
    vals = [v * inv % p for v in vals]
    return tuple(vals) if fp2 else vals[0]


# ------------------------------------------------------------------------------------------------------ eigenvalues
def test_bls12381_g1_split_eigenvalue_is_z2():
    """(z^2 h mod r) G1 = (beta x, -y) of h G1: the point split_halves pairs with the high half"""
    from oracle import bls12381 as O

    beta = _mont("bls12381_params.h", "BETA", O.P, 390)
    assert beta != 1 and pow(beta, 3, O.P) == 1
    rng = random.Random(1)
    for h in [1, 2, O.R - 1] + [rng.randrange(1, O.R) for _ in range(3)]:
        x, y = O.g1_mul(h, O.G1_GEN)
        assert O.g1_mul(X.ADAPTERS["bls12381-g1-split"].eig[1] * h % O.R, O.G1_GEN) == (beta * x % O.P, -y % O.P)


def test_bls12381_g2_psi_eigenvalue_is_z():
    """psi(Q) = (cx conj x, cy conj y) equals (z h mod r) G2 of Q = h G2, z = -|z|: the quarters' images"""
    from oracle import bls12381 as O

    cx = _mont("bls12381_params.h", "PSI_CX", O.P, 390, fp2=True)
    cy = _mont("bls12381_params.h", "PSI_CY", O.P, 390, fp2=True)
    rng = random.Random(2)
    for h in [1, rng.randrange(1, O.R), rng.randrange(1, O.R)]:
        x, y = O.g2_mul(h, O.G2_GEN)
        psi = (O.f2_mul(O.f2_conj(x), cx), O.f2_mul(O.f2_conj(y), cy))
        assert O.g2_mul(-X.Z * h % O.R, O.G2_GEN) == psi
    ad = X.ADAPTERS["bls12381-g2-gls"]
    assert ad.eig == [pow(X.Z, i, O.R) for i in range(4)]  # |z|^i Q = (-1)^i psi^i(Q): the adapter's sign per quarter
    assert (X.Z**4 - X.Z**2 + 1) % O.R == 0  # |z|^4 = z^2 - 1 (mod r): the fold of a4


@pytest.mark.parametrize("suite", ["bn256", "bn254"])
def test_bn_glv_eigenvalue_is_lambda(suite):
    """(lambda h mod n) G1 = (beta x, y) of h G1: phi of bn_msm_glv.inc"""
    import importlib

    O = importlib.import_module("oracle." + suite)
    beta = _mont(suite + "_params.h", "BETA", O.P, 261)
    lam = X.ADAPTERS[suite + "-g1-glv"].eig[1]
    assert (lam * lam + lam + 1) % O.ORDER == 0
    rng = random.Random(3)
    for h in [1, O.ORDER - 1, rng.randrange(1, O.ORDER)]:
        x, y = O.g1_mul(h, O.G1_GEN)
        assert O.g1_mul(lam * h % O.ORDER, O.G1_GEN) == (beta * x % O.P, y)


# ---------------------------------------------------------------------------------------------------- equal pieces
def test_split_restatements_recombine():
    """each restated split gives pieces that recombine to k (mod r) through the eigenvalues -- for edge and random k"""
    rng = random.Random(4)
    for key in ("bls12381-g1-split", "bls12381-g2-gls", "bn256-g1-glv", "bn254-g1-glv"):
        ad = X.ADAPTERS[key]
        r = ad.order
        for k in [0, 1, r - 1, r, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(300)]:
            pieces = ad.pieces(k)
            assert sum(m * e for m, e in pieces) % r == k % r, (key, hex(k))
            assert all(m < 1 << ad.bits for m, _ in pieces), (key, hex(k))


@pytest.mark.parametrize("key", ["bls12381-g1-split", "bls12381-g2-gls", "bn256-g1-glv", "bn254-g1-glv"])
def test_endomorphism_scalars_split_into_equal_pieces(key):
    """k = a (z^2 + 1), a (1 + |z| + |z|^2 + |z|^3), a (1 + lambda): the adapter's split returns a in every piece"""
    ad = X.ADAPTERS[key]
    rng = random.Random(key)
    for _ in range(200):
        k, a = X.endo_scalar(ad, rng)
        assert ad.split(k) == [a] * ad.nsplit, (key, hex(k))
    if key == "bls12381-g1-split":
        assert X.bls_g1_half() == X.Z2 // 2  # the bound in the kernel is z^2 / 2: a < z^2 / 2 is not moved
        a = X.Z2 // 2
        assert X.split_bls_g1(a * (X.Z2 + 1)) == [a, a]
        assert X.split_bls_g1((a + 1) * (X.Z2 + 1)) != [a + 1, a + 1]  # one past the bound: the balancing moves it
    if key == "bls12381-g2-gls":
        a = X.Z >> 1
        assert X.split_bls_g2(a * (1 + X.Z + X.Z**2 + X.Z**3)) == [a] * 4


# ---------------------------------------------------------------------------------------------------- plan, digits
def test_plan_and_recoding_restatement():
    """make_plan's window widths at the sizes the workloads use, and recode_each's digits recombine to the scalar"""
    assert X.make_plan(2) == (3, 86) and X.make_plan(1 << 14) == (11, 24) and X.make_plan(1 << 19, 127) == (16, 8)
    assert X.make_plan((1 << 18) + 14, 127) == (15, 9) and X.make_plan(1 << 22, 63) == (16, 4)
    rng = random.Random(5)
    for c, bits in ((3, 256), (11, 256), (15, 127), (16, 63), (13, 255), (16, 128)):
        nwin = (bits + c) // c
        ks = [0, (1 << bits) - 1, 1 << (bits - 1)] + [rng.randrange(1 << bits) for _ in range(200)]
        d = X.digits(ks, c, nwin, bits)
        assert abs(d).max() <= 1 << (c - 1)
        for i, k in enumerate(ks):
            assert sum(int(d[w, i]) << (c * w) for w in range(nwin)) == k, (c, bits, hex(k))


# ------------------------------------------------------------------------------------------- what the buckets hold
def _all_workloads():
    return [(key, w) for key, ad in X.ADAPTERS.items() for w in X.workloads(ad)]


ALL = _all_workloads()


@pytest.mark.parametrize("key,w", ALL, ids=[repr(w) for _, w in ALL])
def test_workload_buckets_hold_equal_or_opposite_points(key, w):
    ad = w.ad
    r = ad.order
    assert all(0 <= k < ad.kmax for k in w.ks) and all(0 <= h < r for h in w.hs)
    if len(w.ks) > 2:
        assert len(w.ks) >= ad.min_n
    nb, eq, opp, zero = X.bucket_stats(ad, w.ks, w.hs)
    if w.claim == "onepoint":
        assert len({min(h, r - h) for h in w.hs}) == 1 and 0 not in w.hs
        assert {h for h in w.hs} == {w.hs[0], r - w.hs[0]} or len(w.ks) < 8
        if len(w.ks) >= 1000:
            # most buckets of a random +-1 walk over one point hold it twice or both ways
            assert eq + opp >= 0.5 * nb, (nb, eq, opp)
            assert opp >= 0.25 * nb, (nb, eq, opp)
    elif w.claim == "cancel":
        assert w.expected == 0
        assert zero == nb  # every bucket cancels: pieces and joins meet P and -P, the window sums are at infinity
        if w.name == "paired-inf":
            assert set(w.hs) == {0} and eq == opp == 0
        else:
            assert opp == nb and (nb > 0 or all(k % r == 0 for k in w.ks))  # the split adapters reduce k = r to (0, 0)
    elif w.claim == "extra":
        k, h = w.ks[-1], w.hs[-1]
        assert w.expected == k * h % r and h != 0
        c, nwin = X.make_plan(len(w.ks) * ad.nsplit, ad.bits)
        assert opp >= nb - ad.nsplit * nwin and nb - zero <= ad.nsplit * nwin  # only the extra input's buckets do not cancel
    elif w.claim == "equal":
        assert len(set(zip(w.ks, w.hs))) == 1
        assert eq == nb and nb > 0  # every bucket is n copies of one point
    elif w.claim == "endo-double":
        assert eq == nb and nb > 0  # every bucket the workload touches holds the shared image twice
    elif w.claim == "endo-cancel":
        assert opp == nb and nb > 0  # ... or the image and its negation
    else:
        raise AssertionError(w.claim)
    # the buckets replayed as running sums: additions really get equal or opposite operands (a bucket holding both
    # copies is not enough: the second may meet P + E P, not E P)
    adds, exc, longest = X.sequential_additions(ad, w.ks, w.hs)
    if w.name == "paired-inf":
        assert adds == exc == 0  # (see paired(): the identity inputs are the point of this one)
    elif w.name == "paired-zero" and (ad.nsplit > 1 or ad.kmax < r):
        assert adds == exc == 0 and nb == 0
    else:
        assert exc > 0, (adds, exc)
    if w.claim.startswith("endo"):
        # two entries per bucket, nothing else: the bucket's second addition doubles / cancels in either order
        assert longest == 2 and exc == nb and adds == nb


def test_every_adapter_has_every_workload_kind():
    for key, ad in X.ADAPTERS.items():
        names = {w.name for w in X.workloads(ad)}
        assert {"onepoint", "paired-plain", "paired-extra", "paired-zero", "paired-inf", "copies", "copies-alt"} <= names, key
        if ad.nsplit > 1:
            assert {"endo-double", "endo-cancel"} <= names, key
