"""MSM workloads whose buckets, joins and sums meet EQUAL or OPPOSITE operands (the exceptional branches of the additions:
double, or cancel to infinity and restart).  Every point is h G with a known discrete log h (0: the point at infinity), so
every workload is (scalars k_i, logs h_i) and its answer is (sum k_i h_i mod r) G -- a big-integer expectation that does
not go through the bucket pipeline.  tests/test_msm_exceptional_model.py shows on the CPU that each construction does what
it claims (the adapter's split, the digits, the buckets, restated in Python); tests/test_gpu_msm_exceptional.py and the
msmexc workload of tests/_switch_probe.py run them on the device.  No GPU needed to import this module."""
import functools
import os
import random
import re
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kyber_amd", "csrc")

Z = 0xD201000000010000  # |z|, the BLS12-381 parameter is z = -|z|
Z2 = Z * Z              # the BLS12-381 G1 split base: z^2 P = (beta x, -y)
R_BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
L_ED = 2**252 + 27742317777372353535851937790883648493


@functools.lru_cache(None)
def _bn_consts(suite):
    from tests.test_bn_glv_balance_model import _consts

    return _consts(suite + "_params.h")


def bn_lambda(suite):
    """the eigenvalue of phi(x, y) = (beta x, y) on G1, as tests/test_bn_glv_balance_model.py derives it from the lattice"""
    c = _bn_consts(suite)
    return c["GLV_A1"] * pow(c["GLV_B1N"], -1, c["ORDER"]) % c["ORDER"]


@functools.lru_cache(None)
def bls_g1_half():
    """z^2 / 2 as split_halves (bls12381_msm.hip) writes it: the bound of the balanced halves"""
    text = open(os.path.join(CSRC, "bls12381_msm.hip")).read()
    m = re.search(r"const uint32_t HALF\[5\] = \{([^}]*)\}", text)
    return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(m.group(1).split(",")))


# ---------------------------------------------------------------- the adapters' splits, restated (signed pieces)
def split_bls_g1(k):
    """bls12381_msm.hip split_halves: k = k1 z^2 + k0, both moved into (-z^2 / 2, z^2 / 2]"""
    half = bls_g1_half()
    q, r0 = divmod(k, Z2)
    if r0 > half:
        r0, q = r0 - Z2, q + 1
    for _ in range(3):
        if q > half:  # q z^2 = (q - z^2) z^2 + z^4 and z^4 = z^2 - 1 (mod r)
            q, r0 = q - Z2 + 1, r0 - 1
    return [r0, q]


def split_bls_g2(k, bits=256):
    """bls12381_msm_gls.hip BlsG2MsmGls::decode_split: quarters in (-|z| / 2, |z| / 2], the overflow of a3 folded back"""
    k &= (1 << bits) - 1
    q1, a0 = divmod(k, Z)
    q2, a1 = divmod(q1, Z)
    a3, a2 = divmod(q2, Z)
    A, H = [a0, a1, a2, a3], Z >> 1
    for i in range(3):
        if A[i] > H:
            A[i], A[i + 1] = A[i] - Z, A[i + 1] + 1
    a4 = 0
    for _ in range(4):
        if A[3] > H:
            A[3], a4 = A[3] - Z, a4 + 1
    A[2] += a4
    A[0] -= a4
    return A


def split_bn_g1(suite, k):
    """bn_msm_glv.inc decode_split: tests/test_bn_glv_balance_model.py split_balanced"""
    from tests.test_bn_glv_balance_model import split_balanced

    k1, k2, _, _ = split_balanced(_bn_consts(suite), k)
    return [k1, k2]


class Adapter:
    """One MSM adapter: how an input (k, h G) becomes pipeline entries (|piece|, +-E_i h G), and the plan it runs on.
    suite: kyber_amd.pairing module name or "ed25519"; flags: what the call passes to select the adapter."""

    def __init__(self, key, suite, group, order, eig, split, bits, flags=0, kmax=1 << 256, min_n=0):
        self.key, self.suite, self.group, self.order = key, suite, group, order
        self.eig, self.split, self.bits, self.flags, self.kmax, self.min_n = eig, split, bits, flags, kmax, min_n

    @property
    def nsplit(self):
        return len(self.eig)

    def pieces(self, k):
        """[(magnitude, discrete-log multiplier)] of the pipeline entries of (k, G) -- sign folded into the multiplier"""
        parts = self.split(k) if self.split else [k & ((1 << self.bits) - 1)]
        return [(abs(a), (e if a >= 0 else -e) % self.order) for a, e in zip(parts, self.eig)]

    def __repr__(self):
        return self.key


def _scalar_bits_flag(b):
    return (b & 0x1FF) << 16  # KYB_F_SCALAR_BITS(b)


def adapters():
    """every MSM adapter of the engine, keyed as the GPU tests parametrize them"""
    out = {
        # balanced z^2 halves (default); the plain adapter for KYB_F_SCALAR_BITS <= 160
        "bls12381-g1-split": Adapter("bls12381-g1-split", "bls12381", 1, R_BLS, [1, Z2 % R_BLS], split_bls_g1, 127),
        "bls12381-g1-plain": Adapter("bls12381-g1-plain", "bls12381", 1, R_BLS, [1], None, 128, _scalar_bits_flag(128),
                                     kmax=1 << 128),
        # GLS quarters: piece i is (-1)^i psi^i(Q) = |z|^i Q since psi = [z]
        "bls12381-g2-gls": Adapter("bls12381-g2-gls", "bls12381", 2, R_BLS, [Z**i % R_BLS for i in range(4)], split_bls_g2, 63),
        # plain windows: scalars cut at 255 bits (KYB_F_SCALAR_BITS) and more than 2^15 points
        "bls12381-g2-plain": Adapter("bls12381-g2-plain", "bls12381", 2, R_BLS, [1], None, 255, _scalar_bits_flag(255),
                                     kmax=1 << 255, min_n=(1 << 15) + 1),
        "ed25519": Adapter("ed25519", "ed25519", 0, L_ED, [1], None, 256, kmax=1 << 252),
    }
    for s in ("bn256", "bn254"):
        n = _bn_consts(s)["ORDER"]
        out[s + "-g1-glv"] = Adapter(s + "-g1-glv", s, 1, n, [1, bn_lambda(s)], lambda k, s=s: split_bn_g1(s, k), 127)
        out[s + "-g2-plain"] = Adapter(s + "-g2-plain", s, 2, n, [1], None, 256)
    return out


ADAPTERS = adapters()


# ---------------------------------------------------------------- msm_plan.h make_plan / msm.cuh recode_each, restated
def make_plan(n, bits=256, cmax=16):
    lg = n.bit_length() - 1
    c = min(max(lg - 3, 3), cmax)
    return c, (bits + c) // c  # window bits, windows (the scalar bits + the recoding carry)


def digits(mags, c, nwin, bits):
    """signed c-bit digits of every magnitude (window-major [nwin, n]), as recode_each cuts them"""
    m = np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in mags], dtype=np.uint64).reshape(-1, 4)
    half = 1 << (c - 1)
    carry = np.zeros(len(mags), dtype=np.int64)
    out = np.zeros((nwin, len(mags)), dtype=np.int64)
    for w in range(nwin):
        bit = w * c
        raw = np.zeros(len(mags), dtype=np.uint64)
        if bit < bits:
            idx, sh = bit >> 6, bit & 63
            raw = m[:, idx] >> np.uint64(sh)
            if sh + c > 64 and idx + 1 < 4:
                raw |= m[:, idx + 1] << np.uint64(64 - sh)
            raw &= np.uint64((1 << min(c, bits - bit)) - 1)
        d = raw.astype(np.int64) + carry
        carry = (d > half).astype(np.int64)
        out[w] = d - (carry << c)
    return out


def bucket_stats(ad, ks, hs):
    """The accumulate stage's input, restated: the pipeline entries of every (k_i, h_i G) -- the adapter's pieces, cut
    into signed digits -- sorted into (window, bucket).  Points are tracked as +-A with A = min(log, r - log).  Returns
    (non-empty buckets, buckets holding two equal entries, buckets holding an entry and its negation, buckets whose
    entries cancel in +- pairs: signed sum the identity).  Equal (k, h) inputs are counted once, with a multiplicity."""
    r = ad.order
    inputs = Counter(zip(ks, hs))
    n = sum(inputs.values())
    c, nwin = make_plan(max(n * ad.nsplit, 1), ad.bits)
    atoms = {0: 0}
    mags, atom, sgn, mult = [], [], [], []
    for (k, h), cnt in inputs.items():
        for mag, e in ad.pieces(k):
            lg = e * h % r
            a = min(lg, r - lg) if lg else 0
            mags.append(mag)
            atom.append(atoms.setdefault(a, len(atoms)))
            sgn.append(1 if lg == a else -1)
            mult.append(cnt)
    atom, sgn, mult = np.array(atom, dtype=np.int64), np.array(sgn, dtype=np.int64), np.array(mult, dtype=np.float64)
    na = len(atoms)
    d = digits(mags, c, nwin, ad.bits)
    w, j = np.nonzero(d)
    key = w * ((1 << (c - 1)) + 1) + np.abs(d[w, j])
    code = key * na + atom[j]
    s = sgn[j] * np.sign(d[w, j])
    live = atom[j] != 0  # entries at infinity neither double nor cancel

    def counts(sel):
        u, inv = np.unique(code[sel], return_inverse=True)
        return u, np.bincount(inv.ravel(), weights=mult[j][sel])

    up, cp = counts(live & (s > 0))
    un, cn = counts(live & (s < 0))
    eq = np.unique(np.concatenate([up[cp >= 2], un[cn >= 2]]) // na).size
    opp = np.unique(np.intersect1d(up, un) // na).size
    allc = np.union1d(up, un)
    net = np.zeros(allc.size)
    net[np.searchsorted(allc, up)] += cp
    net[np.searchsorted(allc, un)] -= cn
    nb = np.unique(key).size
    return nb, eq, opp, nb - np.unique(allc[net != 0] // na).size


def piece_len(ne, nb):
    """msm_plan.h piece_len: a bucket is accumulated in pieces of this many entries, each from infinity"""
    v = (2 * (ne // nb + 1) + 31) // 32 * 32
    return min(max(v, 64), 256)


def sequential_additions(ad, ks, hs):
    """The accumulate stage replayed as running sums: every bucket's entries in entry order (point index i, piece h at
    h n + i), cut into pieces of piece_len entries that each start from infinity.  Returns (mixed additions onto a finite
    accumulator, those whose operands are equal or opposite -- the doubling / cancelling branch, longest bucket).
    Points are tracked as +-A (A = min(log, r - log)); relations between different A are not used, so the count of
    exceptional additions is a lower bound.  The sort does not promise this order: a claim that must hold for every
    order is made on buckets of two entries."""
    r = ad.order
    n = len(ks)
    ne = n * ad.nsplit
    c, nwin = make_plan(max(ne, 1), ad.bits)
    nb = 1 << (c - 1)
    sub = piece_len(max(ne, 1), nb)
    atoms = {0: 0}
    mags, atom, sgn = [0] * ne, np.zeros(ne, dtype=np.int64), np.zeros(ne, dtype=np.int64)
    cache = {}
    for i, (k, h) in enumerate(zip(ks, hs)):
        if k not in cache:
            cache[k] = ad.pieces(k)
        for p, (mag, e) in enumerate(cache[k]):
            lg = e * h % r
            a = min(lg, r - lg) if lg else 0
            mags[p * n + i] = mag
            atom[p * n + i] = atoms.setdefault(a, len(atoms))
            sgn[p * n + i] = 1 if lg == a else -1
    d = digits(mags, c, nwin, ad.bits)
    w, e = np.nonzero(d)
    key = w * (nb + 1) + np.abs(d[w, e])
    o = np.lexsort((e, key))
    key, at, s = key[o], atom[e[o]], (sgn[e[o]] * np.sign(d[w[o], e[o]]))
    s[at == 0] = 0  # entries at infinity leave the accumulator as it is
    idx = np.arange(key.size)
    first = np.r_[True, key[1:] != key[:-1]] if key.size else np.zeros(0, dtype=bool)
    bstart = np.maximum.accumulate(np.where(first, idx, 0)) if key.size else idx
    seg_first = first | ((idx - bstart) % sub == 0)
    sstart = np.maximum.accumulate(np.where(seg_first, idx, 0)) if key.size else idx
    nonzero = np.zeros(key.size, dtype=np.int64)  # atoms with a non-zero coefficient in the accumulator before the entry
    mine = np.zeros(key.size, dtype=np.int64)     # the entry's own atom's coefficient there
    for a in range(1, len(atoms)):
        x = np.where(at == a, s, 0)
        before = np.cumsum(x) - x
        acc = before - before[sstart]
        nonzero += acc != 0
        mine += np.where(at == a, acc, 0)
    live = s != 0
    adds = int((live & (nonzero > 0)).sum())
    exc = int((live & (nonzero == 1) & (np.abs(mine) == 1)).sum())
    longest = int(np.bincount(np.cumsum(first) - 1).max()) if key.size else 0
    return adds, exc, longest


# ---------------------------------------------------------------- workloads
class Workload:
    def __init__(self, name, ad, ks, hs, claim):
        self.name, self.ad, self.ks, self.hs, self.claim = name, ad, ks, hs, claim
        self.expected = sum(k * h for k, h in zip(ks, hs)) % ad.order

    def __repr__(self):
        return "%s/%s/n=%d" % (self.ad.key, self.name, len(self.ks))


def _rng(ad, name, n):
    return random.Random("%s/%s/%d" % (ad.key, name, n))


def one_point(ad, n):
    """all n points are +-P, random signs and scalars: every bucket is a +-1 walk over multiples of P"""
    rng = _rng(ad, "onepoint", n)
    h = rng.randrange(1, ad.order)
    return Workload("onepoint", ad, [rng.randrange(ad.kmax) for _ in range(n)],
                    [h if rng.random() < 0.5 else ad.order - h for _ in range(n)], "onepoint")


def paired(ad, n, variant="plain"):
    """pairs (k, P_j), (k, -P_j) over a pool of 5 points: the MSM is the identity and so is every bucket.  variant "extra":
    one unpaired (k, P) more; "zero": every scalar 0, r, 2r or 3r (those below the adapter's scalar bound) -- on the
    adapters that split (their split reduces r to (0, 0)) and those bounded below r this only leaves every digit zero and
    every bucket empty, it cancels nothing; "inf": every point at infinity -- the accumulators only ever meet the
    identity, no addition doubles or cancels"""
    rng = _rng(ad, "paired-" + variant, n)
    pool = [rng.randrange(1, ad.order) for _ in range(5)]
    zeros = [j * ad.order for j in range(4) if j * ad.order < ad.kmax]
    ks, hs = [], []
    for i in range(n // 2):
        k = zeros[i % len(zeros)] if variant == "zero" else rng.randrange(ad.kmax)
        h = 0 if variant == "inf" else pool[i % len(pool)]
        ks += [k, k]
        hs += [h, -h % ad.order]
    if variant == "extra":
        ks.append(rng.randrange(ad.kmax))
        hs.append(rng.randrange(1, ad.order))
    return Workload("paired-" + variant, ad, ks, hs, "extra" if variant == "extra" else "cancel")


def copies(ad, n, alternate=False):
    """n copies of one (k, P): every piece and slice of every bucket is equal and their joins double; alternate: (k, P),
    (k, -P) in turn, so pieces and slices cancel or come out as +-kP depending on where they are cut"""
    rng = _rng(ad, "copies-%d" % alternate, n)
    k, h = rng.randrange(ad.kmax), rng.randrange(1, ad.order)
    hs = [h if not alternate or i % 2 == 0 else ad.order - h for i in range(n)]
    return Workload("copies-alt" if alternate else "copies", ad, [k] * n, hs, "cancel" if alternate else "equal")


def endo_scalar(ad, rng):
    """a scalar whose halves / quarters are all equal: (k, a)"""
    if ad.key == "bls12381-g1-split":
        a = rng.randrange(1, Z2 // 2)
        return a * (Z2 + 1), a
    if ad.key == "bls12381-g2-gls":
        a = rng.randrange(1, Z >> 1)
        return a * (1 + Z + Z * Z + Z**3), a
    lam = ad.eig[1]
    while True:  # short a: the balanced split of a (1 + lambda) is (a, a) -- checked, not assumed
        a = rng.randrange(1, 1 << 120)
        k = a * (1 + lam) % ad.order
        if ad.split(k) == [a, a]:
            return k, a


# bits a piece may use in the endomorphism workloads: below the adapters' balancing bounds (z^2 / 2, |z| / 2, and well
# inside the BN halves' box)
ENDO_BITS = {"bls12381-g1-split": 126, "bls12381-g2-gls": 62, "bn256-g1-glv": 120, "bn254-g1-glv": 120}


def endo(ad, m, mode):
    """m pairs whose only live pipeline entries are one endomorphism image, twice ("double") or with its negation
    ("cancel"): (a E, P) splits into (0, P), (a, E P) and (a, +-E P) into (a, E P), (0, ...), where E is what the adapter
    splits on (BLS G1: z^2; BN G1: lambda; BLS G2: (a |z|^i, Q) against (a |z|^(i-1), +-|z| Q), i = 1, 2, 3, so that quarter
    i of the first meets quarter i - 1 of the second).  Every a has a single non-zero digit, in a (window, bucket) of its
    own: each bucket holds exactly the two colliding entries, so its second addition doubles or cancels whatever order
    the sort leaves them in."""
    rng = _rng(ad, "endo-" + mode, m)
    r = ad.order
    sign = {"double": 1, "cancel": -1}[mode]
    c, _ = make_plan(2 * m * ad.nsplit, ad.bits)
    nb = 1 << (c - 1)
    wins = (ENDO_BITS[ad.key] - c) // c + 1  # windows where every digit up to nb fits below the bound
    slots = [(w, d) for w in range(wins) for d in range(1, nb + 1)]
    assert len(slots) >= m, (ad, m)
    rng.shuffle(slots)
    ks, hs = [], []
    for j in range(m):
        w, d = slots[j]
        a = d << (c * w)
        h = rng.randrange(1, r)
        if ad.group == 2:
            i = 1 + j % 3
            ks += [a * Z**i, a * Z ** (i - 1)]
            hs += [h, sign * Z * h % r]
        else:
            e = ad.eig[1]
            ks += [a * e % r if ad.suite != "bls12381" else a * Z2, a]
            hs += [h, sign * e * h % r]
    return Workload("endo-" + mode, ad, ks, hs, "endo-" + mode)


def scalar_bytes(ad, ks):
    """32-byte scalars as the adapter's ABI reads them (big-endian; Ed25519 little-endian)"""
    order = "little" if ad.suite == "ed25519" else "big"
    return np.frombuffer(b"".join(k.to_bytes(32, order) for k in ks), dtype=np.uint8).reshape(len(ks), 32).copy()


def onepoint_sizes(ad):
    """from 2 up past the planner switches (test_gpu_full_size.py test_msm_across_the_planner_thresholds): the window
    width steps with log2 n, four fused tree levels from 16 chunks, a second fold launch from 2^10 chunks, the two-pass
    sort from 2^19 entries per window; the G1 adapters on halves up to 2^18 + 7 inputs (2^19 + 14 halves: the two-pass
    sort and the split tail with fused levels), G2 up to 16 391"""
    if ad.min_n:
        return [ad.min_n + 6]
    sizes = [2, 3, 17, 65, 257, 1025, 4097, 16391]
    if ad.group == 1 and ad.nsplit == 2:
        sizes += [65537, (1 << 18) + 7]
    elif ad.group != 2:
        sizes += [65537]
    return sizes


def workloads(ad):
    """every workload of one adapter (the GPU test runs each; the model test checks each)"""
    big = ad.min_n or 0
    out = [one_point(ad, n) for n in onepoint_sizes(ad)]
    for n in ([big + 2] if big else [2, 40, 3000]):
        out += [paired(ad, n), paired(ad, n, "extra")]
    out += [paired(ad, big + 8 if big else 40, "zero"), paired(ad, big + 8 if big else 40, "inf")]
    nc = max(3000, big + 1)  # even: copies-alt pairs every (k, P) with a (k, -P)
    out += [copies(ad, nc), copies(ad, nc, True)]
    if ad.key == "bls12381-g1-split":
        out += [copies(ad, 1 << 18), copies(ad, 1 << 18, True)]  # the msmgiant shape: 2^19 / 2 copies
    if ad.nsplit > 1:
        for m in (16, 1500):
            out += [endo(ad, m, "double"), endo(ad, m, "cancel")]
    return out
