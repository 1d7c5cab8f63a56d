"""The MSM driver's host arithmetic without a GPU: kyber_amd/csrc/msm_plan.h compiled for the CPU
(tests/msm_plan_harness.cpp).  For every shape the driver can be asked for, the split tail's schedule equals the integer
model of tests/test_msm_split_tail_model.py, every launch of the tail fits the buffer the layout gave it, the offsets are
sound, and the total workspace is what msm.cuh's run() asked for before the layout was written down once.

The layout sizes partial / folded / shift for the ONE schedule the call runs (fused or not, the bits each launch really
emits); run() used to size them for both fuse variants at once and with fold_bits bits per launch.  Totals are therefore
equal for adapters without the split tail and never larger for the others: the table at the end pins both figures."""
import ctypes as C
import os
import subprocess

import pytest

from tests import test_msm_split_tail_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CU = 256

# name: (sizeof Aff, sizeof Acc, split, bits, cmax, coop slots, split tail, fold groups, fold bits) -- the adapter it stands for
TRAITS = {
    "BlsG1": (100, 144, 2, 127, 16, 1, 1, 64, 6),       # bls12381_msm.hip BlsG1Msm: Jac<fp> of 3 x 48 B, GLV halves
    "BlsG1Plain": (100, 144, 1, 256, 16, 1, 1, 64, 6),  # bls12381_msm_plain.hip BlsG1MsmPlain
    "BlsG2": (196, 288, 1, 256, 16, 1, 1, 32, 5),       # bls12381_msm.hip BlsG2Msm: Jac<fp2> of 3 x 96 B, slots of 96 B
    "BlsG2Gls": (196, 288, 4, 63, 16, 1, 1, 32, 5),     # bls12381_msm_gls.hip BlsG2MsmGls: GLS quarters
    "BnG1": (68, 96, 1, 256, 16, 1, 1, 64, 6),          # bn_msm.inc G1Msm (bn256, bn254): Jac<fp> of 3 x 32 B
    "BnG1Glv": (68, 96, 2, 127, 16, 1, 1, 64, 6),       # bn_msm_glv.inc G1MsmGlv
    "BnG2": (132, 192, 1, 256, 16, 1, 1, 32, 5),        # bn_msm.inc G2Msm: Jac<fp2> of 3 x 64 B
    "Ed": (120, 160, 1, 256, 16, 0, 0, 32, 5),          # ed25519.hip EdMsm: ge_precomp / ge_p3, no cooperative slots
    "CoopNoSplit": (68, 96, 1, 256, 16, 1, 0, 64, 6),   # cooperative slots without the split tail (no adapter today)
}
SIZES = [1, 3, 700, 5000, 1 << 13, 1 << 17, 1 << 19, 1 << 20, 1 << 23]
BITS = [256, 128, 8]
SCAN_TILE, MAXSUB = 4096, 256


def align256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build", "libmsmplanharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "msm_plan_harness.cpp")])
    # the switches are read once per process: out of this process's environment while the harness reads them
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("KYB_MSM_")}
    try:
        assert not any(k.startswith("KYB_MSM_") for k in os.environ)
        h = C.CDLL(out)
        h.mph_names.restype = C.c_char_p
        h.mph_call.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64),
                               C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        assert h.mph_switches_set() == 0
    finally:
        os.environ.update(saved)
    return h


class Call:
    def __init__(self, h, traits, n, bits, fuse_ok=True):
        names = h.mph_names().decode().rstrip(",").split(",")
        tr = (C.c_int64 * 9)(*traits)
        plan, offs, misc, tail = (C.c_int64 * 6)(), (C.c_uint64 * (len(names) + 1))(), (C.c_int64 * 11)(), (C.c_int64 * 38)()
        h.mph_call(n, 0 if bits == 256 else bits << 16, NUM_CU, tr, int(fuse_ok), plan, offs, misc, tail)
        self.names, self.offs, self.bytes = names, list(offs)[:-1], offs[len(names)]
        self.c, self.nwin, self.nb, self.chunk, self.nchunks, self.bits = plan
        (self.nbk, self.tiles, self.two_pass, self.cb, self.tiles1, self.m1, self.sub, self.max_pieces, self.n_partial,
         self.n_fold, self.n_chains) = misc
        t = list(tail)
        self.on, self.fuse, self.lb0, self.chbits, self.tz, self.nchains, self.reduce_out, nlevels = t[:8]
        self.levels = [tuple(t[8 + 5 * i:13 + 5 * i]) for i in range(nlevels)]  # nplain, ncur, nout, lb_out, rows written
        self.folds = [tuple(t[29 + 2 * i:31 + 2 * i]) for i in range(t[28])]
        self.nlast = t[37]

    def room(self, name):
        """bytes from this buffer's offset to the next one's"""
        i = self.names.index(name)
        return (self.offs[i + 1] if i + 1 < len(self.names) else self.bytes) - self.offs[i]


def model_schedule(nwin, nchunks, chunk, FG, fuse_ok):
    """the launches split_tail() of the integer model makes: its fold_launch is replaced by a recorder for the call"""
    seen = []
    real = M.fold_launch

    def record(rows, nplain, nbits, nin, lb_out, FG_):
        out, nout = real(rows, nplain, nbits, nin, lb_out, FG_)
        seen.append((nplain, nin, nout, lb_out))
        return out, nout

    nb = nchunks * chunk
    M.fold_launch = record
    try:
        M.split_tail([[0] * nb for _ in range(nwin)], nwin, 1, nb, chunk, FG, fuse_ok)  # asserts done == chbits, nplain
    finally:
        M.fold_launch = real
    return seen


_MODEL = {}


def cases():
    return [(name, n, bits, fuse_ok) for name in TRAITS for n in SIZES for bits in BITS for fuse_ok in (True, False)]


def test_schedule_equals_the_model_and_every_launch_fits_its_buffer(harness):
    ran = 0
    for name, n, bits, fuse_ok in cases():
        tr = TRAITS[name]
        acc, FG, LB = tr[1], tr[7], tr[8]
        c = Call(harness, tr, n, bits, fuse_ok)
        tag = (name, n, bits, fuse_ok)
        assert c.nb == 1 << (c.c - 1) and c.nchunks * c.chunk == c.nb and c.nbk == c.nwin * c.nb, tag
        assert c.on == (tr[6] == 1 and c.nwin > 1), tag
        # what every tail needs: the chunk partials, the first fold level, the window sums
        assert c.n_partial >= c.nwin * c.nchunks or c.on, tag
        assert c.n_fold >= c.nwin * ((c.nchunks + 31) // 32) and c.n_chains >= c.nwin, tag
        assert c.room("partial") >= acc * c.n_partial and c.room("folded") >= acc * c.n_fold, tag
        assert c.room("shift") >= acc * c.n_chains and c.room("shift2") >= acc * ((c.n_chains + 63) // 64), tag
        assert c.room("winsum") >= acc * c.nwin, tag
        assert c.room("tile") >= 4 * ((max(c.nbk, c.m1) + SCAN_TILE - 1) // SCAN_TILE + 1), tag  # launch_scan: tiles + the total
        if not c.on:
            assert not c.levels and not c.folds, tag
            continue
        ran += 1
        key = (c.nwin, c.nchunks, c.chunk, FG, fuse_ok)
        if key not in _MODEL:
            _MODEL[key] = model_schedule(*key)
        assert [l[:4] for l in c.levels] == _MODEL[key], tag
        assert c.fuse == (fuse_ok and c.nchunks >= 16) and c.lb0 == (4 if c.fuse else 0), tag
        assert 1 << c.chbits == c.nchunks and 1 << c.tz == c.chunk, tag
        assert c.lb0 + sum(l[3] for l in c.levels) == c.chbits and c.nchains == c.nwin * (1 + c.chbits), tag
        # the reduce kernel's output, in the layout this call runs and in the other one, fits `partial` ...
        fused, plain = c.nwin * 6 * (c.nchunks // 16), 2 * c.nwin * c.nchunks
        assert c.reduce_out == (fused if c.fuse else plain) and c.reduce_out <= c.n_partial, tag
        # ... every launch of the bit tree its destination (levels 0, 2 write `folded`, level 1 `partial`) ...
        for i, (nplain, ncur, nout, lb_out, rows) in enumerate(c.levels):
            assert nout == (ncur + FG - 1) // FG and lb_out <= LB, tag
            assert rows == (nplain + c.nwin * (lb_out + 1)) * nout, tag
            assert rows <= (c.n_fold if i % 2 == 0 else c.n_partial), (tag, i)
            assert (nplain + c.nwin) * ncur <= (c.reduce_out if i == 0 else c.levels[i - 1][4]), (tag, i)  # what it reads was written
        # ... the chains `shift`, the folds over them `shift2` and `shift` in turn
        assert c.nchains <= c.n_chains, tag
        m = c.nchains
        for i, (nin, nout) in enumerate(c.folds):
            assert nin == m and nout == (nin + 2 * FG - 1) // (2 * FG), tag
            assert nout <= ((c.n_chains + 63) // 64 if i % 2 == 0 else c.n_chains), (tag, i)
            m = nout
        assert m == c.nlast and 1 <= c.nlast <= 2, tag
    assert ran > 300


def test_either_reduce_layout_fits_the_partial_buffer_sized_for_it(harness):
    """reduce_coop_kernel writes W and T rows (2 nwin nchunks) or, with its own four levels, six rows of nchunks / 16:
    whichever the switches choose, the buffer sized for the chosen one holds it, and the fused one is the smaller"""
    for name, n, bits, _ in cases():
        f, u = Call(harness, TRAITS[name], n, bits, True), Call(harness, TRAITS[name], n, bits, False)
        if f.on:
            assert f.reduce_out <= f.n_partial and u.reduce_out <= u.n_partial and f.reduce_out <= u.reduce_out


# the order run() carved the workspace in before the layout was one table
ORDER = ["aff", "digits", "sorted", "hist", "total", "mid", "ch", "offs1", "giant", "gcnt", "lenhist", "lencursor", "nlong", "bad",
         "offs", "nsub", "suboffs", "pieces", "plo", "plen", "order", "pdst", "longlist", "joinlist", "lpart", "buckets", "partial",
         "folded", "shift", "shift2", "tile", "winsum"]


def test_offsets_are_aligned_increasing_and_the_zeroed_region_is_contiguous(harness):
    for name, n, bits, fuse_ok in cases():
        c = Call(harness, TRAITS[name], n, bits, fuse_ok)
        tag = (name, n, bits, fuse_ok)
        assert c.names == ORDER and c.offs[0] == 0 and c.bytes % 256 == 0, tag
        assert all(o % 256 == 0 for o in c.offs), tag
        # never decreasing; a buffer this call does not use (the two-pass sort's in a one-pass call, lpart without
        # cooperative slots) takes no room, every other one starts strictly after its predecessor
        empty = {"mid", "ch", "giant", "gcnt"} if not c.two_pass else set()
        if not TRAITS[name][5]:
            empty.add("lpart")
        for b in c.names:
            assert (c.room(b) == 0) if b in empty else (c.room(b) > 0), (tag, b)
        assert c.offs == sorted(c.offs), tag
        z = c.names.index("lenhist")
        assert c.names[z:z + 5] == ["lenhist", "lencursor", "nlong", "bad", "offs"], tag
        assert [c.room(b) for b in c.names[z:z + 4]] == [align256(4 * (MAXSUB + 2))] * 2 + [256, 256], tag


# Total workspace bytes.  `parent`: what run() computed before the layout was one table (the sizing lines of that
# run() copied verbatim into a stand-alone program, 256 CUs, no switch set).  `new`: None where the layout gives the
# same, else its smaller figure (the tail buffers sized for the one schedule that runs).
TOTALS = [
    # adapter, n, bits, parent, new
    ("BlsG1", 1, 256, 120320, None),
    ("Ed", 1, 256, 188160, None),
    ("BlsG1", 3, 256, 123392, None),
    ("Ed", 3, 256, 190464, None),
    ("BlsG1", 700, 256, 1195008, 1178624),
    ("BlsG1Plain", 700, 256, 1286144, 1236224),
    ("BlsG2", 700, 256, 2207744, 2132992),
    ("BnG1", 700, 256, 970240, 937472),
    ("BnG2", 700, 256, 1585152, 1535232),
    ("Ed", 700, 256, 984576, None),
    ("BnG1", 700, 128, 536320, 519168),
    ("BlsG1", 5000, 256, 6329344, 6119936),
    ("BlsG2Gls", 5000, 256, 12283136, 11885312),
    ("BnG1Glv", 5000, 256, 4760832, 4620800),
    ("Ed", 5000, 256, 5237504, None),
    ("Ed", 5000, 128, 3016704, None),
    ("Ed", 5000, 8, 766976, None),
    ("BlsG1", 131072, 256, 136281856, 131713280),
    ("BlsG1Plain", 131072, 256, 129302784, 124482048),
    ("BlsG2", 131072, 256, 226861312, 216683264),
    ("BnG1", 131072, 256, 96962304, 93748480),
    ("BnG2", 131072, 256, 162001152, 155215616),
    ("Ed", 131072, 256, 106734848, None),
    ("BlsG1", 524288, 256, 387956992, 379842304),
    ("BlsG1", 1048576, 256, 620810752, 612696064),
    ("BlsG1Plain", 1048576, 256, 693481216, 684851968),
    ("BlsG2", 1048576, 256, 1099903744, 1081710080),
    ("BlsG2Gls", 1048576, 256, 1235297024, 1226741248),
    ("BnG1", 1048576, 256, 558318848, 552566016),
    ("BnG1Glv", 1048576, 256, 502537216, 497127168),
    ("BnG2", 1048576, 256, 829266944, 817137664),
    ("Ed", 1048576, 256, 623346176, None),
    ("BlsG2", 1048576, 128, 692007936, 672756992),
    ("Ed", 1048576, 128, 393474048, None),
    ("Ed", 1048576, 8, 155630336, None),
    ("BlsG1", 8388608, 256, 3078186240, 3070071552),
    ("Ed", 8388608, 256, 3144870144, None),
]


def test_total_workspace_is_pinned(harness):
    assert len(TOTALS) >= 12
    for name, n, bits, parent, new in TOTALS:
        got = Call(harness, TRAITS[name], n, bits).bytes
        if new is None:
            assert got == parent, (name, n, bits)
        else:
            assert got == new and new <= parent, (name, n, bits)


def test_total_never_exceeds_the_parent_formula_where_it_is_kept(harness):
    """adapters without the split tail keep run()'s sizing term for term: the same totals at every pinned shape"""
    assert all(new is None for name, _, _, _, new in TOTALS if name == "Ed")
    assert sum(name == "Ed" for name, *_ in TOTALS) >= 6
