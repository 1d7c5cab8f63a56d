"""Every Ed25519 host entry that takes a batch of variable-length elements, called with off[0] != 0: three elements, the
first one empty, three stray bytes of 0x5a in front of it.  The entry rebases the offsets and uploads the bytes from
off[0] on (kyber_amd/csrc/ed_spans.h), so a slip there moves every element and nothing else notices.  Each entry's
result must be byte-equal to the same call without the stray bytes, and to the oracle its own GPU test uses.

The entries come from the `const uint64_t *` parameters of include/kyber_hip.h.  The three that
tests/test_gpu_vss_engine.py already calls this way (schnorr_sign, vss_seal, vss_open) are named in COVERED; every other
one has a case here, and a new entry with offsets fails the enumeration until it has one too.  A seal's or an open's
output lies at the input's offsets (plus the elements' overhead): it is given `lead` bytes more, which must come back
untouched, and what lies behind them must be the other call's output."""
import hashlib
import os
import re

import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _cosi_cases as CC
from tests import _dkg_cases as DC
from tests import _anon_enc_oracle as AE
from tests import _dss_oracle as D
from tests import _ecies_oracle as EC
from tests import _eddsa_oracle as EO
from tests import _shard_cases as T
from tests.test_proof_host import fs_challenge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAD = 3
COVERED = {"kyb_ed25519_schnorr_sign", "kyb_ed25519_vss_seal", "kyb_ed25519_vss_open"}


def pack(msgs, lead):
    """(blob, off): the elements behind `lead` stray bytes, off[0] = lead"""
    assert len(msgs) == 3 and msgs[0] == b"" and msgs[1] and msgs[2]
    off = np.zeros(4, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    return np.frombuffer(b"\x5a" * lead + b"".join(msgs), dtype=np.uint8).copy(), off + np.uint64(lead)


def arr(b, dtype=np.uint8):
    return np.frombuffer(b, dtype=dtype).copy() if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b, dtype=dtype)


def both(entry, msgs, args, outs, displaced=()):
    """entry(*args) twice, without the stray bytes and with them; args() takes (blob pointer, off pointer) and the output
    arrays.  Returns the outputs of the call with the lead after holding them to the other's.  displaced: the indices of
    the flat byte outputs that lie at the input's offsets; they are `lead` bytes longer, and come back without them."""
    got = []
    for lead in (0, LEAD):
        blob, off = pack(msgs, lead)
        out = [np.full(shape[0] + lead if k in displaced else shape, 0xEE, dtype=dt) for k, (shape, dt) in enumerate(outs)]
        _lib.check(getattr(_lib.load(), entry)(*args(blob.ctypes.data, off.ctypes.data, *(o.ctypes.data for o in out))), entry)
        for k in displaced:
            assert (out[k][:lead] == 0xEE).all(), (entry, "bytes in front of the first element were written")
            out[k] = out[k][lead:]
        got.append(out)
    for plain, led in zip(*got):
        assert plain.tobytes() == led.tobytes(), entry
    return got[1]


# -------------------------------------------------------------------------- entries with a row in tests/_shard_cases.py
def shard_row(name):
    """the row at n = 3 on one device: its first message is empty already (msg_lengths); the table is the oracle"""
    from tests.test_gpu_sharded_entries import _against_the_table, _call

    case = T.build(name, 3, 1)
    at = next(k for k, a in enumerate(case.args) if isinstance(a, np.ndarray) and a.dtype == np.uint64)
    blob, off = case.args[at - 1], case.args[at]
    assert off[0] == 0 and off[1] == 0 and off[2] > 0 and off[3] > off[2]
    plain = _call(case)
    case.args[at - 1] = np.concatenate([np.full(LEAD, 0x5A, dtype=np.uint8), blob[:int(off[3])]])
    case.args[at] = off + np.uint64(LEAD)
    led = _call(case)
    for o in case.outs():
        assert plain[o.name].tobytes() == led[o.name].tobytes(), (name, o.name)
    _against_the_table(case, led, name)
    return case, led


def case_verify():
    case, led = shard_row("ed25519/verify/messages")
    assert led["ok"][1] == 1  # the one row nothing is planted in: its message was found


def case_ring_chain():
    case, led = shard_row("ed25519/ring_chain/one ring/no start/c_zero/unlinkable")
    assert led["ok"][2] == 1 and 2 not in case.planted  # the oracle's signature over the last message verifies


def case_ring_challenge():
    shard_row("ed25519/ring_challenge/linkable")


# ------------------------------------------------------------------------------------------- entries with their own oracle
def case_eddsa_sign():
    _, _, msgs, _ = EO.sign_input()
    secrets, prefixes, pubs = (np.ascontiguousarray(x[5:8]) for x in EO.sign_input_keys())
    ms = [b"", msgs[5], msgs[40]]
    sigs, st = both("kyb_ed25519_eddsa_sign", ms,
                    lambda blob, off, sigs, st: (3, secrets.ctypes.data, prefixes.ctypes.data, pubs.ctypes.data, 32, blob, off, sigs, st),
                    [((3, 64), np.uint8), ((3,), np.uint8)])
    assert not st.any()
    assert [bytes(s) for s in sigs] == [EO.sign(bytes(secrets[i]), bytes(prefixes[i]), bytes(pubs[i]), ms[i]) for i in range(3)]


def case_cosi_verify():
    name, m = "5", 5
    rows, exp = CC.rows(name), CC.expected(name)
    pick = [next(k for k, r in enumerate(rows) if r.label == label) for label in ("msg-len/0", "msg-len/47", "msg-len/65")]
    rs, ex = [rows[k] for k in pick], [exp[k] for k in pick]
    roster, sigs, masks = CC.pack_roster(name), CC.pack_sigs(rs), CC.pack_masks(rs, m, 1)
    ok, agg, cnt, st = both("kyb_ed25519_cosi_verify", [r.msg for r in rs],
                            lambda blob, off, ok, agg, cnt, st: (3, m, roster.ctypes.data, blob, off, sigs.ctypes.data, masks.ctypes.data, 1,
                                                                 agg, cnt, ok, st, 0),
                            [((3,), np.uint8), ((3, 32), np.uint8), ((3,), np.uint32), ((3,), np.uint8)])
    assert [(int(ok[i]), bytes(agg[i]), int(cnt[i]), int(st[i])) for i in range(3)] == [tuple(e) for e in ex]
    assert ok.all()


class DssWorld:
    """three participants, tl = tr = 2, three sessions: the first signs the empty message"""
    NP, T, NS = 3, 2, 3

    def __init__(self):
        tag = b"leading offset dss"
        self.privs = [DC.scalar(tag + b" priv %d" % i) for i in range(self.NP)]
        self.pubs = [O.mul_base(DC.le(x)) for x in self.privs]
        self.long = [DC.scalar(tag + b" long %d" % k) for k in range(self.T)]
        self.rand = [[DC.scalar(tag + b" rand %d %d" % (b, k)) for k in range(self.T)] for b in range(self.NS)]
        self.lc = [O.mul_base(DC.le(c)) for c in self.long]
        self.rc = [[O.mul_base(DC.le(c)) for c in row] for row in self.rand]
        self.msgs = [b"", b"session one", b"the third session's message, longer than a SHA-512 block's worth of bytes " * 2]
        self.signer = 1
        self.k = [DC.le(DC.scalar(tag + b" nonce %d" % b)) for b in range(self.NS)]

    def partial_args(self):
        i = self.signer
        return (DC.le(self.privs[i]), DC.le(DC.eval_scalar(self.long, i)),
                b"".join(DC.le(DC.eval_scalar(self.rand[b], i)) for b in range(self.NS)), b"".join(self.k))

    def partials(self):
        """(V, sid, sig) of every session, from the oracle"""
        priv, alpha, beta, k = self.partial_args()
        return [D.partial(priv, self.signer, alpha, beta[32 * b:32 * b + 32], k[32 * b:32 * b + 32], self.lc, self.rc[b], self.msgs[b])
                for b in range(self.NS)]


@pytest.fixture(scope="module")
def dss_world():
    return DssWorld()


def case_dss_partial(w):
    priv, alpha, beta, k = (arr(x) for x in w.partial_args())
    lc, rc = arr(b"".join(w.lc)), arr(b"".join(b"".join(r) for r in w.rc))
    V, sid, sigs = both("kyb_ed25519_dss_partial", w.msgs,
                        lambda blob, off, V, sid, sigs: (w.NS, priv.ctypes.data, w.signer, alpha.ctypes.data, beta.ctypes.data, k.ctypes.data,
                                                         w.T, lc.ctypes.data, w.T, rc.ctypes.data, blob, off, V, sid, sigs),
                        [((3, 32), np.uint8), ((3, 32), np.uint8), ((3, 64), np.uint8)])
    assert [(bytes(V[b]), bytes(sid[b]), bytes(sigs[b])) for b in range(3)] == [tuple(p) for p in w.partials()]


def case_dss_check(w):
    """a partial of every session, all honest -- each passes only under its own session's message -- and a fourth one,
    session 1's with its share moved"""
    parts = w.partials()
    parts.append((DC.le((int.from_bytes(parts[1][0], "little") + 1) % O.L),) + tuple(parts[1][1:]))
    n = len(parts)
    pk, lc, rc = arr(b"".join(w.pubs)), arr(b"".join(w.lc)), arr(b"".join(b"".join(r) for r in w.rc))
    sess, idx = np.array([0, 1, 2, 1], dtype=np.uint32), np.full(n, w.signer, dtype=np.uint32)
    V, sid, sigs = (arr(b"".join(p[j] for p in parts)) for j in range(3))
    ok, st, sst = both("kyb_ed25519_dss_check", w.msgs,
                       lambda blob, off, ok, st, sst: (n, w.NP, pk.ctypes.data, w.T, lc.ctypes.data, w.NS, w.T, rc.ctypes.data, blob, off,
                                                       sess.ctypes.data, idx.ctypes.data, V.ctypes.data, sid.ctypes.data, sigs.ctypes.data,
                                                       ok, st, sst),
                       [((n,), np.uint8), ((n,), np.uint8), ((w.NS,), np.uint8)])
    want = [D.check(w.pubs, w.lc, w.rc[b], w.msgs[b], w.signer, *parts[j]) for j, b in enumerate(sess)]
    assert [(int(ok[j]), int(st[j])) for j in range(n)] == [tuple(x) for x in want] and not sst.any()
    assert list(ok) == [1, 1, 1, 0]


def case_fs_challenge():
    names = [b"", b"a proof's name", bytes(range(130))]
    data = arr(bytes((11 * t + 5) & 0xFF for t in range(3 * 96))).reshape(3, 96)
    c, st = both("kyb_ed25519_fs_challenge", names,
                 lambda blob, off, c, st: (3, blob, off, 0, data.ctypes.data, 96, c, st), [((3, 32), np.uint8), ((3,), np.uint8)])
    assert not st.any() and [bytes(x) for x in c] == [fs_challenge(nm, data[i].tobytes()) for i, nm in enumerate(names)]


def slots(flat, lens):
    """the elements of a flat output, of the given lengths, one behind the other"""
    ends = np.cumsum([0] + list(lens))
    assert len(flat) == ends[-1]
    return [bytes(flat[ends[i]:ends[i + 1]]) for i in range(len(lens))]


class EciesWorld:
    """three recipients; the first message is empty, and so is the first ciphertext handed to an open"""

    def __init__(self):
        self.r, self.x = (arr(hashlib.shake_256(b"leading offset ecies " + t).digest(96)).reshape(3, 32) for t in (b"r", b"x"))
        self.r[:, 31] &= 0x0F
        self.x[:, 31] &= 0x0F
        self.pubs = arr(b"".join(O.mul_base(bytes(x)) for x in self.x)).reshape(3, 32)
        self.msgs = [b"", b"seventeen bytes!!", bytes(range(70))]
        self.sealed = [EC.encrypt(bytes(self.r[i]), bytes(self.pubs[i]), m) for i, m in enumerate(self.msgs)]


def case_ecies_seal():
    w = EciesWorld()
    total = sum(len(c) for c in w.sealed)
    out, st = both("kyb_ed25519_ecies_seal", w.msgs,
                   lambda blob, off, out, st: (3, w.r.ctypes.data, w.pubs.ctypes.data, 32, blob, off, out, st),
                   [((total,), np.uint8), ((3,), np.uint8)], displaced={0})
    assert not st.any() and slots(out, [len(c) for c in w.sealed]) == w.sealed


def case_ecies_open():
    w = EciesWorld()
    cts = [b""] + w.sealed[1:]  # an element of no bytes is too short to open: its status, and a slot of no bytes
    want = [EC.decrypt(bytes(w.x[i]), c) for i, c in enumerate(cts)]
    assert [code for _, code in want] == [_lib.ST_ECIES_SHORT, 0, 0] and [m for m, _ in want[1:]] == w.msgs[1:]
    out, st = both("kyb_ed25519_ecies_open", cts,
                   lambda blob, off, out, st: (3, w.x.ctypes.data, 32, blob, off, out, st),
                   [((sum(len(c) for c in cts),), np.uint8), ((3,), np.uint8)], displaced={0})
    assert [int(s) for s in st] == [code for _, code in want]
    assert slots(out, [len(c) for c in cts]) == [(m or b"").ljust(len(c), b"\0") for (m, _), c in zip(want, cts)]


class AnonWorld:
    """one anonymity set of three keys for the batch, the receiver its middle member"""
    RING, MINE = 3, 1

    def __init__(self):
        pairs = [AE.keypair("leading offset/%d" % k) for k in range(self.RING)]
        self.keys, self.priv = [P for _, P in pairs], pairs[self.MINE][0]
        self.x = [AE.reduced(AE._rng_bytes("leading offset/x/%d" % i, 32)) for i in range(3)]  # (seal's edges: test_gpu_anon_enc.py)
        self.msgs = [b"", b"abc", bytes(range(130))]
        self.sealed = [AE.seal(m, self.keys, x) for m, x in zip(self.msgs, self.x)]


def case_anon_seal():
    w = AnonWorld()
    assert [st for _, st in w.sealed] == [0, 0, 0]
    keys, x = arr(b"".join(w.keys)), arr(b"".join(w.x))
    out, st = both("kyb_ed25519_anon_seal", w.msgs,
                   lambda blob, off, out, st: (3, w.RING, keys.ctypes.data, 0, x.ctypes.data, blob, off, out, st),
                   [((sum(len(c) for c, _ in w.sealed),), np.uint8), ((3,), np.uint8)], displaced={0})
    assert not st.any() and slots(out, [len(c) for c, _ in w.sealed]) == [c for c, _ in w.sealed]


def case_anon_open():
    w = AnonWorld()
    cts = [b""] + [c for c, _ in w.sealed[1:]]  # an element of no bytes: "ciphertext too short", a slot of no bytes
    want = [AE.open_(c, w.keys, w.MINE, w.priv) for c in cts]
    assert [code for _, code in want] == [AE.ST_SHORT, 0, 0] and [m for m, _ in want[1:]] == w.msgs[1:]
    keys, priv, mine = arr(b"".join(w.keys)), arr(w.priv), np.full(3, w.MINE, dtype=np.uint32)
    out, st = both("kyb_ed25519_anon_open", cts,
                   lambda blob, off, out, st: (3, w.RING, keys.ctypes.data, 0, mine.ctypes.data, priv.ctypes.data, 0, blob, off, out, st),
                   [((sum(len(c) for c in cts),), np.uint8), ((3,), np.uint8)], displaced={0})
    assert [int(s) for s in st] == [code for _, code in want]
    assert slots(out, [len(c) for c in cts]) == [(m or b"").ljust(len(c), b"\0") for (m, _), c in zip(want, cts)]


CASES = {"kyb_ed25519_verify": case_verify, "kyb_ed25519_ring_chain": case_ring_chain, "kyb_ed25519_ring_challenge": case_ring_challenge,
         "kyb_ed25519_eddsa_sign": case_eddsa_sign, "kyb_ed25519_cosi_verify": case_cosi_verify, "kyb_ed25519_dss_partial": case_dss_partial,
         "kyb_ed25519_dss_check": case_dss_check, "kyb_ed25519_fs_challenge": case_fs_challenge, "kyb_ed25519_ecies_seal": case_ecies_seal,
         "kyb_ed25519_ecies_open": case_ecies_open, "kyb_ed25519_anon_seal": case_anon_seal, "kyb_ed25519_anon_open": case_anon_open}


def test_every_host_entry_with_offsets_is_covered_or_has_a_case():
    header = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    entries = set(re.findall(r"\bint (kyb_ed25519_\w+)\([^;{]*?const uint64_t \*", header))
    assert COVERED <= entries and not COVERED & set(CASES)
    assert entries - COVERED == set(CASES), entries ^ (COVERED | set(CASES))
    assert {"kyb_ed25519_verify", "kyb_ed25519_ring_chain", "kyb_ed25519_ring_challenge", "kyb_ed25519_eddsa_sign", "kyb_ed25519_dss_check",
            "kyb_ed25519_dss_partial", "kyb_ed25519_cosi_verify"} <= set(CASES)


@pytest.mark.parametrize("entry", sorted(CASES))
def test_three_stray_bytes_in_front_of_an_empty_first_element(entry, dss_world):
    case = CASES[entry]
    if "dss" in entry:
        case(dss_world)
    else:
        case()
