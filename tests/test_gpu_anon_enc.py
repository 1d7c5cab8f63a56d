"""kyb_ed25519_anon_seal / _open on the GPU, through the host entries and the _dev entries, byte for byte against the
sequential restatement tests/_anon_enc_oracle.py on the labelled cases of tests/_anon_enc_cases.py: the two ciphertexts
the reference prints, every message length of the hash's block edges, rings of 1, 3 and 27 (135 lanes: a block edge
inside an element), 1 024 and 1 028 points (the encoder's span edge), one set or one per element, one receiver or one
per element, receivers first, middle and last; Decrypt's rejects one by one between valid neighbours; seal's own edges
and the scalar reduction; sign/anon's Encrypt / Decrypt and their batch forms on top."""
import json
import os

import numpy as np
import pytest

from kyber_amd import _lib
from kyber_amd.util import blake2xb
from tests import _anon_enc_cases as AC
from tests import _anon_enc_oracle as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "anon_enc_examples.json")))["examples"]
SPACES = ("host", "dev")


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _rows(sets, n):
    shared = not isinstance(sets[0], (list, tuple))
    ring = len(sets) if shared else len(sets[0])
    raw = b"".join(sets) if shared else b"".join(b"".join(s) for s in sets)
    return np.frombuffer(raw, dtype=np.uint8).reshape(1 if shared else n, 32 * ring)


def _to_dev(msgs, lead: int):
    """(blob, offsets) on the device, `lead` stray bytes in front: the elements lie at odd addresses"""
    import torch

    off = np.zeros(len(msgs) + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += lead
    blob = np.frombuffer(b"\xa5" * lead + b"".join(msgs) or b"\0", dtype=np.uint8)
    return torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(off).cuda()


def _from_dev(blob, off, n):
    raw, o = blob.cpu().numpy().tobytes(), off.cpu().numpy()
    return [raw[int(o[i]):int(o[i + 1])] for i in range(n)]


def seal(ed, space, ring, sets, xs, msgs):
    n = len(msgs)
    keys, x = _rows(sets, n), np.frombuffer(b"".join(xs), dtype=np.uint8).reshape(n, 32)
    if space == "host":
        out, st = ed.batch_anon_seal(keys, x, msgs, ring)
        return out, [int(s) for s in st]
    import torch

    (blob, off), st = ed.batch_anon_seal(torch.from_numpy(keys.copy()).cuda(), torch.from_numpy(x.copy()).cuda(), _to_dev(msgs, 3), ring)
    torch.cuda.synchronize()
    return _from_dev(blob, off, n), [int(s) for s in st.cpu().numpy()]


def open_(ed, space, ring, sets, mine, privs, cts):
    """the n output slots, each as long as its ciphertext, and the statuses"""
    n = len(cts)
    keys = _rows(sets, n)
    one = not isinstance(privs, (list, tuple))
    p = np.frombuffer(privs if one else b"".join(privs), dtype=np.uint8).reshape(-1, 32)
    if space == "host":
        # (the Python wrapper hands back plaintexts; the raw slots are read through the C entry for the zero check)
        import ctypes as C

        lib = _lib.load()
        blob = np.frombuffer(b"\xa5" + b"".join(cts), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(c) for c in cts], out=off[1:])
        off += np.uint64(1)
        out, st = np.full(int(off[-1]), 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
        m = np.asarray(mine, dtype=np.uint32)
        rc = lib.kyb_ed25519_anon_open(n, ring, keys.ctypes.data, 0 if keys.shape[0] == 1 else 32 * ring, m.ctypes.data, p.ctypes.data,
                                       0 if one else 32, blob.ctypes.data, off.ctypes.data,
                                       out.ctypes.data, st.ctypes.data)
        assert rc == 0, lib.kyb_last_error()
        assert out[0] == 0xEE
        raw = out.tobytes()
        slots = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
        msgs, st2 = ed.batch_anon_open(keys, m, p, cts, ring)  # and the wrapper says the same
        assert [int(s) for s in st2] == [int(s) for s in st]
        for i in range(n):
            assert msgs[i] == (slots[i][:len(cts[i]) - 48 - 32 * ring] if not st[i] else b"")
        return slots, [int(s) for s in st]
    import torch

    (blob, off), st = ed.batch_anon_open(torch.from_numpy(keys.copy()).cuda(), torch.from_numpy(np.asarray(mine, dtype=np.int32)).cuda(),
                                         torch.from_numpy(p.copy()).cuda(), _to_dev(cts, 5), ring)
    torch.cuda.synchronize()
    return _from_dev(blob, off, n), [int(s) for s in st.cpu().numpy()]


def check_open(b, slots, sts):
    assert sts == b["open_status"], [(l, s, w) for l, s, w in zip(b["labels"], sts, b["open_status"]) if s != w]
    for label, slot, want, ct in zip(b["labels"], slots, b["opened"], b["cts"]):
        assert len(slot) == len(ct)
        assert slot == (want or b"").ljust(len(ct), b"\0"), label  # a reject: an all-zero slot


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("ex", GOLDEN, ids=[g["name"] for g in GOLDEN])
def test_the_printed_ciphertexts(ed, ex, space):
    keys, mine, x, rand = E.golden_keys(ex["name"])
    want, msg = bytes.fromhex(ex["ciphertext"]), ex["message"].encode()
    cts, st = seal(ed, space, len(keys), keys, [E.new_key(rand)], [msg])
    assert st == [0] and cts[0] == want
    slots, st = open_(ed, space, len(keys), keys, [mine], x, [want])
    assert st == [0] and slots[0] == msg.ljust(len(want), b"\0")


@pytest.mark.parametrize("ex", GOLDEN, ids=[g["name"] for g in GOLDEN])
def test_the_printed_ciphertexts_through_sign_anon(ed, ex):
    from kyber_amd.sign import anon

    keys, mine, x, rand = E.golden_keys(ex["name"])
    want, msg = bytes.fromhex(ex["ciphertext"]), ex["message"].encode()
    suite = ed.NewSuite()
    assert anon.Encrypt(suite, msg, keys, rand.Clone()) == want
    assert anon.Decrypt(suite, want, keys, mine, ed.Scalar(x)) == msg
    # the batch forms: the keys drawn as sequential Encrypts draw them, ONE seal; ONE open, an error per element
    r1, r2 = rand.Clone(), rand.Clone()
    batch = anon.EncryptBatch([msg, b"", msg + msg], keys, r1)
    assert batch == [anon.Encrypt(suite, m, keys, r2) for m in (msg, b"", msg + msg)] and batch[0] == want
    tampered = bytearray(batch[2])
    tampered[-1] ^= 1
    out = anon.DecryptBatch(batch + [bytes(tampered), batch[0][:40]], keys, mine, x)
    assert out[:3] == [msg, b"", msg + msg]
    assert [str(e) for e in out[3:]] == ["invalid ciphertext: failed MAC check", "ciphertext too short"]
    assert all(isinstance(e, anon.AnonError) for e in out[3:])
    with pytest.raises(anon.AnonError, match="failed MAC check"):
        anon.Decrypt(suite, bytes(tampered), keys, mine, x)
    with pytest.raises(ValueError, match="private-key index out of range"):
        anon.Decrypt(suite, want, keys, len(keys), x)


@pytest.mark.parametrize("space", SPACES)
def test_every_message_length(ed, space):
    b = AC.lengths_batch()
    cts, st = seal(ed, space, b["ring"], b["sets"], b["x"], b["msgs"])
    assert st == b["seal_status"] and cts == b["sealed"]
    check_open(b, *open_(ed, space, b["ring"], b["sets"], b["mine"], b["privs"], b["cts"]))


def _prefix(b, n):
    """the first n elements of a batch over a shared set"""
    c = dict(b)
    for k in ("x", "msgs", "sealed", "seal_status", "labels", "cts", "mine", "opened", "open_status"):
        c[k] = b[k][:n]
    if isinstance(b["privs"], (list, tuple)):
        c["privs"] = b["privs"][:n]
    return c


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n,ring,per_element,one", [(5, 1, False, False), (5, 3, False, False), (5, 3, True, False), (5, 3, False, True),
                                                   (5, 27, False, False), (5, 27, True, False), (256, 3, False, False),
                                                   (257, 3, False, False)])
def test_shapes(ed, space, n, ring, per_element, one):
    b = _prefix(AC.shape_batch(257, 3, False, False), n) if n >= 256 else AC.shape_batch(n, ring, per_element, one)
    cts, st = seal(ed, space, ring, b["sets"], b["x"], b["msgs"])
    assert st == [0] * n and cts == b["sealed"]
    assert all(m is not None for m in b["opened"])
    check_open(b, *open_(ed, space, ring, b["sets"], b["mine"], b["privs"], b["cts"]))


@pytest.mark.parametrize("space", SPACES)
def test_rejects_between_valid_neighbours(ed, space):
    b = AC.rejects_batch()
    check_open(b, *open_(ed, space, b["ring"], b["sets"], b["mine"], b["privs"], b["cts"]))


@pytest.mark.parametrize("space", SPACES)
def test_seal_edges_and_the_scalar_reduction(ed, space):
    b = AC.seal_edge_batch()
    cts, st = seal(ed, space, b["ring"], b["sets"], b["x"], b["msgs"])
    assert st == b["seal_status"] and cts == b["sealed"]
    assert cts[1] == bytes(len(cts[1]))  # the member that is no point: an all-zero slot
    i = b["labels"].index("x + l")
    assert cts[i][32:64] == E.slot(b["x"][i], b["sets"][i][0], E.reduced(b["x"][i]))  # the slots carry x mod l


@pytest.mark.parametrize("space", SPACES)
def test_a_shared_set_with_a_member_that_is_no_point(ed, space):
    ring, K, xs, msgs, cts, mem = AC.shared_bad_set()
    out, st = seal(ed, space, ring, K, xs, msgs)
    assert st == [1, 1, 1] and all(c == bytes(len(c)) for c in out)
    slots, st = open_(ed, space, ring, K, [0, 0, 2, 0], [mem[0][0], mem[0][0], mem[2][0], mem[0][0]], cts + [cts[0][:40]])
    assert st == [1, 1, 1, 11] and all(s == bytes(len(s)) for s in slots)


def test_argument_errors_and_empty_batches_touch_no_device(ed):
    assert ed.batch_anon_seal(np.zeros((1, 96), np.uint8), np.zeros((0, 32), np.uint8), [], 3)[0] == []
    with pytest.raises(ValueError):
        ed.batch_anon_seal(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), [b""], 0)
    with pytest.raises(_lib.KyberHipError):
        ed.batch_anon_open(np.zeros((1, 96), np.uint8), [3, 0], np.zeros((2, 32), np.uint8), [b"", b""], 3)  # mine out of range
