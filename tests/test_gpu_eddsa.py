"""kyb_ed25519_eddsa_expand and kyb_ed25519_eddsa_sign on the GPU, host and _dev entries, against the reference's own
1 024 sign.input lines (every output byte is the fixture's), the RFC 8032 rows and the oracle (tests/_eddsa_oracle.py):
all lines in one call, batch sizes either side of the wave and the block from both ends of the file, one key for the
batch, the piece edge against the standing kyb_ed25519_schnorr_sign, NULL and prefilled status, and sign/eddsa end to
end."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _eddsa_oracle as EO

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 257)
ENTRIES = ["host", "dev"]


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _dev(x, dtype=np.uint8):
    import torch

    return torch.from_numpy(np.frombuffer(x, dtype=dtype).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=dtype)).cuda()


def _dev_msgs(msgs):
    return _dev(b"".join(msgs) or b"\0"), _dev(np.cumsum([0] + [len(m) for m in msgs]).astype(np.int64), np.int64)


def expand(ed, entry, seeds):
    """(secrets, prefixes, pubs) as numpy arrays, through either entry"""
    if entry == "host":
        return tuple(np.asarray(x) for x in ed.batch_eddsa_expand(seeds))
    import torch

    out = ed.batch_eddsa_expand(_dev(seeds))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def sign(ed, entry, secrets, prefixes, pubs, msgs):
    """sigs (n, 64) as a numpy array, through either entry; the status must come back zero"""
    if entry == "host":
        sigs, st = ed.batch_eddsa_sign(secrets, prefixes, pubs, msgs)
    else:
        import torch

        sigs, st = ed.batch_eddsa_sign(_dev(secrets), _dev(prefixes), _dev(pubs), _dev_msgs(msgs))
        torch.cuda.synchronize()
        sigs, st = sigs.cpu().numpy(), st.cpu().numpy()
    assert not np.asarray(st).any()
    return np.asarray(sigs)


def _rows(x):
    return [bytes(r) for r in x]


# ------------------------------------------------------------------------------------------------ the reference's lines
@pytest.mark.parametrize("entry", ENTRIES)
def test_all_sign_input_lines_in_one_call_each(ed, entry):
    seeds, kat, msgs, sigs = EO.sign_input()
    secrets, prefixes, pubs = expand(ed, entry, seeds)
    assert np.array_equal(secrets, kat[:, 0]) and np.array_equal(pubs, kat[:, 1])
    assert np.array_equal(prefixes, EO.sign_input_keys()[1])
    got = sign(ed, entry, secrets, prefixes, pubs, msgs)
    assert _rows(got) == sigs
    assert np.array_equal(got[:, :32], kat[:, 3]) and np.array_equal(got[:, 32:], kat[:, 5])


@pytest.mark.parametrize("entry", ENTRIES)
def test_rfc8032(ed, entry):
    rfc = EO.rfc8032()
    secrets, prefixes, pubs = expand(ed, entry, b"".join(r[0] for r in rfc))
    assert _rows(pubs) == [r[1] for r in rfc]
    assert [(bytes(a), bytes(p), bytes(A)) for a, p, A in zip(secrets, prefixes, pubs)] == [EO.expand(r[0]) for r in rfc]
    assert _rows(sign(ed, entry, secrets, prefixes, pubs, [r[2] for r in rfc])) == [r[3] for r in rfc]


@pytest.mark.parametrize("entry", ENTRIES)
def test_batch_sizes_from_both_ends_of_the_file(ed, entry):
    """the tail's messages are 767 to 1 023 bytes: multi-block messages in the first and the last lane of a block"""
    seeds, kat, msgs, sigs = EO.sign_input()
    want = EO.sign_input_keys()
    for n in SIZES:
        for rows in (slice(0, n), slice(1024 - n, 1024)):
            got = expand(ed, entry, seeds[rows])
            for g, w in zip(got, want):
                assert g.shape == (n, 32) and np.array_equal(g, w[rows]), (n, rows)
            assert _rows(sign(ed, entry, *got, msgs[rows])) == sigs[rows], (n, rows)


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_key_signs_every_message(ed, entry):
    _, _, msgs, _ = EO.sign_input()
    a, p, A = (bytes(x[5]) for x in EO.sign_input_keys())
    got = _rows(sign(ed, entry, a, p, A, msgs))
    for i in EO.BOUNDARY:
        assert got[i] == EO.sign(a, p, A, msgs[i]), i
    ok, st = ed.batch_verify([A] * 1024, msgs, got)
    assert ok.all() and not st.any()


# ------------------------------------------------------------------------------------------------------- one piece edge
@pytest.fixture(scope="module")
def piece_edge(ed):
    """n = 2^18 + 5 messages of 0 to 40 bytes under the 1 024 keys repeated, and their signatures through the standing
    kyb_ed25519_schnorr_sign with r = SHA-512(prefix || msg) mod l from hashlib"""
    n = (1 << 18) + 5
    secrets, prefixes, pubs = EO.sign_input_keys()
    rng = np.random.default_rng(8032)
    lens = rng.integers(0, 41, size=n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    blob = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8).tobytes()
    msgs = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
    idx = np.arange(n) % 1024
    pre = _rows(prefixes)
    r = b"".join((int.from_bytes(hashlib.sha512(pre[i & 1023] + m).digest(), "little") % O.L).to_bytes(32, "little") for i, m in enumerate(msgs))
    want, st = ed.batch_schnorr_sign(r, np.ascontiguousarray(secrets[idx]), msgs)
    assert not np.asarray(st).any()
    return n, idx, msgs, np.asarray(want)


@pytest.mark.parametrize("entry", ENTRIES)
def test_piece_edge_against_schnorr_sign(ed, piece_edge, entry):
    n, idx, msgs, want = piece_edge
    secrets, prefixes, pubs = (np.ascontiguousarray(x[idx]) for x in EO.sign_input_keys())
    got = sign(ed, entry, secrets, prefixes, pubs, msgs)
    assert got.shape == (n, 64) and np.array_equal(got, want)
    for i in (0, (1 << 18) - 1, 1 << 18, (1 << 18) + 4):
        assert bytes(got[i]) == EO.sign(bytes(secrets[i]), bytes(prefixes[i]), bytes(pubs[i]), msgs[i]), i


# ----------------------------------------------------------------------------------------------------------- the status
@pytest.mark.parametrize("entry", ENTRIES)
def test_null_status_and_a_prefilled_status(ed, entry):
    import torch

    _, _, msgs, sigs = EO.sign_input()
    rows = slice(60, 190)
    n = 130
    keys = [np.ascontiguousarray(x[rows]) for x in EO.sign_input_keys()]
    blob = np.frombuffer(b"".join(msgs[rows]), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(m) for m in msgs[rows]]).astype(np.uint64)
    lib = _lib.load()
    for status in (None, np.full(n, 0xEE, dtype=np.uint8)):
        out = np.full((n, 64), 0xEE, dtype=np.uint8)
        if entry == "host":
            rc = lib.kyb_ed25519_eddsa_sign(n, *(k.ctypes.data for k in keys), 32, blob.ctypes.data, off.ctypes.data, out.ctypes.data,
                                            None if status is None else status.ctypes.data)
            st = status
        else:
            d = [_dev(k) for k in keys] + [_dev(blob), _dev(off.view(np.int64), np.int64), _dev(out)]
            d_st = None if status is None else _dev(status)
            rc = lib.kyb_ed25519_eddsa_sign_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 32, d[3].data_ptr(), d[4].data_ptr(),
                                                d[5].data_ptr(), None if d_st is None else d_st.data_ptr(),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            out, st = d[5].cpu().numpy(), (None if d_st is None else d_st.cpu().numpy())
        assert rc == 0 and _rows(out) == sigs[rows]
        assert st is None or not st.any()


# ------------------------------------------------------------------------------------------------------------ end to end
class _SeedStream:
    """a stream that hands out the given seeds, 32 bytes a draw"""

    def __init__(self, seeds):
        self.left = b"".join(seeds)

    def XORKeyStream(self, src: bytes) -> bytes:
        out, self.left = self.left[:len(src)], self.left[len(src):]
        assert len(out) == len(src)
        return out


def test_sign_eddsa_end_to_end_against_the_fixture():
    from kyber_amd.sign import eddsa

    seeds, kat, msgs, sigs = EO.sign_input()
    rows = list(range(90, 154))
    keys = eddsa.NewEdDSABatch(_SeedStream(_rows(seeds[rows])), len(rows))
    assert [k.Public.MarshalBinary() for k in keys] == _rows(kat[rows, 1])
    assert [k.Secret.v for k in keys] == _rows(kat[rows, 0])
    assert [k.MarshalBinary() for k in keys] == [bytes(seeds[i]) + kat[i, 1].tobytes() for i in rows]
    one = eddsa.NewEdDSA(_SeedStream([bytes(seeds[rows[3]])]))
    assert one == keys[3] and eddsa.EdDSA().UnmarshalBinary(one.MarshalBinary()) == one
    got = eddsa.SignBatch(keys, [msgs[i] for i in rows])
    assert got == [sigs[i] for i in rows]
    assert keys[3].Sign(msgs[rows[3]]) == got[3]
    single = eddsa.SignBatch(keys[3], [msgs[i] for i in rows[:5]])
    assert single[3] == got[3] and len(set(single)) == 5
    for k, i, s in zip(keys[:6], rows, got):
        assert eddsa.Verify(k.Public, msgs[i], s) is None
    with pytest.raises(ValueError, match="^error: reconstructed S is not equal to signature$"):
        eddsa.Verify(keys[0].Public, msgs[rows[0]] + b"x", got[0])
    with pytest.raises(ValueError, match="^error: signature length invalid: expect 64 but got 63$"):
        eddsa.Verify(keys[0].Public, msgs[rows[0]], got[0][:63])
