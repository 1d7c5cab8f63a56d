"""kyb_ed25519_fs_challenge on the GPU against the Python XOF (kyber_amd/util/blake2xb.py): every name length around the
64-byte key and the 128-byte block, every data length of tests/test_proof_host.py, one name for the batch and a name per
proof, through the host and the device entry, the device one with a names pointer of every alignment."""
import random

import numpy as np
import pytest

from tests.test_proof_host import DATA_LENS, NAME_LENS, fs_challenge

pytestmark = pytest.mark.gpu

N = 129


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


@pytest.mark.parametrize("data_len", DATA_LENS)
@pytest.mark.parametrize("name_len", NAME_LENS)
def test_challenges_match_the_python_xof(ed, name_len, data_len):
    import torch

    rng = random.Random(name_len * 4096 + data_len + 1)
    data = np.frombuffer(rng.randbytes(N * data_len), dtype=np.uint8).reshape(N, data_len).copy()
    rows = [data[i].tobytes() for i in range(N)]
    # one name for the batch
    name = rng.randbytes(name_len)
    want = b"".join(fs_challenge(name, r) for r in rows)
    c, st = ed.batch_fs_challenge(name, data)
    assert c.tobytes() == want and not st.any()
    c, st = ed.batch_fs_challenge(name, torch.from_numpy(data).cuda())
    assert c.cpu().numpy().tobytes() == want and not st.cpu().numpy().any()
    # a name per proof: lengths around this one, empty ones among them
    names = [rng.randbytes(max(0, name_len + rng.choice((-1, 0, 0, 1))) if i % 7 else 0) for i in range(N)]
    names[-1] = rng.randbytes(name_len)
    want = b"".join(fs_challenge(nm, r) for nm, r in zip(names, rows))
    c, st = ed.batch_fs_challenge(names, data)
    assert c.tobytes() == want and not st.any()
    # the device entry with the names at byte offset 1, 2 or 3 of an allocation
    shift = 1 + name_len % 3
    blob = torch.from_numpy(np.frombuffer(bytes(shift) + b"".join(names) + b"\0", dtype=np.uint8).copy()).cuda()[shift:]
    off = torch.from_numpy(np.cumsum([0] + [len(nm) for nm in names]).astype(np.int64)).cuda()
    assert blob.data_ptr() % 4 == shift
    c, st = ed.batch_fs_challenge((blob, off), torch.from_numpy(data).cuda())
    assert c.cpu().numpy().tobytes() == want and not st.cpu().numpy().any()


def test_an_empty_batch_is_an_empty_answer(ed):
    c, st = ed.batch_fs_challenge(b"name", np.zeros((0, 32), dtype=np.uint8))
    assert c.shape == (0, 32) and st.shape == (0,)
