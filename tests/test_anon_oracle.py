"""The sign/anon oracle (tests/_anon_oracle.py) against what the reference prints: under blake2xb.New(nil) its key
generation and Sign reproduce the six signatures of sig_test.go's examples byte for byte, Verify accepts them and
rejects them under the wrong message, and the tags are the printed ones."""
import json
import os

import pytest

from tests import _anon_oracle as A

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anon.json")))


@pytest.fixture(scope="module")
def signed():
    out = {}
    for name in A.GOLDEN_EXAMPLES:
        keys, scope, mines, xs, r = A.golden_keys(name)
        out[name] = (keys, scope, [A.sign(A.GOLDEN_MESSAGE, keys, scope, m, x, r) for m, x in zip(mines, xs)])
    return out


@pytest.mark.parametrize("name", A.GOLDEN_EXAMPLES)
def test_sign_reproduces_the_printed_signatures(signed, name):
    want = [bytes.fromhex(h) for h in GOLDEN["examples"][name]["signatures"]]
    assert signed[name][2] == want


@pytest.mark.parametrize("name", A.GOLDEN_EXAMPLES)
def test_verify_accepts_the_printed_signatures_and_rejects_the_wrong_message(signed, name):
    keys, scope, _ = signed[name]
    tags = []
    for h in GOLDEN["examples"][name]["signatures"]:
        sig = bytes.fromhex(h)
        tag = A.verify(A.GOLDEN_MESSAGE, keys, scope, sig)
        assert tag is not None and len(tag) == (32 if scope is not None else 0)
        assert A.verify(A.GOLDEN_BAD_MESSAGE, keys, scope, sig) is None
        tags.append(tag.hex())
    if scope is not None:
        assert tags == GOLDEN["examples"][name]["tags"]
        assert tags[0] == tags[1] and tags[2] == tags[3] and tags[0] != tags[2]


def test_rotated_chain_closes_on_a_valid_signature(signed):
    keys, scope, sigs = signed["ExampleSign_linkable"]
    full = A.chain(A.GOLDEN_MESSAGE, keys, scope, sigs[0])
    assert full[2] == 1 and full[0] == sigs[0][:32]
    # from position 1 with c_1 in slot 0, two steps lead back to c_1's predecessor chain: c_zero is the signature's c_0
    c1 = A.chain(A.GOLDEN_MESSAGE, keys, scope, sigs[0], 0, 1)[1]
    rot = A.chain(A.GOLDEN_MESSAGE, keys, scope, c1 + sigs[0][32:], 1, 2)
    assert rot[0] == sigs[0][:32] and rot[3] == 0
