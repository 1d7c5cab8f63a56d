"""The wire form of share/vss's Deal: kyber_amd/share/vss/_wire.py and the oracle's own restatement against the byte
vectors the reference's internal/protobuf tests assert (tests/golden/vss_protobuf.json, copied as data), against each
other on deals of every shape, and against the lengths the engine tests use for "a real deal".

Limit of the check: the reference has no test that prints a marshalled Deal and no Go toolchain is at hand.  The vectors
pin the key byte, the zigzag varint of an int and the length-delimited form; a BinaryMarshaler's bytes pass through
unchanged (the TestBigInt vectors); the field list is vss.go's and v3marshaling.go's, read from the text."""
import json
import os

import pytest

from kyber_amd.share.vss import _wire as W
from tests import _vss_cases as VC
from tests import _vss_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "vss_protobuf.json")))


def _encode(fields, sint, fbytes):
    out = b""
    for kind, num, v in fields:
        out += sint(num, v) if kind == "sint" else fbytes(num, bytes.fromhex(v))
    return out


def test_both_encoders_give_the_references_vectors():
    for v in GOLDEN["vectors"]:
        want = bytes.fromhex(v["bytes"])
        assert _encode(v["fields"], W.f_svarint, W.f_bytes) == want, v["from"]
        assert _encode(v["fields"], VO.pb_sint, VO.pb_bytes) == want, v["from"]
        assert [(n, w) for n, w, _ in W.fields(want)] == [(f[1], 0 if f[0] == "sint" else 2) for f in v["fields"]]
    for m in GOLDEN["marshalers"]:  # a marshaler's bytes travel as they are, behind a key and a length, with no type tag
        b = bytes.fromhex(m["bytes"])
        assert W.f_bytes(2, b) == VO.pb_bytes(2, b) == bytes([0x12, len(b)]) + b
        assert W.fields(W.f_bytes(2, b)) == [(2, 2, b)]


def test_varints_and_zigzag():
    for v, want in ((0, "00"), (1, "01"), (127, "7f"), (128, "8001"), (300, "ac02"), (2**32 - 1, "ffffffff0f")):
        assert W.uvarint(v).hex() == VO.pb_uvarint(v).hex() == want
    for v, z in ((0, 0), (-1, 1), (1, 2), (-2, 3), (37, 74), (2**32 - 1, 2**33 - 2), (-2**63, 2**64 - 1)):
        assert W.zigzag(v) == z and W.unzigzag(z) == v
        assert VO.pb_sint(1, v) == W.f_svarint(1, v)


@pytest.mark.parametrize("t", [0, 1, 2, 17])
@pytest.mark.parametrize("index", [0, 1, 63, 64, 2**32 - 1])
def test_a_deal_travels_both_ways_and_has_the_length_the_engine_tests_use(t, index):
    sid = bytes(range(32))
    commits = [VO.DO.base_mul(j + 1) for j in range(t)]
    d = VO.Deal(sid, VO.PriShare(index, 5 + index), t, commits)
    wire = d.Marshal()
    assert wire == W.encode_deal(sid, W.encode_pri_share(index, VO.sc(5 + index)), t, commits)
    if index < 64 and t in VC.DEAL_LEN:
        assert len(wire) == VC.DEAL_LEN[t]
    assert wire[:2] == b"\x0a\x20" and wire[34] == 0x12 and wire[36] == 0x08  # SessionID; SecShare, in it I first
    got = W.decode_deal(wire)
    assert got == (sid, W.encode_pri_share(index, VO.sc(5 + index)), t, commits)
    assert W.decode_pri_share(got[1]) == (index, VO.sc(5 + index))
    back = VO.Deal.Unmarshal(wire)
    assert (back.SessionID, back.SecShare.I, back.SecShare.V, back.T, back.Commitments) == (sid, index, 5 + index, t, commits)


def test_decoding_refuses_what_the_reference_refuses():
    wire = W.encode_deal(bytes(32), W.encode_pri_share(3, bytes(32)), 4, [VO.DO.base_mul(1)])
    for cut in (1, 33, 35, 40, len(wire) - 1):
        with pytest.raises(ValueError, match="bad protobuf"):
            W.decode_deal(wire[:cut])
    with pytest.raises(ValueError, match="bad wiretype for bytes"):
        W.decode_deal(W.f_uvarint(1, 7))
    with pytest.raises(ValueError, match="bad wiretype for uint"):
        W.decode_deal(W.f_bytes(3, b"x"))
    with pytest.raises(ValueError, match="unknown protobuf wire-type"):
        W.decode_deal(bytes([0x0b]))
    assert W.decode_deal(wire + W.f_uvarint(9, 1)) == W.decode_deal(wire)  # a field the struct does not have is skipped
    for i in (-1, 2**32):
        with pytest.raises(ValueError, match="cannot cast I as uint32 due to overflow"):
            W.decode_pri_share(W.f_svarint(1, i) + W.f_bytes(2, bytes(32)))


@pytest.mark.parametrize("t", [0, 2, 17])
@pytest.mark.parametrize("index", [0, 63, 64, 2**32 - 1])
def test_rabins_deal_has_its_own_field_list(t, index):
    """rabinCompatibleDeal (rabin/vss.go:92-98): SessionID, SecShare, RndShare, T, Commitments as fields 1 to 5"""
    sid = bytes(range(32))
    commits = [VO.DO.base_mul(j + 1) for j in range(t)]
    d = VO.RabinDeal(sid, VO.PriShare(index, 5 + index), VO.PriShare(index, 9 + index), t, commits)
    wire = d.Marshal()
    f, g = W.encode_pri_share(index, VO.sc(5 + index)), W.encode_pri_share(index, VO.sc(9 + index))
    assert wire == W.encode_deal_rabin(sid, f, g, t, commits)
    assert [n for n, _, _ in W.fields(wire)] == [1, 2, 3, 4] + [5] * t
    if index < 64:
        assert len(wire) == 34 + 38 + 38 + 2 + 34 * t
    assert W.decode_deal_rabin(wire) == (sid, f, g, t, commits)
    back = VO.RabinDeal.Unmarshal(wire)
    assert (back.SessionID, back.SecShare.I, back.SecShare.V, back.RndShare.I, back.RndShare.V, back.T, back.Commitments) == (
        sid, index, 5 + index, index, 9 + index, t, commits)
    with pytest.raises(ValueError, match="bad protobuf"):
        W.decode_deal_rabin(wire[:-1])
    with pytest.raises(ValueError, match="bad wiretype for uint"):
        W.decode_deal_rabin(W.f_bytes(4, b"x"))
