"""The case tables of tests/_hash_cases.py reach what they claim: for each hash of expand_message_xmd, every finish
position around the padding switch and the block end, with every class of message length.  Pure arithmetic (no GPU), so
that the tables cannot rot silently; the position formulas themselves are checked against hashlib's block counts."""
import hashlib

import pytest

from tests import _hash_cases as HC

TABLES = [("sha256", HC.SHA256, HC.SHA256_CASES, HC.DST_LENS), ("keccak256", HC.KECCAK256, HC.KECCAK256_CASES, HC.DST_LENS),
          ("sha512", HC.SHA512, HC.SHA512_CASES, HC.DST_LENS_NONEMPTY)]
CLASSES = {"empty", "one byte", "small", "one block", "a few blocks", "several blocks"}


def test_required_positions_are_the_stated_sets():
    assert HC.required_positions(64, 56) == set(range(54, 64)) | {0, 1}
    assert HC.required_positions(128, 112) == set(range(110, 128)) | {0, 1}
    assert HC.required_positions(136, 135) == set(range(126, 136)) | {0, 1}
    for xmd in (HC.SHA256, HC.KECCAK256, HC.SHA512):  # never less than {block - 10 .. block - 1, 0, 1}
        assert HC.required_positions(xmd.block, xmd.threshold) >= set(range(xmd.block - 10, xmd.block)) | {0, 1}


@pytest.mark.parametrize("name,xmd,table,dst_lens", TABLES, ids=[t[0] for t in TABLES])
def test_table_reaches_every_position_in_every_length_class(name, xmd, table, dst_lens):
    req = HC.required_positions(xmd.block, xmd.threshold)
    b0, bi = HC.reached(table, xmd)
    assert req <= set(b0), sorted(req - set(b0))
    assert req <= bi, sorted(req - bi)
    for p in req:
        assert b0[p] == CLASSES, (p, CLASSES - b0[p])
    assert len(table) == len(set(table))
    assert {d for _, d in table} >= set(dst_lens)
    for d in dst_lens:
        assert {(0, d), (1, d), (32, d)} <= set(table)
    assert all(0 <= d <= 255 for _, d in table) and (0 in dst_lens or all(d for _, d in table))
    assert any(m >= 1000 for m, _ in table)
    assert len(table) <= 200  # the oracle's time on the GPU machine is budgeted on this


def test_table_sizes():
    """the counts the docstrings of tests/test_gpu_hash_lengths.py state"""
    assert (len(HC.SHA256_CASES), len(HC.KECCAK256_CASES), len(HC.SHA512_CASES), len(HC.SVDW_CASES)) == (
        len(set(HC.SHA256_CASES)), len(set(HC.KECCAK256_CASES)), len(set(HC.SHA512_CASES)), len(set(HC.SVDW_CASES)))
    assert (len(HC.SHA256_CASES), len(HC.KECCAK256_CASES), len(HC.SHA512_CASES), len(HC.SVDW_CASES)) == (111, 114, 167, 157)


def test_position_formulas_against_hashlib_block_counts():
    """b0_position / bi_position against an independent statement: the bytes hashlib absorbs for b_0 and b_i, and the
    number of compression blocks FIPS 180-4 padding gives them (one more from `threshold` on)"""
    for xmd, hname in ((HC.SHA256, "sha256"), (HC.SHA512, "sha512")):
        lenfield = xmd.block - xmd.threshold
        for m, d in (HC.SHA256_CASES if hname == "sha256" else HC.SHA512_CASES):
            dst_prime = bytes(d) + bytes([d])
            b0_in = bytes(xmd.zpad) + bytes(m) + (xmd.digest * 3).to_bytes(2, "big") + b"\0" + dst_prime
            bi_in = getattr(hashlib, hname)(b0_in).digest() + b"\1" + dst_prime
            assert len(b0_in) % xmd.block == HC.b0_position(m, d, xmd.block, xmd.zpad)
            assert len(bi_in) % xmd.block == HC.bi_position(d, xmd.block, xmd.digest)
            for data, pos in ((b0_in, len(b0_in) % xmd.block), (bi_in, len(bi_in) % xmd.block)):
                blocks = (len(data) + 1 + lenfield + xmd.block - 1) // xmd.block
                assert blocks == len(data) // xmd.block + (2 if pos >= xmd.threshold else 1)


def test_oneshot_and_hkdf_tables():
    req = HC.required_positions(64)
    lens = HC.oneshot_lengths(64)
    for lo, hi in ((0, 64), (64, 128), (1000, 1 << 30)):
        assert {m % 64 for m in lens if lo <= m < hi} == req
    assert 0 in lens and 1 in lens and 55 in lens and 56 in lens
    # HashG1's HKDF: the extract step's inner hash finishes at msg_len mod 64, a long salt's own hash at dst_len mod 64
    assert {m % 64 for m, _ in HC.SVDW_CASES} >= req
    assert {d % 64 for _, d in HC.SVDW_CASES if d > 64} >= req
    assert set(HC.SHA256_CASES) <= set(HC.SVDW_CASES)


def test_boundary_pairs_and_cover():
    x = HC.SHA256
    bp = HC.boundary_pairs(HC.SHA256_CASES, x)
    assert len(set(bp)) == 6 and set(bp) <= set(HC.SHA256_CASES)
    assert [HC.b0_position(*c, x.block, x.zpad) for c in bp[:3]] == [55, 56, 0]
    assert [HC.bi_position(c[1], x.block, x.digest) for c in bp[3:]] == [55, 56, 56] and bp[5][0] >= 1000
    for xmd, table in ((HC.SHA256, HC.SHA256_CASES),):
        cv = HC.cover(table, xmd)
        req = HC.required_positions(xmd.block, xmd.threshold)
        b0, bi = HC.reached(cv, xmd)
        assert req <= set(b0) and req <= bi and set(cv) <= set(table)
        assert 12 <= len(cv) <= 32
        assert any(m == 0 for m, _ in cv) and any(d == 0 for _, d in cv) and any(d == 255 for _, d in cv)


def test_messages_are_deterministic_and_distinct():
    a = HC.messages(b"t", 67, 120)
    assert a.shape == (67, 120) and (a == HC.messages(b"t", 67, 120)).all()
    assert len({bytes(r) for r in a}) == 67
    assert HC.messages(b"t", 67, 0).shape == (67, 0)
    assert len(HC.dst_bytes(255)) == 255 and HC.dst_bytes(0) == b""
