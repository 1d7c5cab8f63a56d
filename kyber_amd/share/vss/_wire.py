"""The wire form of share/vss's Deal: ``internal/protobuf`` restated for exactly the structs vss.go marshals
(pedersenCompatibleDeal, vss.go:64-69, and compatiblePriShare, internal/v3marshaling.go:21-24).  The rules, from encode.go:

  * fields are numbered from 1 in declaration order; a key is the varint (number << 3 | wire type);
  * ``[]byte`` is length-delimited (encode.go:335-339); a kyber.Point or kyber.Scalar behind an interface is its
    MarshalBinary, length-delimited, with NO type tag in front: a tag is written only for a registered generator, and none
    is registered outside the reference's tests (encode.go:268-286);
  * ``uint32`` is a plain varint (encode.go:146-149), ``int64`` a zigzag varint (encode.go:134-137): PriShare.I travels
    as an int64 (v3marshaling.go:21-24);
  * a slice of points is one length-delimited field per element (sliceReflect);
  * zero values are written; a nil interface or pointer is left out.

Decoding (decode.go:108-170) walks the buffer key by key; a field number the struct does not have is skipped, a wrong
wire type is an error, and so is a value that runs past the buffer.  The messages are decode.go's; the reference wraps
them with the name of the Go field, which is not restated."""
from __future__ import annotations


def uvarint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v: int) -> int:
    """encode.go svarint: (v << 1) ^ (v >> 63) on 64 bits"""
    return ((v << 1) ^ (v >> 63)) & 0xFFFFFFFFFFFFFFFF


def unzigzag(u: int) -> int:
    return (u >> 1) ^ -(u & 1)


def f_bytes(num: int, b: bytes) -> bytes:
    return uvarint(num << 3 | 2) + uvarint(len(b)) + bytes(b)


def f_uvarint(num: int, v: int) -> bytes:
    return uvarint(num << 3) + uvarint(v)


def f_svarint(num: int, v: int) -> bytes:
    return uvarint(num << 3) + uvarint(zigzag(v))


def _read_uvarint(buf: bytes, pos: int, what: str):
    v = shift = 0
    while True:
        if pos >= len(buf) or shift > 63:
            raise ValueError(what)
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if b < 0x80:
            return v, pos
        shift += 7


def fields(buf: bytes):
    """[(number, wire type, value)]: value is an int for varints and fixed-width fields, bytes for length-delimited ones"""
    out, pos = [], 0
    while pos < len(buf):
        key, pos = _read_uvarint(buf, pos, "bad protobuf field key")
        wt, num = key & 7, key >> 3
        if wt == 0:
            v, pos = _read_uvarint(buf, pos, "bad protobuf varint value")
        elif wt == 5:
            if pos + 4 > len(buf):
                raise ValueError("bad protobuf 32-bit value")
            v, pos = int.from_bytes(buf[pos:pos + 4], "little"), pos + 4
        elif wt == 1:
            if pos + 8 > len(buf):
                raise ValueError("bad protobuf 64-bit value")
            v, pos = int.from_bytes(buf[pos:pos + 8], "little"), pos + 8
        elif wt == 2:
            n, pos = _read_uvarint(buf, pos, "bad protobuf length-delimited value")
            if pos + n > len(buf):
                raise ValueError("bad protobuf length-delimited value")
            v, pos = bytes(buf[pos:pos + n]), pos + n
        else:
            raise ValueError("unknown protobuf wire-type")
        out.append((num, wt, v))
    return out


def encode_pri_share(i: int, v: bytes) -> bytes:
    """internal.MarshalPriShare: compatiblePriShare{I int64, V kyber.Scalar}"""
    return f_svarint(1, i) + f_bytes(2, v)


def decode_pri_share(buf: bytes):
    """internal.UnmarshalPriShare: (I, V bytes or None)"""
    i, v = 0, None
    for num, wt, val in fields(buf):
        if num == 1:
            if wt != 0:
                raise ValueError("bad wiretype for sint")
            i = unzigzag(val)
        elif num == 2:
            if wt != 2:
                raise ValueError("bad wiretype for bytes")
            v = val
    if i < 0 or i > 0xFFFFFFFF:
        raise ValueError("cannot cast I as uint32 due to overflow")
    return i, v


def encode_deal(sid: bytes, sec_share: bytes, t: int, commits) -> bytes:
    """protobuf.Encode(pedersenCompatibleDeal{SessionID, SecShare, T, Commitments})"""
    return f_bytes(1, sid) + f_bytes(2, sec_share) + f_uvarint(3, t) + b"".join(f_bytes(4, c) for c in commits)


def decode_deal(buf: bytes):
    """(SessionID, SecShare bytes, T, [commitment bytes]) of a pedersenCompatibleDeal"""
    sid, sec, t, commits = b"", b"", 0, []
    for num, wt, val in fields(buf):
        if num in (1, 2, 4) and wt != 2:
            raise ValueError("bad wiretype for bytes" if num != 4 else "bad wiretype for repeated field")
        if num == 1:
            sid = val
        elif num == 2:
            sec = val
        elif num == 3:
            if wt != 0:
                raise ValueError("bad wiretype for uint")
            t = val & 0xFFFFFFFF
        elif num == 4:
            commits.append(val)
    return sid, sec, t, commits


def encode_deal_rabin(sid: bytes, sec_share: bytes, rnd_share: bytes, t: int, commits) -> bytes:
    """protobuf.Encode(rabinCompatibleDeal{SessionID, SecShare, RndShare, T, Commitments}) (rabin/vss.go:92-98)"""
    return f_bytes(1, sid) + f_bytes(2, sec_share) + f_bytes(3, rnd_share) + f_uvarint(4, t) + b"".join(f_bytes(5, c) for c in commits)


def decode_deal_rabin(buf: bytes):
    """(SessionID, SecShare bytes, RndShare bytes, T, [commitment bytes]) of a rabinCompatibleDeal"""
    sid, sec, rnd, t, commits = b"", b"", b"", 0, []
    for num, wt, val in fields(buf):
        if num in (1, 2, 3, 5) and wt != 2:
            raise ValueError("bad wiretype for bytes" if num != 5 else "bad wiretype for repeated field")
        if num == 1:
            sid = val
        elif num == 2:
            sec = val
        elif num == 3:
            rnd = val
        elif num == 4:
            if wt != 0:
                raise ValueError("bad wiretype for uint")
            t = val & 0xFFFFFFFF
        elif num == 5:
            commits.append(val)
    return sid, sec, rnd, t, commits
