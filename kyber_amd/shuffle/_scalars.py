"""Scalar-field vectors of the shuffle provers: Python integers modulo l on the host, (n, 32) little-endian byte rows
at the engine's boundary."""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed

L = ed.ORDER


def ints(rows) -> list:
    """the integers of (n, 32) little-endian rows, unreduced"""
    b = np.ascontiguousarray(np.asarray(rows), dtype=np.uint8).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def rows(values) -> np.ndarray:
    """(n, 32) little-endian rows of integers, each reduced modulo l"""
    values = list(values)
    return np.frombuffer(b"".join((v % L).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


def inv_all(values) -> list:
    """1 / v modulo l for every v by Montgomery's trick: one exponentiation for the batch.  Inv(0) = 0, as the
    reference's exponentiation gives (scalar.go:157-175)."""
    values = [v % L for v in values]
    pre, acc = [], 1
    for v in values:
        pre.append(acc)
        if v:
            acc = acc * v % L
    inv = pow(acc, L - 2, L)
    out = [0] * len(values)
    for i in range(len(values) - 1, -1, -1):
        if values[i]:
            out[i] = inv * pre[i] % L
            inv = inv * values[i] % L
    return out


def points(x) -> np.ndarray:
    """a vector of points as (n, 32) rows: an array, wire bytes, or a sequence of 32-byte encodings / Point mirrors"""
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 32)
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(x), dtype=np.uint8).reshape(-1, 32).copy()
    enc = b"".join(e.MarshalBinary() if hasattr(e, "MarshalBinary") else bytes(e) for e in x)
    return np.frombuffer(enc, dtype=np.uint8).reshape(-1, 32).copy()


def point(x):
    """one point as its 32 bytes; None (the standard base) stays None"""
    if x is None:
        return None
    p = points([x] if hasattr(x, "MarshalBinary") else x)
    if p.shape[0] != 1:
        raise ValueError("one 32-byte point")
    return p.tobytes()


def mul_g(scalar_rows, G) -> np.ndarray:
    """scalars[i] * G as one batched call: Point.Mul(s, nil) is the base-point multiplication (point.go:243) and goes
    through mul_base; a given G goes through mul_same_base.  The two differ in value for unreduced scalars."""
    return np.asarray(ed.commit(scalar_rows, G))


def checked(result, what: str) -> np.ndarray:
    out, st = result
    if np.asarray(st).any():
        raise ValueError(f"{what}: invalid Ed25519 curve point")
    return np.asarray(out)
