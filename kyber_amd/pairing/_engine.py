"""Shared host-side plumbing for the pairing suites (BLS12-381, bn256): batch entry points over the
C ABI and kyber.Scalar / kyber.Point / pairing.Suite mirrors holding canonical wire encodings.
No curve or field arithmetic happens in Python (scalars mod the group order are host plumbing,
like the reference's group/mod.Int)."""
from __future__ import annotations

import os

import numpy as np

from .._buf import HOST, _stream, space_of  # noqa: F401 (_stream: the stream handle the debug entry points take, read from here by the tests)


# flags of the pairing-suite entry points (include/kyber_hip.h)
F_UNCOMPRESSED = 2
F_UNCOMPRESSED_OUT = 4
F_TRUSTED_ALL = 0xF00


# Batch sizes from which a device call beats one CPU core of the reference (tools/latency_probe.py on MI355X,
# profiles/r03_single_call_latency.json; the Go suite's MinDeviceBatch / MinDevicePairings): below them a caller with a
# CPU implementation at hand should use it.  tests/test_callers_host.py holds these equal to the Go suite's.
MIN_DEVICE_BATCH, MIN_DEVICE_PAIRINGS = 64, 8


def F_SCALAR_BITS(b: int) -> int:
    """*_msm only: every scalar is below 2^b (KYB_F_SCALAR_BITS); higher bits are ignored."""
    if not 1 <= b <= 256:
        raise ValueError("scalar bits must be in 1..256")
    return b << 16


def F_TRUSTED(i: int) -> int:
    """Point argument i was validated before (an output of this library / of an earlier UnmarshalBinary)."""
    return 0x100 << i


def pack_fixed(items, width: int):
    """Pack a list of per-element encodings into an (n, width) array.  Elements of the wrong length are replaced by
    `width` zero bytes (which no suite decodes) and their indices returned, so that one malformed element neither
    shifts the elements after it nor makes the native call read past the buffer: the caller reports those lanes as
    ok = False / status = BAD_POINT, the way the reference's UnmarshalBinary rejects only the offending element."""
    n = len(items)
    out = np.zeros((n, width), dtype=np.uint8)
    bad = []
    for i, it in enumerate(items):
        b = bytes(it)
        if len(b) != width:
            bad.append(i)
        else:
            out[i] = np.frombuffer(b, dtype=np.uint8)
    return out, bad


class Engine:
    """Batch API of one pairing suite; `prefix` selects the kyb_<prefix>_* entry points."""

    def __init__(self, prefix, name, order, g1_len, g2_len, gt_len, g1_base, g2_base, g1_null, g2_null, neg):
        self.prefix, self.name, self.ORDER = prefix, name, order
        self.neg = neg  # neg(group, encoding) -> encoding of the inverse point (wire-level, no curve arithmetic)
        self.G1_LEN, self.G2_LEN, self.GT_LEN, self.SCALAR_LEN = g1_len, g2_len, gt_len, 32
        self.G1_BASE, self.G2_BASE, self.G1_NULL, self.G2_NULL = g1_base, g2_base, g1_null, g2_null
        # BLS12-381 inputs may be ZCash uncompressed (KYB_F_UNCOMPRESSED); bn256's wire format already is
        self.unc_factor = 2 if prefix == "bls12381" else 1

    def _in_len(self, group: int, flags: int) -> int:
        w = self.G1_LEN if group == 1 else self.G2_LEN
        return w * self.unc_factor if flags & F_UNCOMPRESSED else w

    def _out_len(self, group: int, flags: int) -> int:
        w = self.G1_LEN if group == 1 else self.G2_LEN
        return w * self.unc_factor if flags & F_UNCOMPRESSED_OUT else w

    def _sym(self, suffix: str) -> str:
        return f"kyb_{self.prefix}_{suffix}"

    def mul(self, group: int, scalars, points, same_base: bool, flags: int = 0):
        wi, w = self._in_len(group, flags), self._out_len(group, flags)
        sp = space_of(scalars)
        s, p = sp.rows(scalars, 32), sp.rows(points, wi)  # (points may be bytes next to device scalars: Commit's default base)
        n = s.shape[0]
        if not same_base and p.shape[0] != n:
            raise ValueError("scalars/points length mismatch")
        out, st = sp.out((n, w)), sp.status(n)
        # one base for the batch: a stride of 0 on the device, an entry point of its own on the host
        stride = (0 if same_base else wi,) if sp.is_device else ()
        name = "mul_same_base" if same_base and not sp.is_device else "mul"
        sp.call(self._sym(f"g{group}_{name}"), n, sp.ptr(s), sp.ptr(p), *stride, sp.ptr(out), sp.ptr(st), flags)
        return out, st[:n]

    def g1_batch_mul(self, scalars, points, flags: int = 0):
        """(out, status): out[i] = scalars[i] * points[i] on G1."""
        return self.mul(1, scalars, points, False, flags)

    def g2_batch_mul(self, scalars, points, flags: int = 0):
        return self.mul(2, scalars, points, False, flags)

    def g1_commit(self, scalars, base=None, flags: int = 0):
        """share.PriPoly.Commit (share/poly.go:143-149): commits[i] = coeffs[i] * base."""
        if base is None:  # the suite's own generator: valid by construction, nothing to re-check in every lane
            return self.mul(1, scalars, self.G1_BASE, True, flags | F_TRUSTED(0))
        return self.mul(1, scalars, base, True, flags)

    def g2_commit(self, scalars, base=None, flags: int = 0):
        if base is None:
            return self.mul(2, scalars, self.G2_BASE, True, flags | F_TRUSTED(0))
        return self.mul(2, scalars, base, True, flags)

    def add(self, group: int, a, b):
        """(out, status): out[i] = a[i] + b[i]  (N x Point.Add).  CUDA tensors stay on the device (enqueue only)."""
        w = self.G1_LEN if group == 1 else self.G2_LEN
        sp = space_of(a)
        x, y = sp.rows(a, w), sp.rows(b, w)
        if x.shape != y.shape:
            raise ValueError("length mismatch")
        n = x.shape[0]
        out, st = sp.out(x.shape), sp.status(n)
        sp.call(self._sym(f"g{group}_add"), n, sp.ptr(x), sp.ptr(y), sp.ptr(out), sp.ptr(st))
        return out, st[:n]

    def batch_unmarshal(self, group: int, points, flags: int = 0):
        """(out, status): N x Point.UnmarshalBinary (kilic/g1.go:127-131; pairing/bn256/point.go:206-238, 466-499):
        status[i] != 0 where the reference returns an error, out[i] = the accepted point re-encoded (uncompressed
        affine with F_UNCOMPRESSED_OUT on BLS12-381).  Host buffers or torch device tensors.  Points that pass may
        be handed to later calls with F_TRUSTED(i) (| F_UNCOMPRESSED)."""
        sp = space_of(points)
        p = sp.rows(points, self._in_len(group, flags))
        n = p.shape[0]
        out, st = sp.out((n, self._out_len(group, flags))), sp.status(n)
        sp.call(self._sym(f"g{group}_unmarshal"), n, sp.ptr(p), sp.ptr(out), sp.ptr(st), flags)
        return out, st[:n]

    def msm(self, group: int, scalars, points, flags: int = 0):
        """(out, status): out = sum_i scalars[i] * points[i] as ONE encoded point -- the MSM-shaped call
        sites of the reference (share/poly.go:340-348, 449-476; sign/bdn/bdn.go:126-181).  If any
        status is non-zero the output is all-zero bytes.  flags: F_TRUSTED(0) for points validated before (as every
        kyber.Point of the reference's call sites is), F_UNCOMPRESSED for BLS12-381 uncompressed-affine input."""
        sp = space_of(scalars)
        s, p = sp.rows(scalars, 32), sp.rows(points, self._in_len(group, flags))
        n = s.shape[0]
        if p.shape[0] != n:
            raise ValueError("scalars/points length mismatch")
        out, st = sp.out(self.G1_LEN if group == 1 else self.G2_LEN), sp.status(n)
        sp.call(self._sym(f"g{group}_msm"), n, sp.ptr(s), sp.ptr(p), sp.ptr(out), sp.ptr(st), flags)
        return out, st[:n]

    def poly_eval(self, group: int, commits, indices, flags: int = 0):
        """(out, status): out[i] = sum_j commits[j] * (indices[i] + 1)^j -- share.PubPoly.Eval (share/poly.go:340-348)
        for many indices in one launch (host buffers); status has one entry per commitment."""
        sp = HOST
        c = sp.rows(commits, self._in_len(group, flags))
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
        n, t = idx.shape[0], c.shape[0]
        out, st = sp.out((n, self.G1_LEN if group == 1 else self.G2_LEN)), sp.status(t)
        sp.call(self._sym(f"g{group}_poly_eval"), n, sp.ptr(idx), t, sp.ptr(c), sp.ptr(out), sp.ptr(st), flags)
        return out, st[:t]

    def scalar_poly_eval(self, coeffs, indices):
        """out[i] = sum_j coeffs[j] * (indices[i] + 1)^j mod the group order, 32-byte big-endian scalars (mod.Int) --
        share.PriPoly.Eval (share/poly.go:85-93) for many indices in one launch: PriPoly.Shares (poly.go:96-102).
        Host buffers."""
        sp = HOST
        c = sp.rows(coeffs, 32)
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
        n, t = idx.shape[0], c.shape[0]
        out = sp.out((n, 32))
        sp.call(self._sym("scalar_poly_eval"), n, sp.ptr(idx), t, sp.ptr(c), sp.ptr(out))
        return out

    def g1_msm(self, scalars, points, flags: int = 0):
        return self.msm(1, scalars, points, flags)

    def g2_msm(self, scalars, points, flags: int = 0):
        return self.msm(2, scalars, points, flags)

    def batch_pair(self, g1, g2, flags: int = 0):
        """(gt, status): gt[i] = e(g1[i], g2[i])  (N x Suite.Pair)."""
        sp = space_of(g1)
        a, b = sp.rows(g1, self._in_len(1, flags)), sp.rows(g2, self._in_len(2, flags))
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("g1/g2 length mismatch")
        gt, st = sp.out((n, self.GT_LEN)), sp.status(n)
        sp.call(self._sym("pair"), n, sp.ptr(a), sp.ptr(b), sp.ptr(gt), sp.ptr(st), flags)
        return gt, st[:n]

    def gt_batch_mul(self, scalars, gts):
        """(out, status): out[i] = gts[i] ^ scalars[i]  (N x GT Point.Mul: pairing/bn256/point.go:613,
        kilic/gt.go:79-84)."""
        sp = space_of(scalars)
        s, g = sp.rows(scalars, 32), sp.rows(gts, self.GT_LEN)
        n = s.shape[0]
        if g.shape[0] != n:
            raise ValueError("length mismatch")
        out, st = sp.out(g.shape), sp.status(n)
        sp.call(self._sym("gt_mul"), n, sp.ptr(s), sp.ptr(g), sp.ptr(out), sp.ptr(st))
        return out, st[:n]

    def batch_validate_pairing(self, p1, p2, inv1, inv2, flags: int = 0):
        """(ok, status): ok[i] = e(p1[i], p2[i]) == e(inv1[i], inv2[i])  (N x Suite.ValidatePairing,
        pairing/pairing.go:13-15).  p1/inv1 are G1, p2/inv2 are G2; F_TRUSTED(0..3) refer to p1, p2, inv1, inv2."""
        w1, w2 = self._in_len(1, flags), self._in_len(2, flags)
        sp = space_of(p1)
        a, b, c, d = sp.rows(p1, w1), sp.rows(p2, w2), sp.rows(inv1, w1), sp.rows(inv2, w2)
        n = a.shape[0]
        if not (b.shape[0] == c.shape[0] == d.shape[0] == n):
            raise ValueError("length mismatch")
        ok, st = sp.status(n), sp.status(n)
        sp.call(self._sym("pair_check"), n, sp.ptr(a), sp.ptr(b), sp.ptr(c), sp.ptr(d), sp.ptr(ok), sp.ptr(st), flags)
        return ok[:n], st[:n]

    # ------------------------------------------------------------ sign/bdn: one roster, many masks
    def bdn_terms(self, group: int, roster, flags: int = 0):
        """(coefs, terms, status): what NewMask precomputes for a roster of m keys of `group` (mask.go:51-61) as ONE
        engine call (kyb_<suite>_bdn_terms_g<group>): coefs[j] = hashPointToR's 16 XOF bytes of key j (little-endian
        they are the coefficient c_j, bdn.go:29-63), terms[j] = (c_j + 1) P_j.  status[j] is key j's UnmarshalBinary
        status; if any key is rejected every coefs and terms byte is zero.  flags: 0 or F_TRUSTED(0).  Host buffers or
        torch device tensors; the call runs on the current device."""
        w = self.G1_LEN if group == 1 else self.G2_LEN
        sp = space_of(roster)
        r = sp.rows(roster, w)
        m = r.shape[0]
        if m < 1:
            raise ValueError("empty roster")
        coefs, terms, st = sp.out((m, 16)), sp.out((m, w)), sp.status(m)
        sp.call(self._sym(f"bdn_terms_g{group}"), m, sp.ptr(r), sp.ptr(coefs), sp.ptr(terms), sp.ptr(st), flags)
        return coefs, terms, st[:m]

    def mask_aggregate(self, group: int, points, masks, flags: int = 0):
        """(out, count, status): out[i] = the sum of the points that masks[i] enables, count[i] = their number --
        AggregatePublicKeys over precomputed terms (bdn.go:166-181) for n masks over ONE list of m points as ONE engine
        call (kyb_<suite>_mask_aggregate_g<group>).  masks: a sequence of byte strings of (m + 7) >> 3 bytes each, or an
        (n, stride) uint8 array or tensor whose rows start with the mask; bit j & 7 of byte j >> 3 enables point j and
        bits at or above m are ignored.  If a point is rejected every status[i] is its status and every out[i] zero.
        The memory space is the masks'; the call runs on the current device."""
        w = self.G1_LEN if group == 1 else self.G2_LEN
        sp = space_of(masks)
        p = sp.rows(points, w)
        m = int(p.shape[0])
        if m < 1:
            raise ValueError("empty roster")
        L = (m + 7) >> 3
        if isinstance(masks, (list, tuple)):
            if any(len(x) != L for x in masks):
                raise ValueError("mismatching mask lengths")
            masks = np.frombuffer(b"".join(bytes(x) for x in masks), dtype=np.uint8).reshape(len(masks), L)
        if len(masks.shape) != 2 or masks.shape[1] < L:
            raise ValueError("masks: (n, stride) bytes, stride >= (m + 7) >> 3")
        n, stride = int(masks.shape[0]), int(masks.shape[1])
        mk = sp.rows(masks, stride)
        if sp.is_device:
            import torch

            cnt = torch.empty(n or 1, dtype=torch.int32, device=sp.device)
        else:
            cnt = np.zeros(n or 1, dtype=np.uint32)
        out, st = sp.out((n or 1, w)), sp.status(n)
        sp.call(self._sym(f"mask_aggregate_g{group}"), n, m, sp.ptr(p), sp.ptr(mk), stride, sp.ptr(out), sp.ptr(cnt), sp.ptr(st), flags)
        return out[:n], cnt[:n], st[:n]

    @staticmethod
    def bdn_plan(n: int, m: int):
        """(width, slices): the subset-table width, 4 or 8, and the slices per mask that a mask_aggregate call of n masks
        over m points uses (kyb_bdn_plan; no device is touched)"""
        import ctypes

        from .._lib import check, load

        plan = (ctypes.c_int * 2)()
        check(load().kyb_bdn_plan(int(n), int(m), ctypes.addressof(plan)), "kyb_bdn_plan")
        return int(plan[0]), int(plan[1])

    # ------------------------------------------------------------ kyber interface mirrors
    def make_types(self):
        eng = self
        ORDER = self.ORDER

        class Scalar:
            """mod.Int modulo the group order, 32-byte big-endian wire format (group/mod/int.go:334-350)."""

            __slots__ = ("v",)

            def __init__(self, v: int = 0):
                self.v = v % ORDER

            def MarshalBinary(self) -> bytes:
                return self.v.to_bytes(32, "big")

            def UnmarshalBinary(self, buf: bytes):
                if len(buf) != 32:
                    raise ValueError("UnmarshalBinary: wrong size buffer")
                x = int.from_bytes(buf, "big")
                if x >= ORDER:  # group/mod/int.go:362-364
                    raise ValueError("UnmarshalBinary: value out of range")
                self.v = x
                return self

            def MarshalSize(self) -> int: return 32
            def SetInt64(self, x: int): self.v = x % ORDER; return self
            def SetBytes(self, b: bytes): self.v = int.from_bytes(b, "big") % ORDER; return self
            def Zero(self): return self.SetInt64(0)
            def One(self): return self.SetInt64(1)
            def Set(self, a): self.v = _sc(a).v; return self
            def Clone(self): return Scalar(self.v)
            def Equal(self, a) -> bool: return self.v == _sc(a).v
            def Add(self, a, b): self.v = (_sc(a).v + _sc(b).v) % ORDER; return self
            def Sub(self, a, b): self.v = (_sc(a).v - _sc(b).v) % ORDER; return self
            def Neg(self, a): self.v = -_sc(a).v % ORDER; return self
            def Mul(self, a, b): self.v = _sc(a).v * _sc(b).v % ORDER; return self
            def Inv(self, a): self.v = pow(_sc(a).v, ORDER - 2, ORDER); return self
            def Div(self, a, b): self.v = _sc(a).v * pow(_sc(b).v, ORDER - 2, ORDER) % ORDER; return self

            def Pick(self, rand=None):
                raw = rand(64) if rand is not None else os.urandom(64)
                self.v = int.from_bytes(raw, "big") % ORDER
                return self

            def String(self) -> str: return self.MarshalBinary().hex()
            __repr__ = String

        def _sc(s) -> Scalar:
            if not isinstance(s, Scalar):
                raise TypeError(f"ErrTypeCast: not a {eng.name} scalar")
            return s

        class _Elt:
            """G1/G2 element held as its canonical wire encoding; arithmetic = engine calls."""

            __slots__ = ("enc",)
            GROUP, LEN, BASE, NULL = 0, 0, b"", b""
            ENGINE = eng  # the suite's batch API (sign/bdn's NewMask takes a kyber.Group and needs its engine)

            def __init__(self, enc=None):
                self.enc = self.NULL if enc is None else bytes(enc)

            def MarshalBinary(self) -> bytes: return self.enc
            def MarshalSize(self) -> int: return self.LEN

            def UnmarshalBinary(self, buf: bytes):
                if len(buf) != self.LEN:
                    raise ValueError(f"{eng.name}: wrong size buffer")
                out, st = eng.mul(self.GROUP, (1).to_bytes(32, "big"), buf, False)
                if st[0]:
                    raise ValueError(f"{eng.name}: malformed point" if st[0] == 1 else f"{eng.name}: point not in subgroup")
                self.enc = bytes(out[0])
                return self

            def Null(self): self.enc = self.NULL; return self
            def Base(self): self.enc = self.BASE; return self
            def Set(self, p): self.enc = self._cast(p).enc; return self
            def Clone(self): return type(self)(self.enc)
            def Equal(self, p) -> bool: return self.enc == self._cast(p).enc

            def Add(self, a, b):
                out, st = eng.add(self.GROUP, self._cast(a).enc, self._cast(b).enc)
                if st.any():
                    raise ValueError(f"{eng.name}: invalid point")
                self.enc = bytes(out[0])
                return self

            def Neg(self, a):
                self.enc = eng.neg(self.GROUP, self._cast(a).enc)
                return self

            def Sub(self, a, b):
                nb = type(self)().Neg(b)
                return self.Add(a, nb)

            def Pick(self, rand=None):
                """A uniformly random group element as k * Base (what pairing/bn256/point.go:48-57 does)."""
                return self.Mul(Scalar().Pick(rand), None)

            def Mul(self, s, A=None):
                """Point.Mul, a batch of ONE: ~1-9 ms on the device whatever the batch size (profiles/
                r03_single_call_latency.json) against 0.1-0.3 ms on a CPU core of the reference.  The Go suite keeps
                single elements on the embedded reference (go/kyberhip/suite/point.go, MinDeviceBatch); this mirror
                has no CPU implementation to delegate to -- the product path has no CPU fallback -- so loops belong
                in g1_batch_mul / g1_commit / g1_msm."""
                base = self.BASE if A is None else self._cast(A).enc
                out, st = eng.mul(self.GROUP, _sc(s).MarshalBinary(), base, False)
                if st[0]:
                    raise ValueError(f"{eng.name}: invalid point")
                self.enc = bytes(out[0])
                return self

            def _cast(self, p):
                if type(p) is not type(self):
                    raise TypeError(f"ErrTypeCast: wrong {eng.name} group element")
                return p

            def String(self) -> str: return self.enc.hex()
            __repr__ = String

        class G1Elt(_Elt):
            __slots__ = ()
            GROUP, LEN, BASE, NULL = 1, eng.G1_LEN, eng.G1_BASE, eng.G1_NULL

        class G2Elt(_Elt):
            __slots__ = ()
            GROUP, LEN, BASE, NULL = 2, eng.G2_LEN, eng.G2_BASE, eng.G2_NULL

        class GTElt:
            __slots__ = ("enc",)

            def __init__(self, enc: bytes = b""):
                self.enc = bytes(enc)

            def MarshalBinary(self) -> bytes: return self.enc
            def MarshalSize(self) -> int: return eng.GT_LEN
            def Equal(self, o) -> bool: return self.enc == o.enc

            def Mul(self, s, q):
                out, st = eng.gt_batch_mul(_sc(s).MarshalBinary(), q.enc)
                if st[0]:
                    raise ValueError(f"{eng.name}: invalid GT element")
                self.enc = bytes(out[0])
                return self

            def Pair(self, p1, p2):
                gt, st = eng.batch_pair(p1.enc, p2.enc)
                if st[0]:
                    raise ValueError(f"{eng.name}: invalid pairing input")
                self.enc = bytes(gt[0])
                return self

        class _Group:
            def __init__(self, elt, gname):
                self._elt, self._name = elt, gname

            def String(self): return self._name
            def ScalarLen(self): return 32
            def Scalar(self): return Scalar()
            def PointLen(self): return self._elt.LEN
            def Point(self): return self._elt()

        class Suite:
            """pairing.Suite (pairing/pairing.go:8-20): G1(), G2(), GT(), Pair, ValidatePairing."""

            def G1(self): return _Group(G1Elt, eng.name + ".G1")
            def G2(self): return _Group(G2Elt, eng.name + ".G2")
            def GT(self): return GTElt

            def Pair(self, p1, p2):
                if not isinstance(p1, G1Elt) or not isinstance(p2, G2Elt):
                    raise TypeError("ErrTypeCast")
                return GTElt().Pair(p1, p2)

            def ValidatePairing(self, p1, p2, inv1, inv2) -> bool:
                ok, st = eng.batch_validate_pairing(p1.enc, p2.enc, inv1.enc, inv2.enc)
                if st[0]:
                    raise ValueError(f"{eng.name}: invalid pairing input")
                return bool(ok[0])

        return Scalar, G1Elt, G2Elt, GTElt, Suite
