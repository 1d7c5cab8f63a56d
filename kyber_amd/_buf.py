"""The one place that knows host memory from device memory.

A batch wrapper picks its memory space once, ``sp = space_of(x)``, and is then written once against it:

  sp.rows(x, width)   (n, width) contiguous uint8 view of an input (bytes / numpy / tensor)
  sp.msgs(x, what)    (buf, n, len) of n equal-length messages
  sp.out(shape)       output buffer
  sp.status(n)        status / verdict buffer of max(n, 1) bytes; the caller returns [:n]
  sp.ptr(x)           its address, None for None
  sp.call(name, ...)  the host space calls ``name``, the device space ``name + "_dev"`` with the current stream appended

HOST serves bytes, numpy arrays and CPU tensors; Device serves CUDA tensors, enqueues on the current stream and leaves
its results on the device.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, load


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _on_device(x) -> bool:
    return type(x).__module__.startswith("torch") and x.is_cuda


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def stream_handle(stream):
    """the raw handle of a torch stream (a raw handle passes through)"""
    return getattr(stream, "cuda_stream", stream)


def _host(buf, width: int) -> np.ndarray:
    a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf, dtype=np.uint8)
    return np.ascontiguousarray(a).reshape(-1, width)


def pack_equal_msgs(msgs, what: str = "batch"):
    """(buf, n, len) of n equal-length messages: a list of byte strings or an (n, len) uint8 array.  An empty buffer
    becomes one dummy byte, so that the native call never sees a NULL message pointer."""
    if isinstance(msgs, (list, tuple)):
        ln = len(msgs[0]) if msgs else 0
        if any(len(x) != ln for x in msgs):
            raise ValueError(f"{what}: messages must have equal length")
        n, buf = len(msgs), np.frombuffer(b"".join(msgs), dtype=np.uint8)
    else:
        a = np.ascontiguousarray(msgs, dtype=np.uint8)
        n, ln = a.shape[0], a.shape[1]
        buf = a.reshape(-1)
    return (buf if buf.size else np.zeros(1, dtype=np.uint8)), n, ln


def pack_msgs(msgs):
    """(blob, offsets) of a sequence of byte strings of any lengths, the layout of kyb_ed25519_verify's msgs / msg_off"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    blob = b"".join(bytes(m) for m in msgs)
    return (np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, dtype=np.uint8)), off


def dst_arg(dst):
    """a domain separation tag as the const void * of the C ABI (the pointer keeps its buffer alive); NULL when empty"""
    dst = bytes(dst)
    return ctypes.cast(ctypes.create_string_buffer(dst, len(dst)), ctypes.c_void_p) if dst else None


class _Host:
    is_device = False
    rows = staticmethod(_host)
    msgs = staticmethod(pack_equal_msgs)

    @staticmethod
    def out(shape):
        return np.zeros(shape, dtype=np.uint8)

    @staticmethod
    def status(n: int):
        return np.zeros(n or 1, dtype=np.uint8)

    @staticmethod
    def ptr(x):
        return None if x is None else x.__array_interface__["data"][0]  # (x.ctypes.data, without building x.ctypes)

    @staticmethod
    def call(name: str, *args) -> None:
        check(getattr(load(), name)(*args), name)


HOST = _Host()


class Device:
    is_device = True

    def __init__(self, device):
        self.device = device

    def rows(self, x, width: int):
        if not _is_torch(x):  # (bytes next to device tensors: a default base, one key, one message)
            import torch

            x = torch.from_numpy(_host(x, width).copy())
        if not x.is_cuda:
            x = x.to(self.device)
        return x.contiguous().view(-1, width)

    @staticmethod
    def msgs(x, what: str = "batch"):
        m = x.contiguous()
        return m, m.shape[0], m.shape[1]

    def out(self, shape):
        import torch

        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def status(self, n: int):
        return self.out(n or 1)

    @staticmethod
    def ptr(x):
        return None if x is None else x.data_ptr()

    @staticmethod
    def call(name: str, *args) -> None:
        name += "_dev"
        check(getattr(load(), name)(*args, _stream()), name)


def space_of(x):
    return Device(x.device) if _on_device(x) else HOST
