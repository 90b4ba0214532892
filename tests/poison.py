"""Poisoned allocations: make "this kernel read memory nobody wrote" a visible, testable event.

The autograd Functions of ``mr_gnas_amd`` take their outputs and workspaces from ``torch.empty``, ``torch.empty_like``,
``torch.empty_strided`` and ``Tensor.new_empty``; none is initialised.  A test process starts on freshly mapped device memory, which
is zero -- the one value that lets a forgotten accumulator initialisation, an unwritten padding row or an unwritten workspace slot
come out right.  ``poisoned(monkeypatch, pattern)`` wraps the four calls for the length of a ``with`` block and fills what they
return, on the current stream, before the caller sees it.

The wrapper acts only when BOTH hold:
  * the calling frame's module (``sys._getframe(1).f_globals["__name__"]``) is ``mr_gnas_amd`` or below it: torch's own Python code
    and the tests' own allocations are left alone;
  * the result is a floating-point tensor or a ``uint8`` tensor (the byte workspaces of ``functional._base._ws``).
Integer-typed tensors are returned as allocated: they are index structures and are not poisoned.

Patterns (two, because ``x > best`` ignores a NaN and a sum does not ignore a large finite value):
  "nan"    floats NaN; uint8 0xFF bytes (NaN read as float32 / float64, -1 read as a signed integer)
  "huge"   float32 3e38, float64 1e306, float16 6e4, bfloat16 3e38; uint8 0x7F bytes (3.39e38 as float32, about 1.4e306 as float64)
  "clean"  zeros: the reference run

``skip_bytes``: call sites whose BYTE workspaces are left as allocated, each "module" or "module:function" of the first frame outside
``functional._base`` (``_ws`` and ``_chunk_plan_args`` are helpers, the site is their caller).  Meant for a workspace whose integer
content a kernel reads as an index: poisoning it would send the kernel out of bounds instead of showing a value dependence.  The
graph and sampler builders are in the default: their workspaces are the temporary storage of integer sorts and scans.

The block yields a ``Fills`` record: how many tensors and bytes were filled (a case asserts the count is above zero, so a path that
stopped allocating through these calls is noticed) and how many byte workspaces were skipped.

Not for use inside ``torch.cuda.graph`` capture."""
import contextlib
import sys

import torch

PACKAGE = "mr_gnas_amd"
HELPERS = ("mr_gnas_amd.functional._base",)
SKIP_BYTES_DEFAULT = ("mr_gnas_amd.graph", "mr_gnas_amd.sampler")
PATTERNS = ("nan", "huge", "clean")
HUGE = {torch.float32: 3e38, torch.float64: 1e306, torch.float16: 6e4, torch.bfloat16: 3e38}
BYTE = {"nan": 0xFF, "huge": 0x7F}


class Fills:
    """What one ``poisoned`` block filled."""

    def __init__(self):
        self.tensors = 0
        self.bytes = 0
        self.skipped = 0

    def __repr__(self):
        return f"Fills(tensors={self.tensors}, bytes={self.bytes}, skipped={self.skipped})"


def in_package(name):
    return name == PACKAGE or name.startswith(PACKAGE + ".")


def _site(frame):
    """(module, function) of the first frame at or above `frame` that is not one of the workspace helpers."""
    while frame is not None and frame.f_globals.get("__name__") in HELPERS:
        frame = frame.f_back
    if frame is None:
        return "", ""
    return frame.f_globals.get("__name__", ""), frame.f_code.co_name


def _fill(t, pattern, fills, frame, skip_bytes):
    if not isinstance(t, torch.Tensor):
        return t
    if t.dtype == torch.uint8:
        mod, fn = _site(frame)
        if mod in skip_bytes or f"{mod}:{fn}" in skip_bytes:
            fills.skipped += 1
            return t
        if pattern == "clean":
            t.zero_()
        else:
            t.fill_(BYTE[pattern])
    elif t.dtype.is_floating_point:
        if pattern == "clean":
            t.zero_()
        elif pattern == "nan":
            t.fill_(float("nan"))
        else:
            t.fill_(HUGE.get(t.dtype, float(torch.finfo(t.dtype).max) / 2))
    else:
        return t
    fills.tensors += 1
    fills.bytes += t.numel() * t.element_size()
    return t


@contextlib.contextmanager
def poisoned(monkeypatch, pattern, skip_bytes=SKIP_BYTES_DEFAULT):
    """Fill every float / uint8 tensor that code of the package allocates uninitialised inside the block; yields the Fills record.
    Everything is restored when the block ends, also by an exception."""
    if pattern not in PATTERNS:
        raise ValueError(f"pattern {pattern!r}: one of {PATTERNS}")
    skip_bytes = frozenset(skip_bytes)
    fills = Fills()

    def wrap(orig):
        def wrapper(*args, **kwargs):
            out = orig(*args, **kwargs)
            frame = sys._getframe(1)
            if not in_package(frame.f_globals.get("__name__", "")):
                return out
            return _fill(out, pattern, fills, frame, skip_bytes)
        wrapper.__name__ = getattr(orig, "__name__", "empty")
        wrapper.__wrapped__ = orig
        return wrapper

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", wrap(torch.empty))
        m.setattr(torch, "empty_like", wrap(torch.empty_like))
        m.setattr(torch, "empty_strided", wrap(torch.empty_strided))
        m.setattr(torch.Tensor, "new_empty", wrap(torch.Tensor.new_empty))
        yield fills
