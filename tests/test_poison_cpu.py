"""tests/poison.py pinned on the CPU (the harness does the same on CPU tensors): what it fills and what it leaves, that it restores
the four calls, its counter, and why BOTH patterns are run -- two deliberately wrong pure-torch functions, one that only a large
finite value shows and one that both patterns show."""
import math
import types

import pytest
import torch

import poison
from poison import poisoned

SRC = """
import torch

def empty(*a, **k):
    return torch.empty(*a, **k)

def empty_like(t, **k):
    return torch.empty_like(t, **k)

def empty_strided(size, stride, **k):
    return torch.empty_strided(size, stride, **k)

def new_empty(t, *a, **k):
    return t.new_empty(*a, **k)

def ws(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8)

def wrong_sum(x):
    # accumulates into an uninitialised buffer: right only on zeroed memory
    acc = torch.empty(x.shape[1], dtype=x.dtype)
    for r in x:
        acc += r
    return acc

def wrong_max(x):
    # a running maximum over an uninitialised buffer, taken as a kernel takes it: fmaxf / v_max_f32 return the operand that is not
    # a NaN.  Right on memory that holds nothing above the data (zeros under positive data) and on NaN
    best = torch.empty(x.shape[1], dtype=x.dtype)
    for r in x:
        best = torch.fmax(best, r)
    return best

def right_max(x):
    best = torch.empty(x.shape[1], dtype=x.dtype)
    best.copy_(x[0])
    for r in x[1:]:
        best = torch.fmax(best, r)
    return best
"""


def module_named(name):
    m = types.ModuleType(name)
    exec(compile(SRC, name.replace(".", "/") + ".py", "exec"), m.__dict__)
    return m


INSIDE = module_named("mr_gnas_amd.functional.fake")
ROOT = module_named("mr_gnas_amd")
OUTSIDE = module_named("somewhere.else")
LOOKALIKE = module_named("mr_gnas_amd_tools.x")           # shares the prefix as a string, is not the package
HELPER = module_named("mr_gnas_amd.functional._base")     # the workspace helper: the site is ITS caller


def four_calls(mod, dtype):
    like = torch.ones(3, 5, dtype=dtype)
    return [mod.empty(3, 5, dtype=dtype), mod.empty_like(like), mod.empty_strided((3, 5), (5, 1), dtype=dtype), mod.new_empty(like, (3, 5))]


def all_equal(t, value):
    if isinstance(value, float) and math.isnan(value):
        return bool(torch.isnan(t).all())
    return bool((t == value).all())


@pytest.mark.parametrize("pattern,dtype,value", [
    ("nan", torch.float32, float("nan")), ("nan", torch.float64, float("nan")), ("nan", torch.bfloat16, float("nan")), ("nan", torch.uint8, 0xFF),
    ("huge", torch.float32, 3e38), ("huge", torch.float64, 1e306), ("huge", torch.uint8, 0x7F),
    ("clean", torch.float32, 0.0), ("clean", torch.float64, 0.0), ("clean", torch.uint8, 0),
])
def test_package_allocations_are_filled(monkeypatch, pattern, dtype, value):
    want = torch.tensor(value, dtype=dtype).item() if not (isinstance(value, float) and math.isnan(value)) else value
    for mod in (INSIDE, ROOT):
        with poisoned(monkeypatch, pattern) as fills:
            got = four_calls(mod, dtype)
        assert all(t.shape == (3, 5) and t.dtype == dtype for t in got)
        assert all(all_equal(t, want) for t in got), (pattern, dtype, got)
        assert fills.tensors == 4 and fills.bytes == 4 * 15 * torch.empty(0, dtype=dtype).element_size() and fills.skipped == 0


def test_byte_patterns_read_as_the_issue_says(monkeypatch):
    """0xFF bytes are NaN as float32 / float64 and -1 as a signed integer; 0x7F bytes are 3.39e38 as float32, about 1.4e306 as float64."""
    with poisoned(monkeypatch, "nan"):
        w = INSIDE.ws(64)
    assert bool(torch.isnan(w.view(torch.float32)).all()) and bool(torch.isnan(w.view(torch.float64)).all())
    assert bool((w.view(torch.int32) == -1).all()) and bool((w.view(torch.int64) == -1).all())
    with poisoned(monkeypatch, "huge"):
        w = INSIDE.ws(64)
    f32, f64 = float(w.view(torch.float32)[0]), float(w.view(torch.float64)[0])
    assert 3.39e38 < f32 < 3.40e38 and 1.38e306 < f64 < 1.40e306
    assert int(w.view(torch.int32)[0]) == 0x7F7F7F7F


@pytest.mark.parametrize("pattern", ["nan", "huge", "clean"])
def test_other_callers_are_left_alone(monkeypatch, pattern):
    torch.manual_seed(0)
    with poisoned(monkeypatch, pattern) as fills:
        for mod in (OUTSIDE, LOOKALIKE):
            for dtype in (torch.float32, torch.uint8):
                for t in four_calls(mod, dtype):
                    t.fill_(7)                                   # (still writable, still the caller's)
        mine = torch.empty(4, 4)                                 # this test module's own allocation
        mine.fill_(1.0)
        torch.nn.Linear(4, 4)                                    # torch's own Python code allocates its parameters with torch.empty
    assert fills.tensors == 0 and fills.bytes == 0


def test_nothing_is_written_to_foreign_memory(monkeypatch):
    """A tensor allocated elsewhere is returned as allocated: recycle a block that holds a known value and look at it."""
    probe = torch.full((1 << 12,), 5.0)
    ptr = probe.data_ptr()
    del probe
    with poisoned(monkeypatch, "nan"):
        again = OUTSIDE.empty(1 << 12)
    if again.data_ptr() == ptr:                                  # the allocator handed the same block back (it does; not required);
        assert bool((again[64:] == 5.0).all())                   # free() keeps its list links in the block's first bytes


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.int16, torch.int8, torch.bool])
def test_integer_tensors_are_untouched(monkeypatch, dtype):
    for pattern in ("nan", "huge", "clean"):
        with poisoned(monkeypatch, pattern) as fills:
            got = four_calls(INSIDE, dtype)
        assert all(t.dtype == dtype for t in got)
        assert fills.tensors == 0 and fills.bytes == 0


def test_restored_on_exit_and_after_an_exception(monkeypatch):
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with poisoned(monkeypatch, "nan"):
        assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned(monkeypatch, "huge"):
            assert torch.empty_like is not before[1]
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    assert not bool(torch.isnan(INSIDE.empty(8).fill_(0.0)).any())
    with pytest.raises(ValueError):
        with poisoned(monkeypatch, "zero"):
            pass
    assert torch.empty is before[0]


def test_blocks_nest_and_unwind(monkeypatch):
    before = torch.empty
    with poisoned(monkeypatch, "clean") as outer:
        with poisoned(monkeypatch, "nan") as inner:
            t = INSIDE.empty(4)
        assert bool(torch.isnan(t).all()) and inner.tensors == 1
        u = INSIDE.empty(4)
        assert bool((u == 0).all())
    assert torch.empty is before and outer.tensors >= 1


def test_fill_counter(monkeypatch):
    with poisoned(monkeypatch, "huge") as fills:
        INSIDE.empty(10, dtype=torch.float32)            # 40 bytes
        INSIDE.empty(3, dtype=torch.float64)             # 24
        INSIDE.ws(100)                                   # 100
        INSIDE.empty(7, dtype=torch.int32)               # not counted
        OUTSIDE.empty(9)                                 # not counted
        INSIDE.empty(0)                                  # a tensor, no bytes
    assert (fills.tensors, fills.bytes, fills.skipped) == (4, 164, 0)
    assert "tensors=4" in repr(fills)


def test_skip_bytes_names_the_call_site(monkeypatch):
    """A byte workspace is skipped by the module, or module:function, of the first frame outside functional._base; floats of the
    same site are still filled."""
    caller = module_named("mr_gnas_amd.evaluation")
    caller.helper = HELPER
    exec("def ranks(n):\n    return helper.ws(n)\ndef other(n):\n    return helper.ws(n)\n", caller.__dict__)
    for skip, ranks_filled, other_filled in (((), True, True), (("mr_gnas_amd.evaluation",), False, False),
                                             (("mr_gnas_amd.evaluation:ranks",), False, True), (("mr_gnas_amd.functional._base",), True, True)):
        with poisoned(monkeypatch, "clean") as _:
            caller.ranks(32).fill_(9)
        with poisoned(monkeypatch, "nan", skip_bytes=skip) as fills:
            a, b, f = caller.ranks(32), caller.other(32), caller.empty(4)
        assert bool((a == 0xFF).all()) == ranks_filled and bool((b == 0xFF).all()) == other_filled, skip
        assert bool(torch.isnan(f).all())
        assert fills.skipped == (not ranks_filled) + (not other_filled) and fills.tensors == 1 + ranks_filled + other_filled
    assert set(poison.SKIP_BYTES_DEFAULT) == {"mr_gnas_amd.graph", "mr_gnas_amd.sampler"}


# ---- why two patterns ---------------------------------------------------------------------------------------------------------------
def verdicts(fn, x, monkeypatch):
    """{pattern: does fn(x) under that pattern equal fn(x) under "clean", bit for bit and finite}."""
    with poisoned(monkeypatch, "clean") as fills:
        ref = fn(x)
    assert fills.tensors > 0
    out = {}
    for pattern in ("nan", "huge"):
        with poisoned(monkeypatch, pattern) as fills:
            got = fn(x)
        assert fills.tensors > 0
        out[pattern] = bool(torch.isfinite(got).all()) and torch.equal(got, ref)
    return ref, out


def test_both_patterns_are_needed(monkeypatch):
    x = torch.rand(9, 6, generator=torch.Generator().manual_seed(3)) + 0.5          # positive data
    # a sum into an uninitialised accumulator: the zero-filled reference is right by construction, both patterns show the bug
    ref, ok = verdicts(INSIDE.wrong_sum, x, monkeypatch)
    assert torch.allclose(ref, x.sum(0)) and ok == {"nan": False, "huge": False}
    # a running maximum over an uninitialised buffer: a NaN in the buffer is dropped by the first fmax, 3e38 is never exceeded
    ref, ok = verdicts(INSIDE.wrong_max, x, monkeypatch)
    assert torch.equal(ref, x.max(0).values)                     # zeros below positive data: the clean run is right
    assert ok == {"nan": True, "huge": False}                    # "nan" does not see it, "huge" does
    # and the correct function passes under both
    ref, ok = verdicts(INSIDE.right_max, x, monkeypatch)
    assert torch.equal(ref, x.max(0).values) and ok == {"nan": True, "huge": True}
