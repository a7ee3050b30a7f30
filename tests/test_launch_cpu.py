"""lib.marshal / lib.workspace: the host half of lib.launch, which needs no GPU."""
import ctypes

import pytest
import torch

from dlwp_benchmark_amd import lib as L


def test_marshal_maps_each_kind_of_argument():
    t = torch.zeros(4)
    d = L.WAttnDesc()
    ptr, none, ref, i, f, b = L.marshal((t, None, d, 3, 1.5, True))
    assert ptr == t.data_ptr() and none is None
    assert type(ref) is type(ctypes.byref(d)) and ref._obj is d
    assert (i, f, b) == (3, 1.5, True) and type(i) is int and type(f) is float and b is True


def test_marshal_passes_ctypes_values_through():
    handle, arr = ctypes.c_void_p(7), (ctypes.c_int32 * 2)(1, 2)
    ref = ctypes.byref(handle)
    out = L.marshal((handle, arr, ref))
    assert out[0] is handle and out[1] is arr and out[2] is ref


def test_marshal_refuses_other_types_and_names_the_position():
    with pytest.raises(L.DlwpError, match="argument 1 .* list"):
        L.marshal((0, [1, 2]))


def test_workspace():
    assert L.workspace(0, "cpu") is None
    ws = L.workspace(12, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == 12 and ws.element_size() == 1


def test_kept_workspace():
    """the first buffer is exactly what was asked for, a smaller request reuses it, a larger one at least doubles it and leaves
    the replaced buffer referenced where it was (a recorded step keeps its address)"""
    bufs = {}
    first = L.kept_workspace(bufs, 100, "cpu", floor=8)
    assert first.dtype == torch.uint8 and first.numel() == 100 and list(bufs) == ["cpu"]
    ptr = first.data_ptr()
    assert L.kept_workspace(bufs, 50, "cpu", floor=8) is first and len(bufs["cpu"]) == 1
    second = L.kept_workspace(bufs, 150, "cpu", floor=8)
    assert second is bufs["cpu"][-1] and second.numel() >= 200 and len(bufs["cpu"]) == 2
    assert bufs["cpu"][0] is first and first.data_ptr() == ptr and second.data_ptr() != ptr
    third = L.kept_workspace(bufs, 10000, "cpu", floor=8)
    assert third.numel() == 10000 and len(bufs["cpu"]) == 3 and bufs["cpu"][0] is first
    other = L.kept_workspace(bufs, 16, "meta", floor=8)
    assert other.numel() == 16 and len(bufs["meta"]) == 1 and bufs["meta"][0] is other and len(bufs["cpu"]) == 3
    assert L.kept_workspace({}, 1, "cpu", floor=256).numel() == 256
    assert L.kept_workspace({}, 0, "cpu").numel() == 8
