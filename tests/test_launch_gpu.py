"""lib.launch as the wrappers use it: the stream it passes, the device it makes current, and that KernelTimer still sees the
calls.  A recording stand-in takes an entry point's place on the library object the way KernelTimer's wrappers do; it
launches nothing."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import ops

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def recording(*names):
    """[(entry point, arguments, device current inside the call)] of the calls made while it is installed"""
    lib = L.load()
    saved = {name: getattr(lib, name) for name in names}
    calls = []

    def stand_in(name):
        def fn(*args):
            calls.append((name, args, torch.cuda.current_device()))
            return 0
        return fn

    try:
        for name in names:
            setattr(lib, name, stand_in(name))
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def test_launch_uses_the_current_stream():
    dev = torch.device("cuda:0")
    z = torch.randn(64, generator=torch.Generator().manual_seed(0)).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        h = ops.activation(z, 1)
        with recording("dlwp_act_f32") as calls:
            ops.activation(z, 1)
    side.synchronize()
    # the bound tests/test_linear_epilogue_train_gpu.py holds dlwp_act_f32 to
    assert float((h.double().cpu() - F.gelu(z.double().cpu())).abs().max()) <= 2e-6
    (name, args, _), = calls
    assert name == "dlwp_act_f32" and args[-1] == side.cuda_stream
    assert side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    assert args[0] == z.data_ptr() and args[2:4] == (64, 1)


def test_launch_makes_the_tensors_device_current():
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two visible devices, {torch.cuda.device_count()} here")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:1")
    stream = torch.cuda.current_stream(dev).cuda_stream
    seq = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.SiLU(), torch.nn.Linear(8, 8), torch.nn.LayerNorm(8)).to(dev)
    ln = torch.nn.LayerNorm(8).to(dev)
    x, z = torch.zeros(16, 4, device=dev), torch.zeros(64, device=dev)
    packed = ops.MgnMlpWeights()
    with recording("dlwp_mgn_mlp_f32", "dlwp_gc_layernorm_f32", "dlwp_act_f32") as calls:
        for call in (lambda: ops.mgn_mlp(packed, seq, x, 1, 16), lambda: ops.gc_layernorm(z.view(8, 8), 1, 8, ln),
                     lambda: ops.activation(z, 1)):
            call()
            assert torch.cuda.current_device() == 0
    assert [c[0] for c in calls] == ["dlwp_mgn_mlp_f32", "dlwp_gc_layernorm_f32", "dlwp_act_f32"]
    for name, args, current in calls:
        assert current == 1, name
        assert args[-1] == stream, name


def test_kernel_timer_sees_a_launch():
    z = torch.zeros(64, device="cuda:0")
    with L.KernelTimer(names=["dlwp_act_f32"]) as kt:
        ops.activation(z, 1)
    assert kt.summary()[0][("dlwp_act_f32", None)]["calls"] == 1
    assert L.load().dlwp_act_f32.argtypes == L.SIGNATURES["dlwp_act_f32"][1]        # the entry point itself is back
