"""Table path of the fused FNO step kernel (one input channel) against the oracle and against the exact
path (lift_table off) of the same kernel: wiring, accuracy at every input scale, the out-of-domain fallback, determinism and
the launch forms.  Smallest fused geometry (32 x 64: four workgroups per sample), B = 2, three steps; one case at 64 x 64, B = 3."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import fno_std_fn, per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
H, W, B, FRAMES = 32, 64, 2, 4
NS_KW = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
             hidden_channels=32, lifting_channels=256, projection_channels=256, n_layers=4, context_size=1)


def _pair(zero_bias=False, w1_scale=1.0):
    """(oracle, HIP module on the CPU: copy it and choose execution forms before the first call)"""
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    ref = FNO2DModuleRef(**NS_KW).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(0.85), gain=0.85)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if zero_bias and (n.endswith("bias") or ".bias" in n):
                p.zero_()
            if n == "fno.lifting.fcs.0.weight":
                p.mul_(w1_scale)
    hip = FNO2DModule(**NS_KW)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


def _on(hip, **form):
    m = copy.deepcopy(hip)
    if form:
        m.set_execution_form(**form)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _field():
    from dlwp_benchmark_amd.synthetic import navier_stokes

    return navier_stokes(B, FRAMES, H, W)[2]


@functools.lru_cache(maxsize=None)
def _case(scale, zero_bias):
    """oracle trajectory of a scaled field, computed once per (scale, zero_bias)"""
    ref, hip = _pair(zero_bias)
    prog = _field() * scale
    with torch.no_grad():
        want = ref(prognostic=prog)
    return hip, prog, want


def test_table_is_wired_and_can_be_switched_off():
    hip, prog, want = _case(1.0, False)
    tab, exact = _on(hip), _on(hip, lift_table=False)
    assert tab.lift_table_state() == 0                    # no plan yet
    a, b = tab(prognostic=prog.to(DEV)), exact(prognostic=prog.to(DEV))
    assert tab.lift_table_state() == 1 and exact.lift_table_state() == 3
    assert not torch.equal(a, b)                          # the two paths round differently somewhere
    assert max(per_step_rel_l2(a, want)) <= TOL and max(per_step_rel_l2(b, want)) <= TOL
    wide = _on(hip, launch_form=3)
    wide(prognostic=prog.to(DEV))
    assert wide.lift_table_state() == 0                   # the unfused kernels stay exact: the independent cross-check


@pytest.mark.parametrize("form", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("zero_bias", [False, True])
@pytest.mark.parametrize("scale", [1.0, 1e-2, 1e-4])
def test_table_path_is_not_measurably_worse_than_the_exact_path(scale, zero_bias, form):
    hip, prog, want = _case(scale, zero_bias)
    tab, exact = _on(hip, precision_form=form), _on(hip, precision_form=form, lift_table=False)
    a, b = tab(prognostic=prog.to(DEV)), exact(prognostic=prog.to(DEV))
    assert tab.lift_table_state() == 1 and exact.lift_table_state() == 3 and tab.range_reruns() == 0
    ea, eb = max(per_step_rel_l2(a, want)), max(per_step_rel_l2(b, want))
    print(f"scale {scale:g} zero_bias {zero_bias} {form}: table {ea:.3e}, exact {eb:.3e}")
    assert eb <= TOL and ea <= TOL, (ea, eb)
    assert ea <= 2.0 * eb + 2e-7, (ea, eb)


def test_rows_outside_the_domain_fall_back_to_the_exact_lifting():
    ref, hip = _pair()
    prog = _field().clone()
    for r in (3, 17, 30):                                 # three rows of sample 0 reach |x| = 40 > 32; sample 1 stays inside
        prog[0, 0, 0, r] *= 40.0 / prog[0, 0, 0, r].abs().max()
    assert prog[1].abs().max() < 32 and torch.isfinite(prog).all()
    with torch.no_grad():
        want = ref(prognostic=prog)
    tab = _on(hip)
    got = tab(prognostic=prog.to(DEV))
    assert tab.lift_table_state() == 1 and tab.range_reruns() == 0
    e = per_step_rel_l2(got, want)
    print("fallback rows: per-step rel-L2", ["%.2e" % v for v in e])
    assert max(e) <= TOL, e
    alone = _on(hip)(prognostic=prog[1:2].to(DEV))
    assert torch.equal(alone[0], got[1])                  # the decision is per row: other samples do not see it


def test_table_path_is_deterministic_at_64x64():
    from dlwp_benchmark_amd.synthetic import navier_stokes

    ref, hip = _pair()
    prog = navier_stokes(3, 7, 64, 64)[2]
    with torch.no_grad():
        want = ref(prognostic=prog)
    tab = _on(hip)
    first = tab(prognostic=prog.to(DEV))
    assert tab.lift_table_state() == 1
    assert max(per_step_rel_l2(first, want)) <= TOL
    for _ in range(4):
        assert torch.equal(tab(prognostic=prog.to(DEV)), first)


def test_step_by_step_launches_match_the_persistent_launch_bitwise():
    hip, prog, want = _case(1.0, False)
    a, b = _on(hip), _on(hip, launch_form=1)
    ya, yb = a(prognostic=prog.to(DEV)), b(prognostic=prog.to(DEV))
    assert a.lift_table_state() == 1 and b.lift_table_state() == 1
    assert torch.equal(ya, yb)
    x = prog[:, 0].to(DEV)
    step = a.one_step(x) + x                              # one_step: the same kernel without the residual
    assert float(torch.linalg.vector_norm(step - ya[:, 0]) / torch.linalg.vector_norm(ya[:, 0])) <= 1e-6


def _rejected_scale():
    """the first power-of-two scale of the lifting's first layer at which the plan-time guard rejects the table"""
    from dlwp_benchmark_amd import lib as L

    ref, _ = _pair()
    sd = ref.state_dict()
    w1 = sd["fno.lifting.fcs.0.weight"].reshape(256).float().contiguous()
    b1, b2 = sd["fno.lifting.fcs.0.bias"].float().contiguous(), sd["fno.lifting.fcs.1.bias"].float().contiguous()
    w2 = sd["fno.lifting.fcs.1.weight"].reshape(32, 256).float().contiguous()
    tab = np.zeros(2 * 32 * 16 * 6 * 32, dtype=np.float32)
    for k in range(1, 13):
        w = (w1 * 2.0 ** k).contiguous()
        ok = ctypes.c_int32(-1)
        L.check(L.load().dlwp_fno2d_lift_table_build(w.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), 256, 32, 4,
                                                     tab.ctypes.data, tab.size, None, ctypes.byref(ok)))
        if ok.value == 0:
            return 2.0 ** k
    raise AssertionError("the guard accepted every scale up to 2^12")


def test_weights_the_guard_rejects_run_on_the_exact_path():
    ref, hip = _pair(w1_scale=_rejected_scale())
    prog = _field()
    with torch.no_grad():
        want = ref(prognostic=prog)
    m = _on(hip)
    got = m(prognostic=prog.to(DEV))
    assert m.lift_table_state() == 2
    assert max(per_step_rel_l2(got, want)) <= TOL
