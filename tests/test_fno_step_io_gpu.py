"""Step I/O of the persistent FNO rollout kernel ("step I/O"): the kernel forms a step's input table,
residual and output slot on the device, each only where it is read -- a step fed from registers (no constants, no prescribed
channels, context 1) forms the output slot alone, every other step builds the table in four fixed slots (constants, prescribed
window, prognostic frames still taken from the input, frames already produced; an absent part is a slot of zero channels).

The cross-check is the table fno_rollout_once builds on the host: launch_form=1 runs the same kernel one step per launch with
that table, so a persistent launch (launch_form=0) must be bit-equal to it for every (constants, prescribed, context,
prognostic) combination -- the same loads from the same addresses feed the same arithmetic.  Every equality asserted here also
holds on a build of the commit before the change (the file was run against it once through DLWP_HIP_LIB: 12 passed).

Geometry: B = 2, 32 x 64 (four workgroups per sample, eight in all), 8 frames, the widths of NS_KW of test_fno_gpu.py."""
import copy
import functools
import os

import pytest
import torch

from helpers import fno_std_fn, per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
H, W, B, T = 32, 64, 2, 8
NS_KW = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
             hidden_channels=32, lifting_channels=256, projection_channels=256, n_layers=4, context_size=1)
# (constants, prescribed, context, prognostic)
FED_1, FED_3 = (0, 0, 1, 1), (0, 0, 1, 3)   # fed from registers from step 1 on
WINDOW = (0, 0, 2, 1)                       # not fed: step 0 reads the input, step 1 one frame of each, later steps produced frames
ALL_FOUR = (2, 1, 3, 2)                     # every slot populated, 2 + (1 + 2) * 3 = 11 input channels
COMBOS = [FED_1, FED_3, WINDOW, ALL_FOUR]


@functools.lru_cache(maxsize=None)
def case(combo):
    """(oracle, HIP module on the CPU: copy it and choose execution forms before the first call, inputs on the device)"""
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes, weatherbench
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    nc, npr, ctx, ng = combo
    kw = dict(NS_KW, constant_channels=nc, prescribed_channels=npr, context_size=ctx, prognostic_channels=ng)
    gain = 0.7 if nc or npr else 0.85   # the gains test_fno_gpu.py uses for the two kinds of input
    ref = FNO2DModuleRef(**kw).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(gain), gain=gain)
    hip = FNO2DModule(**kw)
    hip.load_state_dict(ref.state_dict())
    if nc or npr:
        cpu = weatherbench(B, T, H, W, prognostic_channels=ng, constant_channels=nc, prescribed_channels=npr)
    else:
        cpu = navier_stokes(B, T, H, W, channels=ng)
    names = ("constants", "prescribed", "prognostic")
    inputs = {k: (None if t is None else t.to(DEV).contiguous()) for k, t in zip(names, cpu)}
    return ref, hip, dict(zip(names, cpu)), inputs


def _on(hip, **form):
    m = copy.deepcopy(hip)
    if form:
        m.set_execution_form(**form)
    return m.to(DEV).eval()


DEFAULT_FORM = "f16x3"


@functools.lru_cache(maxsize=None)
def _persistent(combo, form):
    # a cached reference is the DEFAULT kernel path: never create one while a debug switch of the plan is set
    assert "DLWP_FNO_FEED_REGS" not in os.environ
    _, hip, _, inputs = case(combo)
    m = _on(hip, precision_form=form)
    out = m(**inputs)
    m.verify()
    assert m.fused_timeouts() == 0 and m.range_reruns() == 0
    return out


def persistent(combo, form=DEFAULT_FORM):
    """the whole rollout as one persistent launch on the default (fed where eligible) path; one cache entry per (combo, form)
    however it is called; never modified by the tests that share it"""
    return _persistent(combo, form)


@pytest.mark.parametrize("form", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("combo", COMBOS)
def test_persistent_launch_equals_step_by_step_launches(combo, form):
    """launch_form=1: one launch per step, the step's table, residual and output slot from the host."""
    _, hip, _, inputs = case(combo)
    stepwise = _on(hip, precision_form=form, launch_form=1)
    want = stepwise(**inputs)
    got = persistent(combo, form)
    assert got.shape == (B, T - combo[2], combo[3], H, W)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_table_path_in_every_step_equals_the_fed_path(monkeypatch):
    """DLWP_FNO_FEED_REGS=0 (read when the plan is created): every step of the persistent launch builds its table and loads
    its input and residual from memory -- the frames the fed path kept in registers."""
    want = persistent(FED_1)   # the fed reference, created BEFORE the switch is set
    _, hip, _, inputs = case(FED_1)
    monkeypatch.setenv("DLWP_FNO_FEED_REGS", "0")
    unfed = _on(hip)
    got = unfed(**inputs)
    unfed.verify()
    assert torch.equal(got, want)


@pytest.mark.parametrize("combo", [FED_1, ALL_FOUR])
def test_ranges_equal_the_whole_rollout(combo):
    """[0, 2), [2, 3), [3, K): the last range is a persistent launch whose step 0 already reads frames from `out` only, the
    middle one a single step (not persistent)."""
    _, hip, _, inputs = case(combo)
    whole = persistent(combo)
    k = whole.shape[1]
    m = _on(hip)
    out = torch.full_like(whole, float("nan"))
    for lo, hi in ((0, 2), (2, 3), (3, k)):
        m.rollout_into(out, inputs["constants"], inputs["prescribed"], inputs["prognostic"], lo, hi)
    m.verify()
    assert torch.equal(out, whole)


def test_all_four_segments_match_the_oracle():
    ref, _, cpu, _ = case(ALL_FOUR)
    with torch.no_grad():
        want = ref(**cpu)
    errs = per_step_rel_l2(persistent(ALL_FOUR), want)
    assert max(errs) <= TOL, f"per-step rel L2 {['%.2e' % e for e in errs]}"
