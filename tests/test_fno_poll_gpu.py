"""Spectrum hand-offs of the fused FNO kernel (fno_trunk.hpp, DESIGN.md sections 4.1 and 4.6 "hand-off polls") at the shapes
where the consumer side of the hand-off takes its other paths.  A consumer polls its block of four 16-byte loads until no
dword it needs is the sentinel; how many polls that takes depends on timing, the values must not: every run of the same call
is bit-equal, and the persistent launch is bit-equal to one launch per step (other launch boundaries, other timing).  What
changed on this path is small -- a wave requests its second mode's weights only if it has a second mode, and the traced wave
counts its polls -- and neither can change a value; the shapes below are the ones the issue for a deeper poll set, kept as
the pin of the hand-off's consumer side whatever its poll loop becomes.

Shapes at which the poll code can go wrong, not the workload's.  W = 64 (the kernel is specialised for it); H = 32 / 64: four /
eight workgroups per sample, i.e. one / two partials per lane in P2.  B = 1 and 3: a sample's workgroups are dealt out in
sequence; B = 9: the first eight samples share XCDs by construction and the last resident group is partial.
n_modes = [4, 4] keeps M1 = 4 rows and M2 = 3 columns of the spectrum: most waves of a workgroup have no P1 / P3 column, only
the first of the four 16-byte blocks of a P3 poll is live (the other three are masked out of the sentinel test), and some
workgroups own fewer than eight modes in P2 (waves without a mode; NO wave has a second mode, so every second-mode weight
request is skipped; at [12, 12] and H = 64 three waves of eight have one, at H = 32 all do).  One layer (the XCC-id check
and the first exchange only) and four; 1, 2 and 5 rollout steps (5: both parities of the exchange buffers are re-armed and
reused several times); both product forms.

The spin bound is not driven here: tests/test_fno_gpu.py holds the timeout and range-guard tests.

Bounds: those of tests/test_fno_proj_loop_gpu.py for the same two comparisons (fused against the unfused kernels, launch form
3; fused against the oracle).  The unfused rollout and the oracle are computed once per shape at five steps; a rollout with
context 1 is a prefix of a longer one from the same first frame, so shorter ones compare against slices.

Every output of these inputs (launch forms 0 and 1, 288 outputs) is byte-equal between this build and a build of the parent
commit loaded through DLWP_HIP_LIB: profiles/poll_ab_bench.txt."""
import copy
import functools

import pytest
import torch

from helpers import fno_std_fn, per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5        # against the oracle: test_fno_proj_loop_gpu.py
TOL_FORMS = 2e-6  # fused against the unfused kernels: test_fno_proj_loop_gpu.py
W, TMAX = 64, 6   # TMAX frames = 5 steps at context 1
HS = [32, 64]
BS = [1, 3, 9]
MODES = [(12, 12), (4, 4)]
LAYERS = [1, 4]
STEPS = [1, 2, 5]
FORMS = ["f16x3", "bf16x6"]
REPEATS = 5


@functools.lru_cache(maxsize=None)
def case(h, b, modes, layers):
    """(oracle trajectory of 5 steps, HIP module on the CPU, TMAX input frames on the device)"""
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    kw = dict(n_modes=list(modes), constant_channels=0, prescribed_channels=0, prognostic_channels=1, hidden_channels=32,
              lifting_channels=32, projection_channels=32, n_layers=layers, context_size=1)
    ref = FNO2DModuleRef(**kw).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(0.85), gain=0.85)
    hip = FNO2DModule(**kw)
    hip.load_state_dict(ref.state_dict())
    _, _, prog = navier_stokes(b, TMAX, h, W)
    with torch.no_grad():
        want = ref(prognostic=prog)
    return want, hip, prog.to(DEV).contiguous()


def module(h, b, modes, layers, form, launch_form):
    _, hip, _ = case(h, b, modes, layers)
    return copy.deepcopy(hip).set_execution_form(precision_form=form, launch_form=launch_form).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def unfused(h, b, modes, layers, form):
    """5 steps on the unfused kernels (launch form 3)"""
    _, _, prog = case(h, b, modes, layers)
    m = module(h, b, modes, layers, form, 3)
    out = m(prognostic=prog)
    m.verify()
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("layers", LAYERS)
@pytest.mark.parametrize("modes", MODES, ids=lambda m: "m%dx%d" % m)
@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("h", HS)
def test_poll(h, b, modes, layers, steps, form):
    want, _, prog6 = case(h, b, modes, layers)
    prog = prog6[:, :steps + 1].contiguous()
    m = module(h, b, modes, layers, form, 0)
    got = m(prognostic=prog)
    m.verify()
    assert got.shape == (b, steps, 1, h, W)
    assert torch.isfinite(got).all()
    assert m.lift_table_state() != 0, "not on the fused step kernel"
    # how many polls a hand-off takes depends on timing; the values do not
    for i in range(REPEATS):
        again = m(prognostic=prog)
        m.verify()
        assert torch.equal(again, got), f"repeat {i + 1} differs from the first run"
    assert m.fused_timeouts() == 0 and m.range_reruns() == 0
    # the persistent launch equals one launch per step bit for bit
    ms = module(h, b, modes, layers, form, 1)
    stepwise = ms(prognostic=prog)
    ms.verify()
    assert torch.equal(stepwise, got)
    assert ms.fused_timeouts() == 0 and ms.range_reruns() == 0
    # the unfused kernels and the oracle
    eu = per_step_rel_l2(got, unfused(h, b, modes, layers, form)[:, :steps])
    eo = per_step_rel_l2(got, want[:, :steps])
    print(f"H {h} B {b} modes {modes} L {layers} steps {steps} {form}: vs unfused {max(eu):.2e}  vs oracle {max(eo):.2e}")
    assert max(eu) <= TOL_FORMS, f"fused vs unfused: per-step rel L2 {['%.2e' % e for e in eu]}"
    assert max(eo) <= TOL, f"fused vs oracle: per-step rel L2 {['%.2e' % e for e in eo]}"
