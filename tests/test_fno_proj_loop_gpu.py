"""Projection loop of the fused FNO step kernel (proj_segment, DESIGN.md section 4.6 "projection loop"): every loop-carried
value lives in one register set -- the layer-1 accumulators are rewritten in place by the next tile's matrix instructions, the
GELU outputs of pixels 0-1 are consumed in the same trip and those of pixels 2-3 in the next one, the LDS operands are
re-read into the registers they were just used from.  The prologue therefore does layer 2 of pixels 0-1 of tile 0 and the
epilogue layer 2 of pixels 2-3 of the last tile.

Shapes: the smallest at which each edge of that loop is taken, not the workload's.  Width 64 (the kernel is specialised for
it), height 32 (four workgroups per sample at eight rows), B = 2, hidden 32, lifting 32, two layers, three rollout steps.
projection_channels = 16 x tiles: 1 tile (the loop body never runs: prologue + epilogue alone), 2, 3 (odd) and the headline's
16.  1, 2 and 3 prognostic channels -> the layer-2 FMAs built for 1, 2 and 4 outputs (3 channels: one padded output).

All of them take the fused step kernel: step_eligible (fno_trunk.hpp) asks for W = 64, eight rows per workgroup (H = 32 ->
4 workgroups), <= 4 input channels per step, lifting % 32 == 0, widths <= 256 and <= 4 outputs, none of which depends on the
projection width or on 1-3 prognostic channels.  With ONE input channel the plan says so itself: it considers the lifting
table only when step_eligible holds, so lift_table_state() != 0 is asserted there.  launch_form 1 runs the same kernel one
step per launch (bit-equal by construction of the kernel); launch_form 3 runs the unfused kernels, whose projection
(pw_proj_bf16x6_kernel) goes through the same proj_segment with the bf16x6 products.

The arithmetic did not change with the loop: every output of these inputs (launch forms 0, 1 and 3, lifting table on and off)
was compared once with a build of the commit before the change, loaded through DLWP_HIP_LIB, and is byte-equal to it."""
import copy
import functools

import pytest
import torch

from helpers import fno_std_fn, per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5        # against the oracle: test_fno_gpu.py
TOL_FORMS = 2e-6  # HIP path against HIP cross-check path: test_fno_gpu.py (bf16x6 vs fp32_mfma, f16x3 vs bf16x6)
H, W, B, T = 32, 64, 2, 4
KW = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, hidden_channels=32, lifting_channels=32,
          n_layers=2, context_size=1)
PROJ = [16, 32, 48, 256]
NPROG = [1, 2, 3]
FORMS = ["f16x3", "bf16x6"]


@functools.lru_cache(maxsize=None)
def case(proj, nprog):
    """(oracle trajectory, HIP module on the CPU: copy it and choose execution forms before the first call, input on the device)"""
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    kw = dict(KW, projection_channels=proj, prognostic_channels=nprog)
    ref = FNO2DModuleRef(**kw).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(0.85), gain=0.85)
    hip = FNO2DModule(**kw)
    hip.load_state_dict(ref.state_dict())
    _, _, prog = navier_stokes(B, T, H, W, channels=nprog)
    with torch.no_grad():
        want = ref(prognostic=prog)
    return want, hip, prog.to(DEV).contiguous()


def run(proj, nprog, form, launch_form):
    """one rollout on a fresh module; returns (output, module)"""
    _, hip, prog = case(proj, nprog)
    m = copy.deepcopy(hip).set_execution_form(precision_form=form, launch_form=launch_form).to(DEV).eval()
    out = m(prognostic=prog)
    m.verify()
    return out, m


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nprog", NPROG)
@pytest.mark.parametrize("proj", PROJ)
def test_projection_loop(proj, nprog, form):
    want, _, prog = case(proj, nprog)
    got, m = run(proj, nprog, form, 0)
    assert got.shape == (B, T - 1, nprog, H, W)
    assert torch.isfinite(got).all()
    if nprog == 1:
        assert m.lift_table_state() != 0, "not on the fused step kernel"
    # two runs are bit-identical
    again = m(prognostic=prog)
    m.verify()
    assert torch.equal(again, got)
    assert m.fused_timeouts() == 0 and m.range_reruns() == 0
    # the persistent launch equals one launch per step bit for bit
    stepwise, ms = run(proj, nprog, form, 1)
    assert torch.equal(stepwise, got)
    assert ms.fused_timeouts() == 0 and ms.range_reruns() == 0
    # the unfused kernels and the oracle
    unfused, _ = run(proj, nprog, form, 3)
    eu = per_step_rel_l2(got, unfused)
    eo = per_step_rel_l2(got, want)
    es = per_step_rel_l2(unfused, want)
    print(f"proj {proj} nprog {nprog} {form}: vs unfused {max(eu):.2e}  vs oracle {max(eo):.2e}  unfused vs oracle {max(es):.2e}")
    assert max(eu) <= TOL_FORMS, f"fused vs unfused: per-step rel L2 {['%.2e' % e for e in eu]}"
    assert max(eo) <= TOL, f"fused vs oracle: per-step rel L2 {['%.2e' % e for e in eo]}"
    assert max(es) <= TOL, f"unfused vs oracle: per-step rel L2 {['%.2e' % e for e in es]}"
