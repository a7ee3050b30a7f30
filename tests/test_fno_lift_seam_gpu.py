"""Step seam of the fused FNO rollout kernel with a live lifting table: the exact lifting MLP's weights
are staged only in a step in which some wave of a workgroup falls back to it (a workgroup vote through an LDS flag).

The fallback input makes rows leave the table's domain (+-32) at LATER steps of a persistent launch, in workgroups (8 rows) that
stage, stop staging for three steps and stage again, and in which falling-back and table waves mix in every proportion; the
pattern is computed from the oracle trajectory and asserted.  Geometry of test_fno_lift_table_gpu.py (32 x 64, B = 2, four
workgroups per sample), 6 steps; the no-fallback cases use the plain field, one of them at 64 x 64, B = 3 (G = 8, the headline's
group size).

Not compared: the table model against the lift_table=False model on the row-steps outside the domain.  Such a row's lifting is
the same arithmetic in both models, but its OUTPUT is not: the spectral layers mix every row of the sample, and the other rows
were lifted from the table in one model and exactly in the other, so the two outputs differ by the table's rounding from the
first step on -- the comparison is not well defined."""
import copy
import functools

import pytest
import torch

from helpers import fno_std_fn, per_step_rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
RANGE = 32.0                       # the table's domain (kLiftTabRange)
H, W, B, ROWS = 32, 64, 2, 8
NS_KW = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1,
             hidden_channels=32, lifting_channels=256, projection_channels=256, n_layers=4, context_size=1)
FORMS = ["f16x3", "bf16x6"]


def _pair(proj_bias=None):
    """(oracle, HIP module on the CPU: copy it and choose execution forms before the first call)"""
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    ref = FNO2DModuleRef(**NS_KW).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(0.85), gain=0.85)
    if proj_bias is not None:
        with torch.no_grad():
            dict(ref.named_parameters())["fno.projection.fcs.1.bias"].fill_(proj_bias)
    hip = FNO2DModule(**NS_KW)
    hip.load_state_dict(ref.state_dict())
    return ref, hip


def _on(hip, **form):
    m = copy.deepcopy(hip)
    if form:
        m.set_execution_form(**form)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def fallback_case():
    """(HIP module, input, oracle trajectory, rows outside the domain [B, steps, H] of the oracle's step inputs)"""
    from dlwp_benchmark_amd.synthetic import navier_stokes

    ref, hip = _pair(proj_bias=-9.0)
    prog = navier_stokes(B, 7, H, W)[2].clone()
    prog[0, 0, 0, 5] = 0.5 * prog[0, 0, 0, 5] + 38
    prog[1, 0, 0] -= 4 * (torch.arange(H) % 8)[:, None].to(prog.dtype)
    with torch.no_grad():
        want = ref(prognostic=prog)
    x_in = torch.cat([prog[:, :1], want[:, :-1]], dim=1)[:, :, 0]          # [B, steps, H, W]: what each step lifts
    row_max = x_in.abs().amax(dim=-1)
    return hip, prog, want, row_max


@functools.lru_cache(maxsize=None)
def plain_case():
    from dlwp_benchmark_amd.synthetic import navier_stokes

    ref, hip = _pair()
    prog = navier_stokes(B, 4, H, W)[2]
    with torch.no_grad():
        want = ref(prognostic=prog)
    return hip, prog, want


def test_the_fallback_input_exercises_the_vote_at_later_steps():
    _, prog, want, row_max = fallback_case()
    assert torch.isfinite(want).all() and want.abs().max() < 100          # far inside the f16 range
    assert ((row_max - RANGE).abs() > 0.05).all(), "a row decides within 0.05 of the domain's edge"
    outside = ~(row_max < RANGE)                                          # [B, steps, H]: the kernel's predicate, per row
    per_wg = outside.reshape(B, outside.shape[1], H // ROWS, ROWS).sum(-1)   # falling-back waves per workgroup
    for b in range(B):
        print(f"sample {b}: rows outside per workgroup, by step:", per_wg[b].tolist())
    mixed = (per_wg > 0) & (per_wg < ROWS)
    assert mixed[:, 1:].any(), "no step >= 1 with table and exact waves in one workgroup"
    stages = (per_wg > 0).permute(0, 2, 1).reshape(-1, per_wg.shape[1]).tolist()   # per workgroup: does it stage, by step
    assert any(any(s[i] and not s[k] and s[m] for i in range(len(s)) for k in range(i + 1, len(s)) for m in range(k + 1, len(s)))
               for s in stages), "no workgroup stages, stops staging and stages again"


@pytest.mark.parametrize("form", FORMS)
def test_rows_that_leave_the_domain_at_later_steps(form):
    hip, prog, want, _ = fallback_case()
    x = prog.to(DEV)
    m = _on(hip, precision_form=form)
    got = m(prognostic=x)
    assert m.lift_table_state() == 1 and m.range_reruns() == 0
    e = per_step_rel_l2(got, want)
    print(f"{form}: per-step rel-L2", ["%.2e" % v for v in e])
    assert max(e) <= TOL, e
    assert torch.equal(m(prognostic=x), got)                              # a second run of the same call
    assert m.range_reruns() == 0
    stepwise = _on(hip, precision_form=form, launch_form=1)
    assert torch.equal(stepwise(prognostic=x), got)                       # one launch per step: every step votes as a step 0
    assert stepwise.lift_table_state() == 1 and stepwise.range_reruns() == 0
    alone = _on(hip, precision_form=form)(prognostic=prog[1:2].to(DEV))
    assert torch.equal(alone[0], got[1])                                  # the vote is per workgroup: other samples do not see it


@pytest.mark.parametrize("form", FORMS)
def test_no_fallback_launch_forms_agree_bitwise(form):
    hip, prog, want = plain_case()
    a, b = _on(hip, precision_form=form), _on(hip, precision_form=form, launch_form=1)
    ya, yb = a(prognostic=prog.to(DEV)), b(prognostic=prog.to(DEV))
    assert a.lift_table_state() == 1 and b.lift_table_state() == 1 and a.range_reruns() == 0
    assert max(per_step_rel_l2(ya, want)) <= TOL
    assert torch.equal(ya, yb)
    x = prog[:, 0].to(DEV)
    step = a.one_step(x) + x                                              # one_step: the same kernel without the residual
    assert float(torch.linalg.vector_norm(step - ya[:, 0]) / torch.linalg.vector_norm(ya[:, 0])) <= 1e-6


def test_no_fallback_is_deterministic_at_the_headline_group_size():
    from dlwp_benchmark_amd.synthetic import navier_stokes

    ref, hip = _pair()
    prog = navier_stokes(3, 7, 64, 64)[2]                                 # 64 rows: G = 8 workgroups per sample, 6 steps
    with torch.no_grad():
        want = ref(prognostic=prog)
    m = _on(hip)
    first = m(prognostic=prog.to(DEV))
    assert m.lift_table_state() == 1 and m.range_reruns() == 0
    assert max(per_step_rel_l2(first, want)) <= TOL
    for _ in range(4):
        assert torch.equal(m(prognostic=prog.to(DEV)), first)
