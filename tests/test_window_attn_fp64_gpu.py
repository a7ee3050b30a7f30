"""The window-attention forward kernels (csrc/window_attn.hip, window_attn2.hip, window_attn3.hip) against an independent
float64 reference (tests/window_attn_ref.py: the reference's own pad / roll / window_partition / attention sequence, built from
the fixture-pinned geometry helpers of oracle/restate).  The three kernels share csrc/window_attn_desc.hpp, so comparing them
with each other cannot see an error there; this file can.  Case tables, inputs and the restated host rules:
tests/test_window_attn_ref_cpu.py.

Tolerances come from the references, never from the kernels:
  fp32-accurate forms  rel-L2 <= max(2e-6, 4 floor), and per token max_t |got_t - want_t| / |want_t| <= max(1e-5, 4 floor_t),
                       where floor / floor_t are the same two figures of training.window_attention_torch evaluated in fp32 on
                       the CPU on the same inputs: what fp32 arithmetic costs at this input (2e-6 is the suite's bound for the
                       operator; 4 allows another summation order and v_exp_f32).  The per-token figure catches a single
                       mis-routed or mis-masked token, which a global norm dilutes.
  bf16 form            1e-6 < rel-L2 <= min(2e-2, 3 emu), emu = the rel-L2 of the reference with bf16-rounded operands
                       (q, k, v and the un-normalised probabilities); 3 covers rounding in another order than the emulation.
"""
import ctypes
import functools

import pytest
import torch

import test_window_attn_ref_cpu as C
from helpers import rel_l2

pytestmark = pytest.mark.gpu

F32_FORMS = ("fp32_mfma", "bf16x6", "fp32")


def per_token(a, want):
    """max over tokens of |a_t - want_t|_2 / |want_t|_2 (float64, t over batch x tokens)"""
    a, want = a.detach().double().cpu(), want.detach().double().cpu()
    return float(((a - want).norm(dim=-1) / want.norm(dim=-1)).max())


def _bounds(spec, qkv, bias, table, want, want16):
    """the reference-derived figures of one case: (fp32 floor, fp32 per-token floor, bf16 emulation error)"""
    from dlwp_benchmark_amd import training

    f32 = training.window_attention_torch(qkv.float(), bias.float(), table.float(), spec)
    assert f32.dtype == torch.float32 and not f32.is_cuda
    return rel_l2(f32, want), per_token(f32, want), (rel_l2(want16, want) if want16 is not None else None)


@functools.lru_cache(maxsize=None)
def _swin(case, shifted):
    qkv, bias, table = C.swin_inputs(case)
    spec = C.swin_spec(case, shifted)
    want = C.swin_reference(case, shifted, qkv, table)
    want16 = C.swin_reference(case, shifted, qkv, table, operands="bf16")
    return spec, (qkv, bias, table), want, _bounds(spec, qkv, bias, table, want, want16)


@functools.lru_cache(maxsize=None)
def _pangu(case, shifted):
    qkv, bias, table = C.pangu_inputs(case)
    spec = C.pangu_spec(case, shifted)[0]
    want = C.pangu_reference(case, shifted, qkv, bias, table)
    want16 = C.pangu_reference(case, shifted, qkv, bias, table, operands="bf16")
    return spec, (qkv, bias, table), want, _bounds(spec, qkv, bias, table, want, want16)


def _covered(spec, batch, bf16):
    from dlwp_benchmark_amd import lib as L

    dsc = spec.to_c()
    dsc.form = -1 if bf16 else 1
    return L.load().dlwp_window_attn_workspace_bytes(ctypes.byref(dsc), batch, 1 if bf16 else 0) > 0


def _check_f32(tag, got, want, floor, floor_t, failures):
    assert torch.isfinite(got).all(), tag
    e, et = rel_l2(got, want), per_token(got, want)
    tol, tol_t = max(2e-6, 4 * floor), max(1e-5, 4 * floor_t)
    print("%-44s rel-L2 %.2e (<= %.2e, floor %.2e)  per token %.2e (<= %.2e, floor %.2e)" % (tag, e, tol, floor, et, tol_t, floor_t))
    if not e <= tol:
        failures.append((tag, "rel-L2", e, tol))
    if not et <= tol_t:
        failures.append((tag, "per token", et, tol_t))


def _check_bf16(tag, got16, want, emu, failures):
    assert torch.isfinite(got16).all(), tag
    e, tol = rel_l2(got16, want), min(2e-2, 3 * emu)
    print("%-44s rel-L2 %.2e (1e-6 < . <= %.2e, emulation %.2e)" % (tag, e, tol, emu))
    if not 1e-6 < e <= tol:
        failures.append((tag, "bf16 rel-L2", e, tol))


def _run_case(name, path, spec, inputs, want, bounds):
    """every precision of one descriptor against the float64 reference; all figures are printed before anything is asserted"""
    from dlwp_benchmark_amd import ops

    floor, floor_t, emu = bounds
    qkv, bias, table = (t.cuda() for t in inputs)
    b = qkv.shape[0]
    fast = path != "gen"
    assert _covered(spec, b, False) == fast and _covered(spec, b, True) == fast, "the case does not run on the kernel its table names"
    failures = []
    for prec in F32_FORMS:
        if prec == "bf16x6" and path == "k2":
            got, fb = ops.window_attention(qkv, bias, table, spec, precision=prec, count_fallbacks=True)
            assert fb == 0, (name, "exponent-slack fallbacks", fb)
        else:
            got = ops.window_attention(qkv, bias, table, spec, precision=prec)
        torch.cuda.synchronize()
        # (the fp32-MFMA form is the generic kernel whatever the descriptor)
        _check_f32(f"{name} {'gen' if prec == 'fp32_mfma' else path} {prec}", got, want, floor, floor_t, failures)
    got16 = ops.window_attention(qkv, bias, table, spec, precision="bf16")
    torch.cuda.synchronize()
    _check_bf16(f"{name} {path} bf16", got16, want, emu, failures)
    assert not failures, failures


@pytest.mark.parametrize("p", C.SWIN_PARAMS, ids=C.case_id)
def test_swin_windows_match_the_fp64_reference(p):
    """bias_mode 0.  On a fast-path case "fp32_mfma" is the generic kernel (PREC 0) and "bf16x6" / "fp32" / "bf16" are kernel 2;
    on a generic case the four precisions are PREC 0, 2, by size, and 1 of the generic kernel."""
    case, shifted = p
    _run_case(C.case_id(p), C.SWIN_CASES[case][shifted], *_swin(case, shifted))


@pytest.mark.parametrize("p", C.PANGU_PARAMS, ids=C.case_id)
def test_earth_windows_match_the_fp64_reference(p):
    """bias_mode 1: the nine plans of kernel 3, and the descriptors it declines on the generic kernel."""
    case, shifted = p
    _run_case(C.case_id(p), C.PANGU_CASES[case][0], *_pangu(case, shifted))


@pytest.mark.parametrize("shifted", [False, True])
def test_exponent_slack_fallback_matches_the_fp64_reference(shifted):
    """The inputs of test_exponent_slack_fallback_is_exact (logits up to ~300): fp32 arithmetic itself costs ~2.6e-5 here
    (the floor), so the same rule gives a bound of about 1e-4."""
    from dlwp_benchmark_amd import ops

    spec, qkv, bias, table, want = C.slack_case(shifted)
    floor, floor_t, _ = _bounds(spec, qkv, bias, table, want, None)
    qkv, bias, table = qkv.cuda(), bias.cuda(), table.cuda()
    failures = []
    got, fb = ops.window_attention(qkv, bias, table, spec, precision="bf16x6", count_fallbacks=True)
    torch.cuda.synchronize()
    assert fb > 0, "the adversarial logits did not trigger the exact fallback"
    _check_f32(f"slack shifted={shifted} k2 bf16x6", got, want, floor, floor_t, failures)
    got = ops.window_attention(qkv, bias, table, spec, precision="fp32_mfma")
    _check_f32(f"slack shifted={shifted} gen fp32_mfma", got, want, floor, floor_t, failures)
    assert not failures, failures


def test_earth_window_large_logits_match_the_fp64_reference():
    """The inputs of test_earth_window_kernel_large_logits (logits in the hundreds, rolled and padded)."""
    from dlwp_benchmark_amd import ops

    spec, qkv, bias, table, want = C.earth_large_logits_case()
    floor, floor_t, _ = _bounds(spec, qkv, bias, table, want, None)
    assert _covered(spec, 1, False)
    qkv, bias, table = qkv.cuda(), bias.cuda(), table.cuda()
    failures = []
    for prec in ("bf16x6", "fp32_mfma"):
        got = ops.window_attention(qkv, bias, table, spec, precision=prec)
        torch.cuda.synchronize()
        _check_f32(f"earth large logits {prec}", got, want, floor, floor_t, failures)
    assert not failures, failures
