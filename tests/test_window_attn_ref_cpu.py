"""The case tables of the fp64 window-attention tests (tests/test_window_attn_fp64_gpu.py), checked on the CPU:

* training.window_attention_torch -- the differentiable restatement the backward tests differentiate -- equals the
  independent float64 reference (tests/window_attn_ref.py) at every geometry of the tables, in float64;
* the tables reach the kernels they claim.  plan2 / plan3 / generic_variant restate the host rules (wattn2::make_plan in
  csrc/window_attn2.hip, wattn3::make_plan3 in csrc/window_attn3.hip, launch_wattn in csrc/window_attn.hip; the first two on
  the Desc that normalise_desc of csrc/window_attn_desc.hpp fills, ordered by select_path of csrc/window_attn.hip); the GPU
  tests and tests/test_window_attn_host_cpu.py assert the same coverage again with dlwp_window_attn_workspace_bytes, so a
  stale restatement cannot hide a miss.
"""
import dataclasses
import functools

import pytest
import torch

import window_attn_ref as R
from helpers import rel_l2

# ---------------------------------------------------------------------------------------------------------------------
# the tables.  path: "k2" csrc/window_attn2.hip, "k3" csrc/window_attn3.hip, "gen" the generic kernel of csrc/window_attn.hip
# ---------------------------------------------------------------------------------------------------------------------
# (h, w, wh, ww, heads, d) -> (path unshifted, path shifted)
SWIN_CASES = {
    (8, 32, 8, 32, 2, 8): ("k2", "k2"),            # N = 256, SUB 2, one window
    (16, 64, 8, 32, 2, 16): ("k2", "k2"),          # 4 windows, shifted mask across windows
    (8, 32, 4, 16, 2, 24): ("k2", "gen"),          # N = 64, SUB 1; the shifted boundary cuts a 16-key block
    (32, 64, 32, 64, 2, 24): ("k2", "k2"),         # N = 2048, SUB 4
    (32, 64, 32, 64, 1, 48): ("k2", "k2"),         # head_dim 48, SUB forced to 2
    (12, 64, 6, 32, 2, 48): ("k2", "k2"),          # N = 192, SUB 1
    (24, 96, 12, 48, 2, 24): ("k2", "gen"),        # window width 48, N = 576
    (12, 20, 6, 10, 2, 32): ("gen", "gen"),        # N = 60, SUB 1, LON4 off, ragged tile
    (14, 24, 7, 12, 2, 64): ("gen", "gen"),        # N = 84, SUB 2, head_dim 64
    (10, 36, 10, 18, 1, 8): ("gen", "gen"),        # N = 180, SUB 3, LON4 off
    (15, 34, 15, 17, 2, 16): ("gen", "gen"),       # N = 255, SUB 4, ragged in queries and keys
    (16, 36, 16, 36, 2, 24): ("gen", "gen"),       # N = 576 >= 512, SUB 2
}
# (grid, window, head_dim) -> (path, (RP, PP, PB) or None); rolled as well wherever a roll exists (all of window // 2 non-zero)
PANGU_CASES = {
    ((1, 16, 32), (2, 6, 12), 32): ("k3", (1, 1, 5)),
    ((1, 10, 17), (2, 5, 7), 32): ("k3", (1, 1, 3)),
    ((1, 9, 30), (2, 3, 10), 32): ("k3", (1, 1, 2)),
    ((2, 12, 24), (2, 6, 12), 32): ("k3", (2, 0, 5)),
    ((2, 11, 13), (2, 5, 7), 32): ("k3", (2, 0, 3)),
    ((4, 8, 16), (2, 4, 8), 32): ("k3", (2, 0, 2)),
    ((2, 12, 24), (1, 6, 12), 32): ("k3", (1, 0, 5)),       # no roll exists (spl = 0)
    ((1, 10, 16), (1, 5, 8), 32): ("k3", (1, 0, 3)),        # no roll exists
    ((1, 8, 16), (1, 4, 8), 32): ("k3", (1, 0, 2)),         # no roll exists
    ((3, 7, 13), (2, 6, 12), 32): ("gen", None),            # mixed real and padded planes, padded on every axis
    ((1, 16, 32), (2, 6, 12), 16): ("gen", None),           # Pangu's narrow heads never reach kernel 3
}
PANGU_HEADS = 2
BATCH = 2


def pangu_rolls(window):
    return all(w // 2 for w in window)


SWIN_PARAMS = [(c, s) for c in SWIN_CASES for s in (False, True)]
PANGU_PARAMS = [(c, s) for c in PANGU_CASES for s in ((False, True) if pangu_rolls(c[1]) else (False,))]


def case_id(p):
    case, shifted = p
    flat = [v for part in case for v in (part if isinstance(part, tuple) else (part,))]
    return "x".join(str(v) for v in flat) + ("-shifted" if shifted else "")


# ---------------------------------------------------------------------------------------------------------------------
# descriptors and inputs (CPU tensors; the GPU tests move them)
# ---------------------------------------------------------------------------------------------------------------------
def swin_spec(case, shifted):
    from test_window_attn_gpu import _sub_window_spec

    return _sub_window_spec(*case, shifted)[0]


def pangu_spec(case, shifted):
    from test_window_attn_gpu import _earth_spec

    grid, window, d = case
    spec, rows, types = _earth_spec(grid, window, PANGU_HEADS, shifted)
    if d != 32:
        spec = dataclasses.replace(spec, head_dim=d, scale=d ** -0.5)
    return spec, rows, types


@functools.lru_cache(maxsize=None)
def swin_inputs(case):
    h, w, wh, ww, heads, d = case
    g = torch.Generator().manual_seed(1000 + list(SWIN_CASES).index(case))
    qkv = torch.randn(BATCH, h * w, 3, heads, d, generator=g)
    qkv[:, :, :2] *= 2.0
    bias = torch.randn(3 * heads * d, generator=g) * 0.1
    table = torch.randn((2 * wh - 1) * (2 * ww - 1), heads, generator=g) * 0.5
    return qkv.reshape(BATCH, h * w, 3 * heads * d), bias, table


@functools.lru_cache(maxsize=None)
def pangu_inputs(case):
    grid, window, d = case
    _, rows, types = pangu_spec(case, False)
    heads = PANGU_HEADS
    g = torch.Generator().manual_seed(2000 + list(PANGU_CASES).index(case))
    ltok = grid[0] * grid[1] * grid[2]
    qkv = torch.randn(BATCH, ltok, 3, heads, d, generator=g)
    qkv[:, :, :2] *= 1.5
    bias = torch.randn(3 * heads * d, generator=g) * 0.3
    table = torch.randn(rows, types, heads, generator=g) * 0.5
    return qkv.reshape(BATCH, ltok, 3 * heads * d), bias, table


def swin_reference(case, shifted, qkv, table, operands="fp64"):
    h, w, wh, ww, heads, d = case
    return R.ref_swin(qkv, table, h, w, (wh, ww), (wh // 2, ww // 2) if shifted else (0, 0), heads, d, operands=operands)


def pangu_reference(case, shifted, qkv, bias, table, heads=PANGU_HEADS, operands="fp64"):
    grid, window, d = case
    shift = tuple(w // 2 for w in window) if shifted else (0, 0, 0)
    return R.ref_pangu(qkv, bias, table, grid, window, shift, heads, d, operands=operands)


# the adversarial inputs of tests/test_window_attn_gpu.py, rebuilt on the CPU
def slack_case(shifted):
    """test_exponent_slack_fallback_is_exact: logits that climb by hundreds of binades along the key order"""
    from test_window_attn_gpu import _spec

    h, w, heads, d = 16, 32, 2, 24
    spec, rows = _spec(h, w, heads, d, shifted)
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(1, h * w, 3, heads, d, generator=g)
    bias = torch.randn(3 * heads * d, generator=g) * 0.1
    table = torch.randn(rows, heads, generator=g) * 0.5
    n = h * w
    ramp = torch.linspace(0.0, 1.0, n).view(1, n, 1, 1)
    c = torch.ones(d) / d ** 0.5
    qkv[:, :, 0] = c * 6.0
    qkv[:, :, 1] = c * (ramp * 250.0)
    qkv = qkv.reshape(1, n, 3 * heads * d)
    want = R.ref_swin(qkv, table, h, w, (h, w), (h // 2, w // 2) if shifted else (0, 0), heads, d)
    return spec, qkv, bias, table, want


def earth_large_logits_case():
    """test_earth_window_kernel_large_logits: q, k x 6 and a bias table of +-20"""
    from test_window_attn_gpu import _earth_spec

    grid, window = (1, 16, 32), (2, 6, 12)
    spec, rows, types = _earth_spec(grid, window, 2, True)
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(1, 512, 3, 2, 32, generator=g)
    qkv[:, :, :2] *= 6.0
    qkv = qkv.reshape(1, 512, 192)
    bias = torch.randn(192, generator=g) * 0.3
    table = torch.randn(rows, types, 2, generator=g) * 20.0
    want = R.ref_pangu(qkv, bias, table, grid, window, (1, 3, 6), 2, 32)
    return spec, qkv, bias, table, want


# ---------------------------------------------------------------------------------------------------------------------
# the host rules, restated
# ---------------------------------------------------------------------------------------------------------------------
def plan2(spec):
    """wattn2::make_plan (csrc/window_attn2.hip): None when the 2-D fast kernel declines the descriptor, else its SUB
    (64 SUB queries per workgroup)."""
    if spec.bias_mode != 0 or spec.grid[0] != 1 or spec.window[0] != 1 or spec.padded[0] != 1:
        return None
    if tuple(spec.padded) != tuple(spec.grid) or any(spec.pad_lead):
        return None
    lat, lon, wlat, wlon = spec.grid[1], spec.grid[2], spec.window[1], spec.window[2]
    if wlat <= 0 or wlon <= 0 or lat % wlat or lon % wlon or wlon % 16:
        return None
    n, d = wlat * wlon, spec.head_dim
    if n % 64 or n > 16384 or d not in (8, 16, 24, 48):
        return None
    if spec.use_mask and any(b < lon and b % 16 for b in (spec.mask_b1[2], spec.mask_b2[2])):
        return None          # a longitude region boundary inside a 16-key block
    sub = 4 if (n >= 2048 and n % 256 == 0) else (2 if (n >= 256 and n % 128 == 0) else 1)
    return 2 if (d == 48 and sub == 4) else sub


def plan3(spec):
    """wattn3::make_plan3 (csrc/window_attn3.hip): None when the earth-window kernel declines the descriptor, else (RP, PP, PB):
    real planes and padded planes per window, 16-key blocks per plane."""
    if spec.bias_mode != 1 or spec.head_dim != 32 or spec.heads <= 0:
        return None
    wpl, wlat, wlon = spec.window
    if not 1 <= wpl <= 2 or wlat < 1 or wlon < 1 or wlat * wlon > 80:
        return None
    for g, p, w, lead in zip(spec.grid, spec.padded, spec.window, spec.pad_lead):
        if g <= 0 or p <= 0 or p % w or p < g + lead or lead < 0:
            return None
    ppl, npl = spec.padded[0], spec.padded[0] // wpl
    sf0 = spec.shift_fwd[0] % ppl
    real = [sum(0 <= (ipl * wpl + z + sf0) % ppl - spec.pad_lead[0] < spec.grid[0] for z in range(wpl)) for ipl in range(npl)]
    if min(real) == wpl:
        rp, pp = wpl, 0
    elif wpl == 2 and npl == 1 and real == [1]:
        rp, pp = 1, 1
    else:
        return None
    npq = wlat * wlon
    pb = 2 if npq <= 32 else (3 if npq <= 48 else 5)
    if spec.use_mask:          # at most two cut window rows and two cut window columns
        inside = lambda b, lo, n: lo < b < lo + n
        for axis in (1, 2):
            w = spec.window[axis]
            cut = sum(inside(spec.mask_b1[axis], r * w, w) or inside(spec.mask_b2[axis], r * w, w)
                      for r in range(spec.padded[axis] // w))
            if cut > 2:
                return None
    return rp, pp, pb


def generic_variant(spec):
    """launch_wattn (csrc/window_attn.hip): (SUB, LON4) of the generic kernel"""
    n = spec.window[0] * spec.window[1] * spec.window[2]
    sub = 2 if n >= 512 else (1 if n <= 64 else (2 if n <= 128 else (3 if n <= 192 else 4)))
    return sub, spec.window[2] % 4 == 0


def path(spec):
    return "k2" if plan2(spec) is not None else ("k3" if plan3(spec) is not None else "gen")


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_reach_the_kernels_they_claim():
    sub2, dims2, gen, plans = set(), set(), [], set()
    for (case, shifted) in SWIN_PARAMS:
        spec = swin_spec(case, shifted)
        assert path(spec) == SWIN_CASES[case][shifted], (case, shifted)
        if path(spec) == "k2":
            sub2.add(plan2(spec))
            dims2.add(spec.head_dim)
        else:
            gen.append(spec)
    for (case, shifted) in PANGU_PARAMS:
        spec, _, _ = pangu_spec(case, shifted)
        want_path, want_plan = PANGU_CASES[case]
        assert path(spec) == want_path and plan3(spec) == want_plan, (case, shifted, plan3(spec))
        if want_path == "k3":
            plans.add((want_plan, bool(spec.use_mask)))
        else:
            gen.append(spec)
    assert sub2 == {1, 2, 4} and dims2 == {8, 16, 24, 48}
    nine = {(rp, pp, pb) for rp, pp in ((1, 1), (2, 0), (1, 0)) for pb in (5, 3, 2)}
    assert {p for p, _ in plans} == nine
    assert all((p, rolled) in plans for p in nine if p[:2] != (1, 0) for rolled in (False, True))
    assert {generic_variant(s)[0] for s in gen} == {1, 2, 3, 4}
    assert {generic_variant(s)[1] for s in gen} == {False, True}
    assert {s.head_dim for s in gen} >= {32, 64}
    assert {s.head_dim for s in gen if s.bias_mode == 0} >= {32, 64}                 # ... on 2-D windows
    n_of = lambda s: s.window[0] * s.window[1] * s.window[2]
    assert any(n_of(s) % 32 for s in gen)                                            # ragged last key tile
    assert any(n_of(s) % (64 * generic_variant(s)[0]) for s in gen)                  # ragged last query block
    assert any(n_of(s) >= 512 for s in gen)
    assert any(s.bias_mode == 1 and tuple(s.padded) != tuple(s.grid) for s in gen)   # padded earth-bias descriptor
    assert any(s.bias_mode == 1 and s.use_mask for s in gen)
    # the mixed-plane case: kernel 3 declines it for its planes (one window level is real, the other half padded), not for its head_dim
    spec, _, _ = pangu_spec(((3, 7, 13), (2, 6, 12), 32), False)
    assert all(p > g for p, g in zip(spec.padded, spec.grid)) and all(spec.pad_lead[1:])


@pytest.mark.parametrize("p", SWIN_PARAMS, ids=case_id)
def test_swin_restatement_equals_the_reference_in_fp64(p):
    from dlwp_benchmark_amd import training

    case, shifted = p
    qkv, bias, table = (t.double() for t in swin_inputs(case))
    want = swin_reference(case, shifted, qkv, table)
    got = training.window_attention_torch(qkv, bias, table, swin_spec(case, shifted))
    assert got.dtype == torch.float64 and want.dtype == torch.float64 and got.shape == want.shape
    e = rel_l2(got, want)
    print(case_id(p), "restatement vs reference, fp64: %.2e" % e)
    assert e <= 1e-12


@pytest.mark.parametrize("p", PANGU_PARAMS, ids=case_id)
def test_pangu_restatement_equals_the_reference_in_fp64(p):
    from dlwp_benchmark_amd import training

    case, shifted = p
    qkv, bias, table = (t.double() for t in pangu_inputs(case))
    want = pangu_reference(case, shifted, qkv, bias, table)
    got = training.window_attention_torch(qkv, bias, table, pangu_spec(case, shifted)[0])
    assert got.dtype == torch.float64 and want.dtype == torch.float64 and got.shape == want.shape
    e = rel_l2(got, want)
    print(case_id(p), "restatement vs reference, fp64: %.2e" % e)
    assert e <= 1e-12


def test_large_logit_restatement_equals_the_reference_in_fp64():
    from dlwp_benchmark_amd import training

    cases = [slack_case(False), slack_case(True), earth_large_logits_case()]
    for spec, qkv, bias, table, want in cases:
        got = training.window_attention_torch(qkv.double(), bias.double(), table.double(), spec)
        assert rel_l2(got, want) <= 1e-12


def test_reference_sees_a_wrong_descriptor():
    """The comparison is not blind where the kernels share their arithmetic: a symmetric forward roll (the reference rolls
    longitude by the LATITUDE shift, panguweather.py:291), a mask boundary one column off and a leading pad one row off all
    leave the restatement far from the reference; the boundary, which touches few tokens, mostly in the per-token figure."""
    from dlwp_benchmark_amd import training

    case = ((1, 16, 32), (2, 6, 12), 32)
    qkv, bias, table = (t.double() for t in pangu_inputs(case))
    want = pangu_reference(case, True, qkv, bias, table)
    spec = pangu_spec(case, True)[0]
    b1 = tuple(spec.mask_b1)
    lead = tuple(spec.pad_lead)
    for wrong in (dataclasses.replace(spec, shift_fwd=tuple(spec.shift_back)),
                  dataclasses.replace(spec, mask_b1=(b1[0], b1[1], b1[2] + 1)),
                  dataclasses.replace(spec, pad_lead=(lead[0], lead[1] - 1, lead[2]))):
        got = training.window_attention_torch(qkv, bias, table, wrong)
        per_token = float(((got - want).norm(dim=-1) / want.norm(dim=-1)).max())
        print("%.2e %.2e" % (rel_l2(got, want), per_token))
        assert rel_l2(got, want) > 1e-3 and per_token > 1e-2


def test_bf16_operand_model_costs_what_bf16_costs():
    """operands="bf16" rounds four things to 8 significant bits: its distance from the fp64 reference is a few 2^-9, neither
    zero (nothing rounded) nor percent-sized (something else broken)."""
    case = (8, 32, 8, 32, 2, 8)
    qkv, _, table = swin_inputs(case)
    e = rel_l2(swin_reference(case, True, qkv, table, operands="bf16"), swin_reference(case, True, qkv, table))
    assert 2.0 ** -11 < e < 2.0 ** -6, e
