"""The case tables of the fp64 window-attention tests (tests/test_window_attn_fp64_gpu.py), checked on the CPU:

* training.window_attention_torch -- the differentiable restatement the backward tests differentiate -- equals the
  independent float64 reference (tests/window_attn_ref.py) at every geometry of the tables, in float64;
* the tables reach the kernels they claim.  plan2 / plan3 / generic_variant restate the host rules (wattn2::make_plan in
  csrc/window_attn2.hip, wattn3::make_plan3 in csrc/window_attn3.hip, launch_wattn in csrc/window_attn.hip; the first two on
  the Desc that normalise_desc of csrc/window_attn_desc.hpp fills, ordered by select_path of csrc/window_attn.hip); the GPU
  tests and tests/test_window_attn_host_cpu.py assert the same coverage again with dlwp_window_attn_workspace_bytes, so a
  stale restatement cannot hide a miss.

And the case tables of the fp64 backward tests (tests/test_window_attn_bwd_fp64_gpu.py), BWD_SWIN / BWD_PANGU and the three
large-logit inputs, chosen by what csrc/window_attn_bwd.hip branches on (the six DH instances, the bias mode, ragged or whole
32-row tiles, npl / nlat / nlon, padding per axis, mask, heads, batch):
* the tables reach what they claim (asserted from the descriptors);
* autograd through the float64 reference equals autograd through the restatement in float64, at every backward case and every
  row of the forward tables;
* the reference gradient is a gradient (central finite differences), and the figures the GPU file asserts see a wrong
  descriptor.
"""
import collections
import dataclasses
import functools
import zlib

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


# ---------------------------------------------------------------------------------------------------------------------
# the backward tables (tests/test_window_attn_bwd_fp64_gpu.py).  The forward's k2 / k3 / gen paths do not matter to
# csrc/window_attn_bwd.hip; what it branches on does.  Each row runs unshifted and shifted wherever a shift exists.
# ---------------------------------------------------------------------------------------------------------------------
# (h, w, wh, ww, heads, d, batch)
BWD_SWIN = [
    (8, 8, 4, 4, 1, 8, 1),              # N = 16: one partial tile, 4 windows
    (12, 20, 6, 10, 2, 32, 3),          # N = 60, ragged
    (14, 24, 7, 12, 3, 64, 2),          # N = 84, three heads, d 64
    (15, 34, 15, 17, 2, 16, 2),         # N = 255
    (16, 36, 16, 36, 1, 24, 2),         # N = 576: 18 tiles, 2201 table rows
    (12, 64, 6, 32, 2, 48, 1),          # N = 192: whole tiles, d 48
]
# (grid, window, heads, d, batch)
BWD_PANGU = [
    ((1, 16, 32), (2, 6, 12), 2, 32, 2),    # the geometry of tests/test_window_attn_bwd_gpu.py
    ((3, 7, 13), (2, 6, 12), 2, 24, 3),     # two level windows, one half padded; padded on every axis
    ((4, 8, 16), (2, 4, 8), 3, 8, 1),       # npl = nlat = nlon = 2: four types, N = 64
    ((2, 11, 13), (2, 5, 7), 2, 48, 2),     # N = 70, padded in lat and lon
    ((2, 12, 24), (1, 6, 12), 2, 64, 2),    # wpl 1, two level windows; no roll exists
    ((1, 9, 30), (2, 3, 10), 1, 16, 2),     # rolled: the padded level is masked off, the reference dbias is ~1e-16 of dqkv
]
BWD_SWIN_PARAMS = [(c, s) for c in BWD_SWIN for s in (False, True)]
BWD_PANGU_PARAMS = [(c, s) for c in BWD_PANGU for s in ((False, True) if pangu_rolls(c[1]) else (False,))]
LARGE_LOGIT_NAMES = ("slack", "slack-shifted", "earth-large-logits")

# one backward case: CPU fp32 inputs, the descriptor, and ref(qkv, bias, table) -> the float64 reference output
BwdCase = collections.namedtuple("BwdCase", "name spec qkv bias table gout ref")


def _seed(tag, case):
    return zlib.crc32(repr((tag, case)).encode())


def _swin_ref(h, w, wh, ww, heads, d, shifted):
    shift = (wh // 2, ww // 2) if shifted else (0, 0)
    return lambda qkv, bias, table: R.ref_swin(qkv, table, h, w, (wh, ww), shift, heads, d)


def _pangu_ref(grid, window, heads, d, shifted):
    shift = tuple(w // 2 for w in window) if shifted else (0, 0, 0)
    return lambda qkv, bias, table: R.ref_pangu(qkv, bias, table, grid, window, shift, heads, d)


@functools.lru_cache(maxsize=None)
def bwd_swin_case(case, shifted):
    from test_window_attn_gpu import _sub_window_spec

    h, w, wh, ww, heads, d, batch = case
    spec, rows = _sub_window_spec(h, w, wh, ww, heads, d, shifted)
    g = torch.Generator().manual_seed(_seed("bwd_swin", case))
    qkv = torch.randn(batch, h * w, 3, heads, d, generator=g)
    qkv[:, :, :2] *= 2.0
    bias = torch.randn(3 * heads * d, generator=g) * 0.1
    table = torch.randn(rows, heads, generator=g) * 0.5
    gout = torch.randn(batch, h * w, heads * d, generator=g)
    return BwdCase(case_id((case, shifted)), spec, qkv.reshape(batch, h * w, 3 * heads * d), bias, table, gout,
                   _swin_ref(h, w, wh, ww, heads, d, shifted))


@functools.lru_cache(maxsize=None)
def bwd_pangu_case(case, shifted):
    from test_window_attn_gpu import _earth_spec

    grid, window, heads, d, batch = case
    spec, rows, types = _earth_spec(grid, window, heads, shifted)
    spec = dataclasses.replace(spec, head_dim=d, scale=d ** -0.5)
    ltok = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(_seed("bwd_pangu", case))
    qkv = torch.randn(batch, ltok, 3, heads, d, generator=g)
    qkv[:, :, :2] *= 1.5
    bias = torch.randn(3 * heads * d, generator=g) * 0.3
    table = torch.randn(rows, types, heads, generator=g) * 0.5
    gout = torch.randn(batch, ltok, heads * d, generator=g)
    return BwdCase(case_id((case, shifted)), spec, qkv.reshape(batch, ltok, 3 * heads * d), bias, table, gout,
                   _pangu_ref(grid, window, heads, d, shifted and pangu_rolls(window)))


@functools.lru_cache(maxsize=None)
def bwd_large_logit_case(name):
    """slack_case(False), slack_case(True), earth_large_logits_case() with a seeded grad_out"""
    if name == "earth-large-logits":
        spec, qkv, bias, table, _ = earth_large_logits_case()
        ref = _pangu_ref((1, 16, 32), (2, 6, 12), 2, 32, True)
    else:
        shifted = name == "slack-shifted"
        spec, qkv, bias, table, _ = slack_case(shifted)
        ref = _swin_ref(16, 32, 16, 32, 2, 24, shifted)
    g = torch.Generator().manual_seed(_seed("bwd_large", name))
    gout = torch.randn(qkv.shape[0], qkv.shape[1], spec.heads * spec.head_dim, generator=g)
    return BwdCase(name, spec, qkv, bias, table, gout, ref)


@functools.lru_cache(maxsize=None)
def fwd_row_as_bwd_case(kind, p):
    """a row of SWIN_PARAMS / PANGU_PARAMS with a seeded grad_out"""
    case, shifted = p
    if kind == "swin":
        qkv, bias, table = swin_inputs(case)
        spec, ref = swin_spec(case, shifted), _swin_ref(*case, shifted)
    else:
        qkv, bias, table = pangu_inputs(case)
        spec, ref = pangu_spec(case, shifted)[0], _pangu_ref(case[0], case[1], PANGU_HEADS, case[2], shifted)
    g = torch.Generator().manual_seed(_seed("fwd_row", p))
    gout = torch.randn(qkv.shape[0], qkv.shape[1], spec.heads * spec.head_dim, generator=g)
    return BwdCase("fwd-" + case_id(p), spec, qkv, bias, table, gout, ref)


def all_bwd_cases():
    """(id, thunk) of every backward case: the two tables and the three large-logit inputs"""
    out = [(case_id(p), functools.partial(bwd_swin_case, *p)) for p in BWD_SWIN_PARAMS]
    out += [(case_id(p), functools.partial(bwd_pangu_case, *p)) for p in BWD_PANGU_PARAMS]
    out += [(n, functools.partial(bwd_large_logit_case, n)) for n in LARGE_LOGIT_NAMES]
    return out


def _grads(fn, case, dtype, gout):
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (case.qkv, case.bias, case.table)]
    out = fn(*leaves)
    assert out.dtype == dtype and not out.is_cuda
    gout = case.gout if gout is None else gout
    return tuple(torch.autograd.grad(out, leaves, gout.to(dtype), allow_unused=True))


def reference_grads(case, gout=None):
    """the float64 reference gradients (dqkv, dbias, dtable) of a case: torch.autograd.grad through R.ref_swin / R.ref_pangu on
    leaf copies.  dbias is None where the reference never reads the bias (Swin); a Pangu case that pads nothing gives zeros."""
    return _grads(case.ref, case, torch.float64, gout)


def restatement_grads(case, dtype, spec=None, gout=None):
    """the same three gradients from training.window_attention_torch on the CPU, under `spec` (default: the case's own)"""
    from dlwp_benchmark_amd import training

    spec = case.spec if spec is None else spec
    return _grads(lambda q, b, t: training.window_attention_torch(q, b, t, spec), case, dtype, gout)


def floor_grads(case, gout=None):
    """the fp32 floor: what fp32 arithmetic costs at these inputs -- the restatement's gradients in float32 on the CPU"""
    return restatement_grads(case, torch.float32, gout=gout)


# every case's reference gradients and floor, computed once and shared (nothing may write into them)
@functools.lru_cache(maxsize=None)
def cached_reference_grads(name):
    return reference_grads(bwd_case(name))


@functools.lru_cache(maxsize=None)
def cached_floor_grads(name):
    return floor_grads(bwd_case(name))


_CASES = dict(all_bwd_cases())
BWD_IDS = list(_CASES)


def bwd_case(name):
    return _CASES[name]()


# ---- the figures of the backward comparison (got: anything; want: the float64 reference) --------------------------------------
def _f64(t):
    return t.detach().double().cpu()


def per_token_rms(got, want):
    """max over (batch, token) of |got_t - want_t|_2 over the RMS over tokens of |want_t|_2.  NOT over the token's own norm:
    rolled and padded cases have tokens whose reference gradient is 1e-45 of the RMS, where fp32 itself is off by order 1."""
    got, want = _f64(got), _f64(want)
    return float((got - want).norm(dim=-1).max() / want.norm(dim=-1).square().mean().sqrt())


def per_entry(got, want):
    """max |got - want| / max |want|"""
    got, want = _f64(got), _f64(want)
    return float((got - want).abs().max() / want.abs().max())


def is_padded(spec):
    return tuple(spec.padded) != tuple(spec.grid)


def dbias_on_its_own_scale(want):
    """the qkv-bias gradient is judged on its own norm wherever the reference's is at least 1e-3 of |dqkv|; below that (the
    rolled (1, 9, 30) case, whose padded level is masked off) on the scale of dqkv"""
    return float(_f64(want[1]).norm()) >= 1e-3 * float(_f64(want[0]).norm())


def grad_figures(spec, got, want, outputs=("dqkv", "dbias", "dtable")):
    """{figure name: value} of gradients `got` = (dqkv, dbias, dtable) against the float64 reference `want`, for the named
    outputs (the others of `got` are not looked at)"""
    f = {}
    if "dqkv" in outputs:
        f.update({"dqkv rel-L2": rel_l2(got[0], want[0]), "dqkv per token": per_token_rms(got[0], want[0])})
    if "dtable" in outputs:
        f.update({"dtable rel-L2": rel_l2(got[2], want[2]), "dtable per entry": per_entry(got[2], want[2])})
    if "dbias" in outputs and is_padded(spec):
        err = float((_f64(got[1]) - _f64(want[1])).norm())
        if dbias_on_its_own_scale(want):
            f["dbias own scale"] = err / float(_f64(want[1]).norm())
        else:
            f["dbias on dqkv scale"] = err / float(_f64(want[0]).norm())
    return f


def exact_zero_entries(want_dtable):
    """where the reference table gradient is exactly 0.0: never indexed, or indexed only by cropped queries"""
    return _f64(want_dtable) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# backward tests
# ---------------------------------------------------------------------------------------------------------------------
def test_backward_tables_reach_what_they_claim():
    specs = [bwd_swin_case(*p).spec for p in BWD_SWIN_PARAMS] + [bwd_pangu_case(*p).spec for p in BWD_PANGU_PARAMS]
    batches = {c[-1] for c in BWD_SWIN} | {c[-1] for c in BWD_PANGU}
    n_of = lambda s: s.window[0] * s.window[1] * s.window[2]
    all_d = {8, 16, 24, 32, 48, 64}
    assert {s.head_dim for s in specs if s.bias_mode == 1} == all_d        # the six DH instances under the earth bias ...
    assert {s.head_dim for s in specs if s.bias_mode == 0} == all_d        # ... and under the Swin bias
    assert any(n_of(s) < 32 for s in specs)                                # a window below one 32-row tile
    assert any(n_of(s) > 32 and n_of(s) % 32 for s in specs)               # ragged last tile after whole ones
    assert any(n_of(s) % 32 == 0 for s in specs)
    assert any(s.padded[0] // s.window[0] > 1 and s.padded[0] > s.grid[0] for s in specs)   # npl > 1 beside a padded level
    assert any(s.window[0] == 1 and s.bias_mode == 1 and s.padded[0] // s.window[0] > 1 for s in specs)   # wpl 1, npl 2
    assert {s.heads for s in specs} == {1, 2, 3} and batches == {1, 2, 3}
    assert any(is_padded(s) and s.use_mask and any(s.shift_fwd) for s in specs)             # padded and rolled
    # all three window counts above one at once, and a padded level next to real ones in the same window
    assert any(all(p // w > 1 for p, w in zip(s.padded, s.window)) and s.bias_mode == 1 for s in specs)
    spec = bwd_pangu_case(((3, 7, 13), (2, 6, 12), 2, 24, 3), True).spec
    assert all(p > g for p, g in zip(spec.padded, spec.grid)) and spec.padded[0] // spec.window[0] == 2
    # the shifted rows are really shifted and masked, the wpl 1 row has no roll
    assert all(bwd_swin_case(c, True).spec.use_mask for c in BWD_SWIN)
    assert [c for c in BWD_PANGU if not pangu_rolls(c[1])] == [((2, 12, 24), (1, 6, 12), 2, 64, 2)]
    # the large-logit inputs are what tests/test_window_attn_fp64_gpu.py runs forward
    for name in LARGE_LOGIT_NAMES:
        c = bwd_large_logit_case(name)
        assert c.gout.shape == (c.qkv.shape[0], c.qkv.shape[1], c.spec.heads * c.spec.head_dim)


def _assert_restatement_equals_reference(case, want):
    got = restatement_grads(case, torch.float64)
    eq, et = rel_l2(got[0], want[0]), rel_l2(got[2], want[2])
    print(case.name, "gradient of the restatement vs of the reference, fp64: dqkv %.2e dtable %.2e" % (eq, et))
    assert eq <= 1e-12 and et <= 1e-12
    if got[1] is None or want[1] is None:
        # the Swin reference takes no bias; the restatement reads it only where the descriptor pads
        assert not is_padded(case.spec)
        assert all(g is None or float(g.abs().max()) == 0.0 for g in (got[1], want[1]))
    else:
        err = float((got[1] - want[1]).norm())
        print(case.name, "dbias %.2e of max(|dbias|, |dqkv|)" % (err / max(float(want[1].norm()), float(want[0].norm()))))
        assert err <= 1e-12 * max(float(want[1].norm()), float(want[0].norm()))


@pytest.mark.parametrize("name", BWD_IDS)
def test_backward_case_restatement_gradient_equals_the_reference_gradient(name):
    _assert_restatement_equals_reference(bwd_case(name), cached_reference_grads(name))


def test_backward_tables_dbias_scale_and_exact_zero_conditions():
    """Two conditions the GPU file relies on, from the reference alone: the qkv-bias gradient has a scale of its own at every
    padded case but the rolled (1, 9, 30) one, and every Pangu case with a padded level leaves at least a quarter of the
    table gradient exactly zero (so the exact-zero check is not vacuous)."""
    for p in BWD_PANGU_PARAMS:
        name = case_id(p)
        spec, want = bwd_case(name).spec, cached_reference_grads(name)
        if is_padded(spec):
            own = dbias_on_its_own_scale(want)
            ratio = float(want[1].norm() / want[0].norm())
            print(name, "|dbias| / |dqkv| = %.2e" % ratio)
            assert own == (p != (((1, 9, 30), (2, 3, 10), 1, 16, 2), True)), (name, ratio)
        else:
            assert float(want[1].abs().max()) == 0.0
        if spec.padded[0] > spec.grid[0]:
            frac = float(exact_zero_entries(want[2]).double().mean())
            print(name, "exactly-zero table gradient entries: %.2f" % frac)
            assert frac >= 0.25, (name, frac)
    for p in BWD_SWIN_PARAMS:
        assert cached_reference_grads(case_id(p))[1] is None
    want = cached_reference_grads("earth-large-logits")
    assert dbias_on_its_own_scale(want)


@pytest.mark.parametrize("p", SWIN_PARAMS, ids=case_id)
def test_swin_restatement_gradient_equals_the_reference_gradient(p):
    case = fwd_row_as_bwd_case("swin", p)
    _assert_restatement_equals_reference(case, reference_grads(case))


@pytest.mark.parametrize("p", PANGU_PARAMS, ids=case_id)
def test_pangu_restatement_gradient_equals_the_reference_gradient(p):
    case = fwd_row_as_bwd_case("pangu", p)
    _assert_restatement_equals_reference(case, reference_grads(case))


@pytest.mark.parametrize("name", [case_id((((3, 7, 13), (2, 6, 12), 2, 24, 3), True)), case_id(((8, 8, 4, 4, 1, 8, 1), True))])
def test_reference_gradient_is_a_gradient(name):
    """One central finite difference of sum(ref(x) * grad_out) along a seeded random direction in each input, float64, h = 1e-6:
    truncation ~h^2 and rounding ~2^-53 |f| / h are both far below 1e-6 of the directional derivative."""
    case, want = bwd_case(name), cached_reference_grads(name)
    x0 = [t.double() for t in (case.qkv, case.bias, case.table)]
    gout = case.gout.double()
    g = torch.Generator().manual_seed(_seed("fd", name))
    h = 1e-6
    for i, what in enumerate(("qkv", "bias", "table")):
        if want[i] is None:
            assert what == "bias" and case.spec.bias_mode == 0       # ref_swin takes no bias
            continue
        u = torch.randn(x0[i].shape, generator=g, dtype=torch.float64)
        f = []
        for sign in (1.0, -1.0):
            x = list(x0)
            x[i] = x0[i] + sign * h * u
            f.append(float((case.ref(*x) * gout).sum()))
        fd, ip = (f[0] - f[1]) / (2 * h), float((want[i] * u).sum())
        print(name, what, "finite difference %.9e  <gradient, direction> %.9e" % (fd, ip))
        assert abs(ip) > 1e-3 * float(want[i].norm())               # the direction is not orthogonal to the gradient by accident
        assert abs(fd - ip) <= 1e-6 * abs(ip), (what, fd, ip)


def test_reference_gradient_sees_a_wrong_descriptor():
    """The figures of tests/test_window_attn_bwd_fp64_gpu.py are not blind: the three corruptions of
    test_reference_sees_a_wrong_descriptor, differentiated through the restatement in float64, all move dqkv's per-token figure
    by more than 1e-2 (a bound of 1e-4 is asserted there), and at least one moves the table gradient's per-entry figure so."""
    name = case_id((BWD_PANGU[0], True))
    case, want = bwd_case(name), cached_reference_grads(name)
    spec = case.spec
    b1, lead = tuple(spec.mask_b1), tuple(spec.pad_lead)
    moved_table = 0
    for wrong in (dataclasses.replace(spec, shift_fwd=tuple(spec.shift_back)),
                  dataclasses.replace(spec, mask_b1=(b1[0], b1[1], b1[2] + 1)),
                  dataclasses.replace(spec, pad_lead=(lead[0], lead[1] - 1, lead[2]))):
        f = grad_figures(spec, restatement_grads(case, torch.float64, spec=wrong), want)
        print(", ".join("%s %.2e" % kv for kv in f.items()))
        assert f["dqkv per token"] > 1e-2
        moved_table += f["dtable per entry"] > 1e-2
    assert moved_table >= 1
    right = grad_figures(spec, restatement_grads(case, torch.float64), want)
    assert max(right.values()) <= 1e-12
