"""The window-attention backward kernels (csrc/window_attn_bwd.hip, dlwp_window_attn_bwd_f32: a stats kernel and a key-owned main
kernel) against the gradient of an independent float64 reference: torch.autograd.grad through ref_swin / ref_pangu of
tests/window_attn_ref.py (the reference's own pad / roll / window_partition / attention sequence; its gradient through
F.pad(x - bias) + bias is the qkv-bias gradient).  Case tables, inputs, figures and the CPU checks of the reference gradient
(it equals the restatement's in float64, it is a gradient, the figures see a wrong descriptor): tests/test_window_attn_ref_cpu.py.

Figures, per case (all printed before anything is asserted):
  dqkv, dtable     rel-L2
  dqkv per token   max over (batch, token) of |got_t - want_t|_2 over the RMS over tokens of |want_t|_2: one mis-routed or
                   mis-masked token, which the global norm dilutes
  dtable per entry max |got - want| / max |want|: one entry written to the wrong (type, head) column
  dtable zeros     wherever the reference gradient is exactly 0.0 (never indexed, or indexed only by cropped queries, whose
                   grad_out is zero) the kernel's is exactly 0.0
  dbias            |got - want|_2 over |want|_2, its own scale, wherever the descriptor pads and |want| >= 1e-3 |want_dqkv|;
                   the rolled (1, 9, 30) case, whose padded level is masked off (reference dbias ~1e-16 of dqkv), keeps the
                   absolute rule of tests/test_window_attn_bwd_gpu.py: |got - want|_2 <= 2e-5 |want_dqkv|_2

Bounds come from the reference and the project, never from the kernel:
  rel-L2 figures and dbias on its own scale   <= max(2e-5, 4 floor)
  per-token and per-entry figures             <= max(1e-4, 4 floor)
floor is the same figure of the restatement's gradient in float32 on the CPU on the same inputs (what fp32 arithmetic costs
there); 2e-5 is the project's bound for this operator's gradients; 1e-4 keeps the 5 : 1 ratio of per-token to global bound of
tests/test_window_attn_fp64_gpu.py; 4 is that file's allowance for another summation order and v_exp_f32 -- here 8-lane
partial sweeps in the stats kernel and one float atomic per key block into dq.

What fails if the kernel file is broken, by reading it (no broken kernel was built or run):
  type without ipl * D.nlat    the rows with two level windows ((3, 7, 13), (4, 8, 16), wpl 1): windows of the upper level
                               read and write the bias column of the lower one -- dqkv per token, dtable rel-L2 and per entry
                               (every case of tests/test_window_attn_bwd_gpu.py has one level window)
  dq of padded queries not     "dbias own scale" at every padded row but the rolled (1, 9, 30): the q third of the bias
  added to dbias               gradient stays zero
  grad_table memset without    test_outputs_are_fully_written at (3, 7, 13): four types, so three quarters of the NaN
  types                        prefill survive under the atomics (torch.empty_like in ops may or may not hide it)
  kn < N dropped from the      alone it changes no result while the bias is finite: the dead rows of a ragged tile are staged
  key staging                  from the bias pointer and multiplied by p = ds = 0.  test_unpadded_descriptor_never_reads_the_qkv_bias
                               makes it visible: N = 16, a NaN bias, and 0 x NaN reaches dq
"""
import ctypes
import dataclasses
import functools

import pytest
import torch

import test_window_attn_ref_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GLOBAL, FINE = 2e-5, 1e-4
PROJECT_BOUND = {"dqkv rel-L2": GLOBAL, "dtable rel-L2": GLOBAL, "dbias own scale": GLOBAL, "dqkv per token": FINE,
                 "dtable per entry": FINE}
ERR_INVALID_ARGUMENT = -1      # DLWP_ERR_INVALID_ARGUMENT (include/dlwp_hip.h)

ROLLED_3_7_13 = ("pangu", ((3, 7, 13), (2, 6, 12), 2, 24, 3), True)
SHIFTED_8_8 = ("swin", (8, 8, 4, 4, 1, 8, 1), True)
SHIFTED_8_8_BATCH3 = ("swin", (8, 8, 4, 4, 1, 8, 3), True)
WPL1 = ("pangu", ((2, 12, 24), (1, 6, 12), 2, 64, 2), False)


def _small(key):
    kind, case, shifted = key
    return (C.bwd_swin_case if kind == "swin" else C.bwd_pangu_case)(case, shifted)


@functools.lru_cache(maxsize=None)
def _small_refs(key):
    """(reference gradients, fp32 floor) of a small case, which need not be a row of the tables (batch 3 of the 8 x 8 one)"""
    case = _small(key)
    return C.reference_grads(case), C.floor_grads(case)


def _bounds(spec, want, floor, outputs):
    """{figure: (bound, floor)}"""
    out = {}
    for k, f in C.grad_figures(spec, floor, want, outputs).items():
        # the absolute rule of the rolled (1, 9, 30) case is the existing file's: no floor enters it
        out[k] = (GLOBAL, f) if k == "dbias on dqkv scale" else (max(PROJECT_BOUND[k], 4 * f), f)
    return out


def _check(tag, spec, got, want, floor, failures, outputs=("dqkv", "dbias", "dtable")):
    """prints every figure of `got` against the reference, its bound and its floor; appends what misses to `failures`"""
    bounds = _bounds(spec, want, floor, outputs)
    for k, v in C.grad_figures(spec, got, want, outputs).items():
        bound, f = bounds[k]
        print("%-34s %-20s %.2e (<= %.2e, floor %.2e, %.1f floors)" % (tag, k, v, bound, f, v / f if f else float("inf")))
        if not v <= bound:
            failures.append((tag, k, v, bound))
    for i, name in enumerate(("dqkv", "dbias", "dtable")):
        if name in outputs and got[i] is not None and not bool(torch.isfinite(got[i]).all()):
            failures.append((tag, name, "not finite"))
    if "dtable" in outputs:
        zero = C.exact_zero_entries(want[2])
        wrong = int((got[2].detach().cpu()[zero] != 0.0).sum())
        frac = float(zero.double().mean())
        print("%-34s %-20s %d of %d entries (%.2f of the table) that the reference leaves exactly zero are not" %
              (tag, "dtable zeros", wrong, int(zero.sum()), frac))
        if wrong:
            failures.append((tag, "dtable zeros", wrong))
        if spec.bias_mode == 1 and spec.padded[0] > spec.grid[0] and not frac >= 0.25:
            failures.append((tag, "the exact-zero check is nearly vacuous", frac))


def _to_dev(case):
    return tuple(t.to(DEV) for t in (case.qkv, case.bias, case.table, case.gout))


@pytest.mark.parametrize("name", C.BWD_IDS)
def test_backward_matches_the_fp64_reference(name):
    """ops.window_attention_backward at every row of BWD_SWIN / BWD_PANGU, unshifted and shifted, and at the three large-logit
    inputs (logits in the hundreds: the stats kernel's online rescaling of l and delta does real work, the running maximum
    keeps moving along the keys).  Those fall under the same rule; their floors are large because fp32 arithmetic itself
    loses that much there."""
    from dlwp_benchmark_amd import ops

    case = C.bwd_case(name)
    want, floor = C.cached_reference_grads(name), C.cached_floor_grads(name)
    qkv, bias, table, gout = _to_dev(case)
    gq, gb, gt = ops.window_attention_backward(qkv, bias, table, case.spec, gout)
    torch.cuda.synchronize()
    failures = []
    _check(name, case.spec, (gq, gb, gt), want, floor, failures)
    assert (gb is not None) == C.is_padded(case.spec)         # where nothing is padded there is no qkv-bias gradient
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# the entry point itself: what it zeroes, what it writes, what it refuses
# ---------------------------------------------------------------------------------------------------------------------
def _nwin(spec):
    return (spec.padded[0] // spec.window[0]) * (spec.padded[1] // spec.window[1]) * (spec.padded[2] // spec.window[2])


def _workspace_bytes(spec, batch):
    from dlwp_benchmark_amd import lib as L

    d = spec.to_c()
    return int(L.load().dlwp_window_attn_bwd_workspace_bytes(ctypes.byref(d), batch))


def _raw_call(spec, qkv, bias, table, gout, ws_fill=0xFF, guard=0):
    """dlwp_window_attn_bwd_f32 through lib.launch as ops.window_attention_backward calls it, but on outputs prefilled with NaN
    and a workspace of `ws_fill` bytes (`guard` more bytes are allocated than the entry point is told of).  Returns the
    outputs, the workspace and the byte count the query gave."""
    from dlwp_benchmark_amd import lib as L

    b, c = qkv.shape[0], qkv.shape[2] // 3
    nbytes = _workspace_bytes(spec, b)
    gq, gt = torch.full_like(qkv, float("nan")), torch.full_like(table, float("nan"))
    gb = torch.full((3 * c,), float("nan"), device=qkv.device) if C.is_padded(spec) else None
    ws = torch.full((nbytes + guard,), ws_fill, dtype=torch.uint8, device=qkv.device)
    L.launch("dlwp_window_attn_bwd_f32", qkv.device, spec.to_c(), qkv, bias, table, gout, gq, gb, gt, b, ws, nbytes)
    torch.cuda.synchronize()
    return (gq, gb, gt), ws, nbytes


@pytest.mark.parametrize("key", [ROLLED_3_7_13, SHIFTED_8_8_BATCH3], ids=["3x7x13-rolled", "8x8-shifted-batch3"])
def test_outputs_are_fully_written(key):
    """grad_qkv, grad_qkv_bias and grad_table prefilled with NaN and a workspace of 0xFF bytes (NaN statistics), batch 3: the
    entry point zeroes all it accumulates into (dq and the table gradient arrive through atomics, the qkv-bias gradient too),
    sized by the batch and by types x heads, and the stats kernel writes every row the main kernel reads."""
    from dlwp_benchmark_amd import ops

    case = _small(key)
    want, floor = _small_refs(key)
    assert case.qkv.shape[0] == 3
    qkv, bias, table, gout = _to_dev(case)
    raw, _, _ = _raw_call(case.spec, qkv, bias, table, gout)
    via_ops = ops.window_attention_backward(qkv, bias, table, case.spec, gout)
    torch.cuda.synchronize()
    failures = []
    for a in raw:
        assert a is None or bool(torch.isfinite(a).all())
    _check("prefilled " + case.name, case.spec, raw, want, floor, failures)
    # and against the ops call, which differs in nothing but the order of the atomics: the same bounds with the ops call's
    # result in the reference's place
    for k, v in C.grad_figures(case.spec, raw, via_ops).items():
        bound = GLOBAL if k == "dbias on dqkv scale" else PROJECT_BOUND[k]
        print("prefilled vs ops %-22s %-20s %.2e (<= %.2e)" % (case.name, k, v, bound))
        if not v <= bound:
            failures.append((case.name, "vs ops", k, v, bound))
    assert not failures, failures


@pytest.mark.parametrize("key", [ROLLED_3_7_13, SHIFTED_8_8, WPL1], ids=["3x7x13-rolled", "8x8-shifted", "wpl1"])
def test_kernels_stay_inside_the_queried_workspace(key):
    """nbytes + 4096 bytes of 0xA5 are allocated and nbytes passed: the last 4096 bytes, all inside the allocation, are
    unchanged afterwards, and the statistics in front of them were written.  nbytes is what the header promises:
    3 floats per (batch, window, head, row) and 256 bytes."""
    case = _small(key)
    spec = case.spec
    qkv, bias, table, gout = _to_dev(case)
    b, n = qkv.shape[0], spec.window[0] * spec.window[1] * spec.window[2]
    got, ws, nbytes = _raw_call(spec, qkv, bias, table, gout, ws_fill=0xA5, guard=4096)
    assert nbytes == b * _nwin(spec) * spec.heads * n * 12 + 256
    assert ws.numel() == nbytes + 4096
    assert bool((ws[nbytes:] == 0xA5).all()), "the kernels wrote past the workspace size their own query returns"
    used = ws[:nbytes - 256]
    assert not bool((used.view(-1, 4) == 0xA5).all(dim=1).any()), "a statistic of a live row was never written"
    assert all(a is None or bool(torch.isfinite(a).all()) for a in got)


def test_unpadded_descriptor_never_reads_the_qkv_bias():
    """Nothing is padded, so no token carries the qkv bias: a bias of NaN changes nothing.  N = 16 leaves rows 16 .. 31 of the
    only tile dead; their staging points at the bias and is kept from reading it by the row bound alone (a staged NaN would
    reach dq as 0 x NaN)."""
    from dlwp_benchmark_amd import ops

    case = _small(SHIFTED_8_8)
    want, floor = _small_refs(SHIFTED_8_8)
    assert not C.is_padded(case.spec) and case.spec.window[1] * case.spec.window[2] < 32
    qkv, bias, table, gout = _to_dev(case)
    gq, gb, gt = ops.window_attention_backward(qkv, torch.full_like(bias, float("nan")), table, case.spec, gout)
    torch.cuda.synchronize()
    failures = []
    _check("NaN bias " + case.name, case.spec, (gq, gb, gt), want, floor, failures)
    assert gb is None and not failures, failures


def _untouched(outs):
    return all(a is None or bool(torch.isnan(a).all()) for a in outs)


def test_statuses_that_return_before_any_launch():
    """head_dim 20, a padded descriptor without a grad_qkv_bias buffer, a workspace one byte short: each raises DlwpError
    with its status, and the NaN-prefilled outputs are still all NaN (no memset and no kernel ran)."""
    from dlwp_benchmark_amd import lib as L

    case = _small(ROLLED_3_7_13)
    spec = case.spec
    qkv, bias, table, gout = _to_dev(case)
    b, l = qkv.shape[:2]

    spec20 = dataclasses.replace(spec, head_dim=20, scale=20 ** -0.5)
    c20 = spec.heads * 20
    g = torch.Generator().manual_seed(20)
    qkv20, bias20, gout20 = (torch.randn(*s, generator=g).to(DEV) for s in ((b, l, 3 * c20), (3 * c20,), (b, l, c20)))
    for kwargs in ({"with_gbias": False}, {"short": 1}):
        outs = []
        with pytest.raises(L.DlwpError) as e:
            _raw_into(outs, spec, qkv, bias, table, gout, **kwargs)
        assert e.value.status == ERR_INVALID_ARGUMENT, kwargs
        assert outs and _untouched(outs), kwargs
    outs = []
    with pytest.raises(L.DlwpError) as e:
        _raw_into(outs, spec20, qkv20, bias20, table, gout20)
    assert e.value.status == L.ERR_UNSUPPORTED and outs and _untouched(outs)


def _raw_into(outs, spec, qkv, bias, table, gout, short=0, with_gbias=True):
    """_raw_call for a call that is to raise: the NaN-prefilled outputs are appended to `outs` before the entry point is called"""
    from dlwp_benchmark_amd import lib as L

    b, c = qkv.shape[0], qkv.shape[2] // 3
    nbytes = _workspace_bytes(spec, b)
    outs += [torch.full_like(qkv, float("nan")), torch.full((3 * c,), float("nan"), device=qkv.device),
             torch.full_like(table, float("nan"))]
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=qkv.device)
    try:
        L.launch("dlwp_window_attn_bwd_f32", qkv.device, spec.to_c(), qkv, bias, table, gout, outs[0], outs[1] if with_gbias else None,
                 outs[2], b, ws, nbytes - short)
    finally:
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the autograd layer: training.window_attention, HIP forward and HIP backward
# ---------------------------------------------------------------------------------------------------------------------
def _through_autograd(case, loss, requires=(True, True, True)):
    from dlwp_benchmark_amd import training

    q, b, t = (x.to(DEV).clone().requires_grad_(r) for x, r in zip((case.qkv, case.bias, case.table), requires))
    loss(training.window_attention(q, b, t, case.spec)).backward()
    torch.cuda.synchronize()
    return q.grad, b.grad, t.grad


@pytest.mark.parametrize("key", [ROLLED_3_7_13, SHIFTED_8_8], ids=["3x7x13-rolled", "8x8-shifted"])
def test_autograd_layer_with_expanded_and_transposed_grad_out(key):
    """out.sum().backward() hands the Function a stride-0 grad_out, (out.transpose(1, 2) * r).sum().backward() a
    non-contiguous one; the kernel reads rows of C contiguous floats."""
    case = _small(key)
    failures = []
    ones = torch.ones_like(case.gout)
    got = _through_autograd(case, lambda out: out.sum())
    _check("sum() " + case.name, case.spec, got, C.reference_grads(case, gout=ones), C.floor_grads(case, gout=ones), failures)
    g = torch.Generator().manual_seed(7)
    r = torch.randn(case.gout.shape[0], case.gout.shape[2], case.gout.shape[1], generator=g)
    got = _through_autograd(case, lambda out: (out.transpose(1, 2) * r.to(DEV)).sum())
    gout = r.transpose(1, 2)
    _check("transposed " + case.name, case.spec, got, C.reference_grads(case, gout=gout), C.floor_grads(case, gout=gout), failures)
    if not C.is_padded(case.spec):
        assert float(got[1].abs().max()) == 0.0
    assert not failures, failures


@pytest.mark.parametrize("key", [ROLLED_3_7_13, SHIFTED_8_8], ids=["3x7x13-rolled", "8x8-shifted"])
def test_autograd_layer_returns_only_the_gradients_asked_for(key):
    case = _small(key)
    want, floor = _small_refs(key)
    failures = []
    loss = lambda out: (out * case.gout.to(DEV)).sum()
    gq, gb, gt = _through_autograd(case, loss, requires=(False, False, True))
    assert gq is None and gb is None and gt is not None
    _check("table only " + case.name, case.spec, (None, None, gt), want, floor, failures, outputs=("dtable",))
    gq, gb, gt = _through_autograd(case, loss, requires=(True, False, False))
    assert gq is not None and gb is None and gt is None
    _check("qkv only " + case.name, case.spec, (gq, None, None), want, floor, failures, outputs=("dqkv",))
    assert not failures, failures


def test_autograd_layer_unpadded_bias_gradient_is_exactly_zero():
    """An unpadded Swin block never reads the qkv bias: a bias that requires grad gets exact zeros, not None and not noise."""
    case = _small(SHIFTED_8_8)
    want, floor = _small_refs(SHIFTED_8_8)
    assert not C.is_padded(case.spec)
    gq, gb, gt = _through_autograd(case, lambda out: (out * case.gout.to(DEV)).sum())
    assert gb is not None and gb.shape == case.bias.shape and float(gb.abs().max()) == 0.0
    failures = []
    _check("unpadded bias " + case.name, case.spec, (gq, gb, gt), want, floor, failures)
    assert not failures, failures
