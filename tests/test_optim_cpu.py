"""The training step's tail (csrc/optim.hip, dlwp_benchmark_amd/optim.py) without a GPU: the C ABI of the new entry points, the
pure-Python table builder, the refusals, and the case builders and float64 oracles the GPU file (tests/test_optim_gpu.py)
shares.

The oracle is torch itself on the CPU: torch.optim.AdamW(foreach=False) and torch.nn.utils.clip_grad_norm_, run in float64 on
the same fp32 inputs.  The AdamW bound is not fixed in advance: it is twice the error of torch's OWN fp32 CPU AdamW against
that float64 run (`adamw_bound`), because an equally valid order of the same fp32 operations (lerp against multiply-add,
1 / sqrt(bc2) against a divide) adds at most about one more rounding per operation.  test_reference_error_figures prints
those figures (DESIGN section 27 quotes them)."""
import copy
import os
import re

import pytest
import torch

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import optim as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["dlwp_mt_chunk_elems", "dlwp_mse_loss_partials", "dlwp_mse_loss_f32", "dlwp_mse_loss_scale_grad_f32",
                    "dlwp_mt_grad_norm_f32", "dlwp_mt_scale_f32", "dlwp_mt_zero_f32", "dlwp_mt_adamw_f32", "dlwp_mt_ema_f32"]
LR, WD, MAX_NORM, STEPS = 1e-3, 1e-5, 1e-3, 5          # the reference's values (clip at max_norm = lr)
VIEW_ELEMS = 1023                                       # the parameter that is base[1:1 + 1023]: 4-byte aligned only


def chunk():
    return int(L.load().dlwp_mt_chunk_elems())


def standard_sizes():
    e = chunk()
    return [1, 3, 5, e - 1, e, e + 1, 2 * e + 7]


# roles of the tensors of a case beside "plain"
VIEW, NO_GRAD, FROZEN = "view", "no_grad", "frozen"


def make_case(sizes=None, steps=STEPS, seed=0, extras=True, integer_grads=False):
    """{"params": [fp32 CPU tensors], "roles": [...], "grads": [step][tensor] (None where the tensor has no gradient)}.
    Parameters N(0, 1); gradients N(0, 1) times a per-tensor power of ten in [1e-6, 10] (integers in [-4, 4] for
    integer_grads).  extras: the unaligned view, one tensor with grad=None and one with requires_grad=False."""
    sizes = list(standard_sizes() if sizes is None else sizes)
    roles = ["plain"] * len(sizes)
    if extras:
        sizes += [VIEW_ELEMS, 37, 19]
        roles += [VIEW, NO_GRAD, FROZEN]
    g = torch.Generator().manual_seed(1234 + seed)
    params = [torch.randn(n, generator=g, dtype=torch.float32) for n in sizes]
    grads = []
    for _ in range(steps):
        row = []
        for i, (n, role) in enumerate(zip(sizes, roles)):
            if role in (NO_GRAD, FROZEN):
                row.append(None)
            elif integer_grads:
                row.append(torch.randint(-4, 5, (n,), generator=g).float())
            else:
                row.append(torch.randn(n, generator=g, dtype=torch.float32) * 10.0 ** (i % 8 - 6))
        grads.append(row)
    return {"params": params, "roles": roles, "grads": grads}


def torch_run(case, dtype, steps=None, lr=LR, wd=WD, max_norm=MAX_NORM, cosine_t_max=None, device="cpu", state_dict=None,
              first_step=0):
    """torch's own training tail on `case`: clip_grad_norm_ (when max_norm) and AdamW(foreach=False) for `steps` steps in
    `dtype`.  Returns {"p", "exp_avg", "exp_avg_sq": lists (None state for a tensor never stepped), "norms", "opt"}."""
    steps = len(case["grads"]) if steps is None else steps
    params = [p.to(device=device, dtype=dtype).clone().requires_grad_(role != FROZEN)
              for p, role in zip(case["params"], case["roles"])]
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd, foreach=False)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=cosine_t_max) if cosine_t_max else None
    norms = []
    for s in range(first_step, first_step + steps):
        for p, g in zip(params, case["grads"][s]):
            p.grad = None if g is None else g.to(device=device, dtype=dtype).clone()
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm).detach().cpu())
        opt.step()
        if sched is not None:
            sched.step()
    state = [opt.state.get(p, {}) for p in params]
    return {"p": [p.detach().cpu() for p in params], "exp_avg": [s.get("exp_avg") for s in state],
            "exp_avg_sq": [s.get("exp_avg_sq") for s in state], "norms": norms, "opt": opt}


def run_errors(got, want):
    """(p, exp_avg, exp_avg_sq): the maximum over tensors of the max absolute error for p, and of the max absolute error
    divided by the tensor's max magnitude for the two moments (tensors without state are left out)"""
    out = []
    for key in ("p", "exp_avg", "exp_avg_sq"):
        worst = 0.0
        for a, b in zip(got[key], want[key]):
            if b is None:
                continue
            a, b = a.detach().double().cpu(), b.detach().double().cpu()
            err = float((a - b).abs().max())
            if key != "p":
                err /= max(float(b.abs().max()), 1e-300)
            worst = max(worst, err)
        out.append(worst)
    return tuple(out)


def ref_error(case, **kw):
    """the three errors of torch's own fp32 CPU AdamW against its float64 run on the same inputs, and that float64 run"""
    want = torch_run(case, torch.float64, **kw)
    return run_errors(torch_run(case, torch.float32, **kw), want), want


def adamw_bound(case, **kw):
    """(bound per quantity = 2 x ref_error, the float64 run)"""
    err, want = ref_error(case, **kw)
    return tuple(2.0 * e for e in err), want


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_mirrored_and_exported():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/dlwp_hip.h"
        assert name in L.SIGNATURES, f"{name} is not in lib.SIGNATURES"
        assert hasattr(lib, name), f"libdlwp_hip.so does not export {name}"
        if name.endswith("_f32"):
            assert L.SIGNATURES[name][1][-1] is L.c_void_p, f"{name}: the stream comes last"
    # every entry point names what it replaces, file:line, in the comment above it
    block = header[header.index("The tail of a training step"):]
    for where in ("train.py:186", "train.py:299-305", "train.py:309", "train.py:312", "losses.py:175-188", "clip_grad.py:165-169",
                  "optim/adam.py:347-547"):
        assert where in block, where
    assert "typedef struct" not in block


def test_queries():
    lib = L.load()
    e = lib.dlwp_mt_chunk_elems()
    assert e > 0 and e % 4 == 0
    assert lib.dlwp_mse_loss_partials(0) == 0 and lib.dlwp_mse_loss_partials(-5) == 0
    last = 0
    for n in [1, 2, 63, 64, 1000, 4096, 4097, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 10]:
        p = lib.dlwp_mse_loss_partials(n)
        assert 0 < p <= n and p >= last, (n, p)
        last = p


# ---- the table builder (pure Python) ------------------------------------------------------------------------------------
def check_table(numels, e):
    t = O.build_table(numels, e)
    assert t["numel"] == list(numels)
    seen = [[] for _ in numels]
    for ti, first in zip(t["chunk_tensor"], t["chunk_first"]):
        assert 0 <= ti < len(numels) and first % e == 0 and 0 <= first < numels[ti]
        seen[ti].append(first)
    for n, firsts in zip(numels, seen):                # every element of every tensor exactly once
        assert firsts == list(range(0, n, e))
    assert t["chunk_tensor"] == sorted(t["chunk_tensor"])
    spans = sorted((off, off + n) for off, n in zip(t["state_off"], numels))
    for (a0, a1), (b0, _) in zip(spans, spans[1:]):
        assert a1 <= b0, "state offsets overlap"
    assert all(off % 4 == 0 for off in t["state_off"]) and t["state_elems"] >= spans[-1][1]
    return t


def test_table_builder_covers_the_standard_list():
    e = chunk()
    sizes = standard_sizes() + [VIEW_ELEMS, 37, 19]
    t = check_table(sizes, e)
    assert len(t["chunk_tensor"]) == 1 + 1 + 1 + 1 + 1 + 2 + 3 + 1 + 1 + 1
    check_table([0, 7, 0, 3 * e], e)                  # a tensor without elements has no chunk
    check_table([5], 4)
    assert check_table([10 ** 7 + 1], e)["chunk_first"][-1] == 10 ** 7 // e * e


def test_table_builder_needs_no_device(monkeypatch):
    monkeypatch.setattr(torch, "tensor", lambda *a, **k: pytest.fail("the table builder made a tensor"))
    O.build_table([3, 4097], 4096)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_cpu_parameters_are_refused():
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        O.FusedAdamW([torch.zeros(4, requires_grad=True)])
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        p = torch.zeros(4, requires_grad=True)
        p.grad = torch.ones(4)
        O.clip_grad_norm_([p], 1.0)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        O.ExponentialMovingAverage(torch.nn.Linear(2, 2), 0.99).register()


def test_unsupported_options_are_refused():
    p = [torch.zeros(4, requires_grad=True)]
    with pytest.raises(L.DlwpError, match="amsgrad"):
        O.FusedAdamW(p, amsgrad=True)
    with pytest.raises(L.DlwpError, match="maximize"):
        O.FusedAdamW(p, maximize=True)
    with pytest.raises(L.DlwpError, match="norm type"):
        O.clip_grad_norm_(p, 1.0, norm_type=1.0)


def test_loss_refuses_cpu_tensors_and_keeps_no_reduction_in_torch():
    from dlwp_benchmark_amd import losses

    x, t = torch.randn(2, 3, 4), torch.randn(2, 3, 4)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        losses.CustomMSELoss()(x, t)
    w = torch.rand(3, 4, dtype=torch.float64)
    d = losses.CustomMSELoss(weights=w, reduction="none", weighted=True)(x, t)
    assert d.dtype == torch.float64 and torch.equal(d, ((t - x) ** 2) * w)


def test_mse_loss_torch_is_the_reference_expression():
    from dlwp_benchmark_amd import training as T

    x, t = torch.randn(2, 3, 4), torch.randn(2, 3, 4)
    w = torch.rand(3, 4, dtype=torch.float64)
    assert torch.equal(T.mse_loss_torch(x, t), torch.mean((t - x) ** 2))
    got = T.mse_loss_torch(x, t, w)
    assert got.dtype == torch.float64 and torch.equal(got, torch.mean(((t - x) ** 2) * w))


# ---- the figures the bounds come from ----------------------------------------------------------------------------------
def test_reference_error_figures():
    """torch fp32 against torch float64 on exactly the inputs the GPU test uses: the figures behind the AdamW bound."""
    case = make_case()
    (ep, em, ev), want = ref_error(case)
    print(f"torch fp32 CPU AdamW against float64, {STEPS} steps: p {ep:.2e} (absolute), exp_avg {em:.2e}, exp_avg_sq {ev:.2e}")
    assert 0 < ep < 5e-6 and 0 < em < 5e-6 and 0 < ev < 5e-6, "the inputs no longer give a rounding-level reference error"
    assert want["exp_avg"][case["roles"].index(NO_GRAD)] is None and len(want["norms"]) == STEPS
    # the oracle is deterministic: the GPU file may rebuild it
    again = torch_run(copy.deepcopy(case), torch.float64)
    assert all(torch.equal(a, b) for a, b in zip(again["p"], want["p"]))
