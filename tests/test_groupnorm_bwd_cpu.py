"""GroupNorm + activation backward, the parts that need no GPU: the three C entry points are declared, exported and in the
ctypes table, and training.groupnorm_act_backward_torch (the formulas of csrc/groupnorm_bwd.hip as torch operators) in fp32
agrees with fp64 autograd of act(F.group_norm(x, G, gamma, beta, 1e-5)) within the project's fp32 bound of 1e-5 (relative
L2; the formulas themselves sit near 5e-7, torch's own fp32 backward near 2e-6).

CASES, inputs(), reference(), term_norms() and deviation() are shared with tests/test_groupnorm_bwd_gpu.py."""
import functools
import os
import re

import pytest
import torch

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd.weights import normal
from helpers import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dlwp_groupnorm_act_fwd_stats_f32", "dlwp_groupnorm_act_bwd_workspace_bytes", "dlwp_groupnorm_act_bwd_f32"]
ACT_FNS = {0: lambda t: t, 1: torch.nn.functional.gelu, 2: torch.tanh, 3: torch.nn.functional.relu,
           4: torch.nn.functional.silu}

# (x shape, groups, x starts one float into its storage): what each reaches is listed in test_groupnorm_bwd_gpu.py
CASES = {
    "rows_of_4": ((2, 8, 2, 2), 8, False),
    "hw35": ((3, 12, 5, 7), 4, False),
    "one_group": ((2, 16, 8, 8), 1, False),
    "rank3_300": ((2, 6, 300), 3, False),
    "hw1056": ((1, 4, 33, 32), 2, False),
    "rows1632": ((12, 136, 8, 8), 1, False),
    "offset_view": ((2, 8, 4, 4), 2, True),
    "hw257": ((2, 3, 257), 1, False),
}


def inputs(tag):
    """fp32 (x, gamma, beta, gy) of a case on the CPU, identical on every machine"""
    shape, _, _ = CASES[tag]
    c = shape[1]
    x = 3.0 + 2.0 * normal(f"test/groupnorm_bwd/{tag}/x", shape, 1.0)
    gamma = 1.0 + 0.5 * normal(f"test/groupnorm_bwd/{tag}/gamma", (c,), 1.0)
    beta = 0.5 * normal(f"test/groupnorm_bwd/{tag}/beta", (c,), 1.0)
    gy = normal(f"test/groupnorm_bwd/{tag}/gy", shape, 1.0)
    return x, gamma, beta, gy


@functools.lru_cache(maxsize=None)
def reference(tag, act, affine, mean_gy=False):
    """fp64 autograd of act(F.group_norm(x, G, gamma, beta, 1e-5)): (dx, dgamma, dbeta), the last two None without affine.
    mean_gy: the output gradient of y.mean() instead of the case's dense one."""
    x, gamma, beta, gy = inputs(tag)
    groups = CASES[tag][1]
    x = x.double().requires_grad_(True)
    gy = torch.full_like(x, 1.0 / x.numel()) if mean_gy else gy.double()
    wrt = [x]
    if affine:
        gamma, beta = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        wrt += [gamma, beta]
    else:
        gamma = beta = None
    y = ACT_FNS[act](torch.nn.functional.group_norm(x, groups, gamma, beta, 1e-5))
    grads = list(torch.autograd.grad(y, wrt, gy))
    return tuple(grads) if affine else (grads[0], None, None)


@functools.lru_cache(maxsize=None)
def term_norms(tag, act, affine, mean_gy=False):
    """The sizes, in fp64, of the terms the gradients are sums of: (|| rstd gv gamma ||, || sum |gv xh| ||, || sum |gv| ||)
    for dx = rstd (gv gamma - a - xh b), dgamma = sum gv xh, dbeta = sum gv.  With a constant output gradient and the identity
    activation some of these sums cancel exactly (dx = 0 without affine or with one channel per group; dgamma = 0 with one
    channel per group, where sum_hw xh = 0): a relative error against that zero says nothing, so such a gradient is
    measured against the size of its terms (deviation())."""
    x, gamma, beta, gy = inputs(tag)
    (n, c), groups = x.shape[:2], CASES[tag][1]
    x = x.double()
    gy = torch.full_like(x, 1.0 / x.numel()) if mean_gy else gy.double()
    bc = (1, c) + (1,) * (x.dim() - 2)
    gm = gamma.double().reshape(bc) if affine else torch.ones(bc, dtype=torch.float64)
    bt = beta.double().reshape(bc) if affine else torch.zeros(bc, dtype=torch.float64)
    xh = torch.nn.functional.group_norm(x, groups, None, None, 1e-5)
    v = (xh * gm + bt).requires_grad_(True)
    gv, = torch.autograd.grad(ACT_FNS[act](v), v, gy)
    rstd = torch.rsqrt(x.reshape(n, groups, -1).var(dim=2, unbiased=False) + 1e-5)
    rstd = rstd.repeat_interleave(c // groups, dim=1).reshape((n, c) + (1,) * (x.dim() - 2))
    per_c = lambda t: t.abs().reshape(n, c, -1).sum(dim=(0, 2))
    norm = lambda t: float(torch.linalg.vector_norm(t))
    return norm(rstd * gv * gm), norm(per_c(gv * xh)), norm(per_c(gv))


def deviation(got, want, scale):
    """relative L2 of got against want; against `scale` (term_norms) where want is an exact cancellation"""
    if float(torch.linalg.vector_norm(want)) < 1e-6 * scale:
        return float(torch.linalg.vector_norm(got.detach().double().cpu() - want)) / scale
    return rel_l2(got, want)


def test_header_table_and_library_carry_the_groupnorm_training_entries():
    src = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"include/dlwp_hip.h does not declare {name}"
        assert name in L.SIGNATURES, f"lib.SIGNATURES lacks {name}"
        assert hasattr(lib, name), f"libdlwp_hip.so does not export {name}"
    assert len(L.SIGNATURES["dlwp_groupnorm_act_fwd_stats_f32"][1]) == len(L.SIGNATURES["dlwp_groupnorm_act_f32"][1]) + 1
    assert len(L.SIGNATURES["dlwp_groupnorm_act_bwd_f32"][1]) == 15
    assert lib.dlwp_groupnorm_act_bwd_workspace_bytes(3, 5) == 2 * 3 * 5 * 4
    assert lib.dlwp_groupnorm_act_bwd_workspace_bytes(0, 5) == 0 and lib.dlwp_groupnorm_act_bwd_workspace_bytes(3, -1) == 0


def test_backward_entry_refuses_bad_arguments_before_touching_the_device():
    lib = L.load()
    one = 16                                           # any non-null pointer: the checks come before the first launch
    args = lambda **k: [k.get("x", one), k.get("stats", one), None, None, k.get("gy", one), None, None, None, k.get("ws", one),
                        k.get("batch", 2), k.get("channels", 6), k.get("hw", 4), k.get("groups", 3), k.get("act", 1), None]
    for bad in (dict(groups=4), dict(act=5), dict(act=-1), dict(x=None), dict(stats=None), dict(gy=None), dict(ws=None),
                dict(batch=0), dict(channels=0), dict(hw=0), dict(groups=0)):
        assert lib.dlwp_groupnorm_act_bwd_f32(*args(**bad)) == -1, bad          # DLWP_ERR_INVALID_ARGUMENT
    assert lib.dlwp_groupnorm_act_fwd_stats_f32(one, None, None, one, None, 2, 6, 4, 3, 1e-5, 0, None) == -1


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("tag", list(CASES))
def test_backward_formulas_in_fp32_match_fp64_autograd(tag, act, affine):
    from dlwp_benchmark_amd.training import groupnorm_act_backward_torch

    x, gamma, beta, gy = inputs(tag)
    groups = CASES[tag][1]
    if not affine:
        gamma = beta = None
    n, c = x.shape[:2]
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(dim=2)
    rstd = torch.rsqrt(xg.var(dim=2, unbiased=False) + 1e-5)
    dx, dgamma, dbeta = groupnorm_act_backward_torch(x, mean, rstd, gamma, beta, gy, groups, act)
    assert dx.dtype == torch.float32 and dx.shape == x.shape and dgamma.shape == (c,) and dbeta.shape == (c,)
    want = reference(tag, act, affine)
    errs = {"dx": rel_l2(dx, want[0])}
    if affine:
        errs["dgamma"], errs["dbeta"] = rel_l2(dgamma, want[1]), rel_l2(dbeta, want[2])
    print(tag, act, affine, {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= 1e-5, errs
