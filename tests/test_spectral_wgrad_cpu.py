"""Spectral weight gradient, CPU side: the fixtures the REAL reference SpectralConv2d produced at rectangular channel
counts, a kept Nyquist column and a 40-sample batch (tests/golden/spectral_wgrad_*.npz, tools/make_golden_spectral_grad.py)
against `training.spectral_weight_grad` and the adjoint identity in double -- this pins fixtures and formula to each
other before any GPU run -- and the C ABI of the HIP weight-gradient entry.  No GPU needed."""
import os
import re
import sys

import pytest
import torch

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd.training import pde_arena_rows, spectral_weight_grad
from helpers import load_golden, rel_l2
from oracle.restate.fno import spectral_conv2d_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["c24x40_32x64_m8x6_b3", "c12x4_16x16_m4_b2", "c5x2_12x20_m3x11_b2", "c32_32x64_m8x6_b40"]
NEW_SYMBOLS = ["dlwp_spectral_conv2d_wgrad_workspace_bytes", "dlwp_spectral_conv2d_wgrad_f32"]


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_spectral_grad as tool
    finally:
        sys.path.pop(0)
    return tool


def test_fixture_cases_match_the_tool():
    tool = _tool()
    assert sorted(tool.CASES) == sorted(TAGS)
    for tag in TAGS:
        assert tuple(int(v) for v in load_golden(f"spectral_wgrad_{tag}")["case"]) == tool.CASES[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_weight_gradient_and_adjoint_match_reference_gradients(tag):
    """fixtures are fp32 autograd of the real class; the formula runs in double here, so the bound is the fixtures' own
    fp32 rounding (2e-6, the bound tests/test_training_cpu.py uses for the two older fixtures)"""
    tool = _tool()
    ci, co, h, w, m1, m2, b = tool.CASES[tag]
    g = load_golden(f"spectral_wgrad_{tag}")
    x, w1, w2, r = tool.case_tensors(tag)
    assert tool.tensor_sha(x, w1, w2, r) == str(g["sha"]), "filler drifted: regenerate fixtures"
    rows, _ = pde_arena_rows(h, m1)
    gw = spectral_weight_grad(x.double(), r.double(), rows, rows, m2, 1.0, 1.0 / (h * w))
    assert tuple(gw.shape) == (ci, co, 2 * m1, m2, 2)
    assert rel_l2(gw[:, :, :m1], torch.from_numpy(g["gw1"])) < 2e-6
    assert rel_l2(gw[:, :, m1:], torch.from_numpy(g["gw2"])) < 2e-6
    # backward-data = the co -> ci operator with conjugate-transposed weights
    adj = lambda t: torch.view_as_real(torch.view_as_complex(t.contiguous()).conj().transpose(0, 1).contiguous())
    gx = spectral_conv2d_ref(r, adj(w1), adj(w2))
    y = spectral_conv2d_ref(x, w1, w2)
    if "gx" in g.files:
        assert rel_l2(gx, torch.from_numpy(g["gx"])) < 2e-6
        assert rel_l2(y, torch.from_numpy(g["y"])) < 2e-6
    assert rel_l2(gx[0, :4], torch.from_numpy(g["gx_head"])) < 2e-6
    assert rel_l2(y[0, :4], torch.from_numpy(g["y_head"])) < 2e-6
    assert abs(float(gx.double().norm()) - float(g["gx_norm"])) <= 2e-6 * float(g["gx_norm"])
    proj = float((gx.double() * tool.gx_probe(tag).double()).sum())
    # a projection on a random direction is a sum of ~N terms of random sign: bound it by the norms, not by itself
    assert abs(proj - float(g["gx_proj"])) <= 2e-6 * float(g["gx_norm"]) * float(tool.gx_probe(tag).double().norm())


def test_rectangular_weight_gradient_matches_autograd_in_double():
    """FNO geometry at Ci != Co: distinct rows_in / rows_out, forward-normalised transforms, Nyquist column kept."""
    torch.manual_seed(5)
    b, ci, co, h, w, n_cols = 3, 3, 5, 12, 16, 9
    rows_in, rows_out = [0, 1, 2, 10, 11], [1, 2, 3, 11, 0]
    fwd, inv = 1.0 / (h * w), 1.0

    def op(x, wt, ri, ro):
        xf = torch.fft.rfft2(x) * fwd
        out = torch.zeros(x.shape[0], wt.shape[1], h, w // 2 + 1, dtype=torch.complex128)
        out[:, :, ro, :n_cols] = torch.einsum("bixy,ioxy->boxy", xf[:, :, ri, :n_cols], wt)
        return torch.fft.irfft2(out, s=(h, w)) * (h * w) * inv

    x = torch.randn(b, ci, h, w, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(ci, co, len(rows_in), n_cols, dtype=torch.complex128, requires_grad=True)
    y = op(x, wt, rows_in, rows_out)
    r = torch.randn_like(y)
    (y * r).sum().backward()
    assert rel_l2(op(r, wt.detach().conj().transpose(0, 1), rows_out, rows_in), x.grad) < 1e-12
    gw = spectral_weight_grad(x.detach(), r, rows_in, rows_out, n_cols, fwd, inv)
    assert rel_l2(gw, torch.view_as_real(wt.grad)) < 1e-12


def test_header_table_and_library_carry_the_weight_gradient_entries():
    src = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"include/dlwp_hip.h does not declare {name}"
        assert name in L.SIGNATURES, f"lib.SIGNATURES lacks {name}"
        assert hasattr(lib, name), f"libdlwp_hip.so does not export {name}"
    assert len(L.SIGNATURES["dlwp_spectral_conv2d_wgrad_f32"][1]) == 8
    # a null plan needs no workspace and does not touch the device
    assert lib.dlwp_spectral_conv2d_wgrad_workspace_bytes(None, 4) == 0


def test_spectral_training_path_refuses_cpu():
    from dlwp_benchmark_amd import training as T
    from dlwp_benchmark_amd.models import SpectralConv2d

    rows, _ = pde_arena_rows(16, 4)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        T.SpectralOperator(3, 16, 16, rows, rows, 4, 1.0, 1.0 / 256, "cpu", out_channels=8)
    mod = SpectralConv2d(3, 8, 4, 4).train()
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        mod(torch.zeros(1, 3, 16, 16, requires_grad=True))
