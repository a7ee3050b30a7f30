"""The Navier-Stokes scheme without a GPU: the float64 restatement tests/ns_ref.py (what pins csrc/navier_stokes.hip; the
reference tree holds no solver) against a closed-form solution and its own order in dt, and the C ABI of the new entry point."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ns_ref as R
from dlwp_benchmark_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [32, 64])
def test_taylor_green_vortex_decays_in_closed_form(n):
    """cos(2 pi m a) cos(2 pi m b) without forcing: the advection term vanishes identically, so 100 sub-steps multiply the
    field by ((1 - dt nu lam / 2) / (1 + dt nu lam / 2))^100 with lam = 8 pi^2 m^2 (measured: 5e-15)"""
    m, nu, dt, steps = 2, 1e-2, 1e-3, 100
    w0 = R.taylor_green(n, m)
    out = R.solve(w0[None], 2, steps, dt, nu, forcing=None, dtype=np.float64)
    want = R.taylor_green_decay(m, steps, dt, nu) * w0
    assert np.abs(out[0, 0] - w0).max() <= 1e-12
    assert np.abs(out[0, 1] - want).max() <= 1e-12
    assert 0.3 < R.taylor_green_decay(m, steps, dt, nu) < 0.8       # the decay is no rounding matter


def test_scheme_is_first_order_in_dt():
    """E(dt) = |run(dt) - run(dt / 4)| at a fixed end time: E(dt) / E(dt / 2) = 2 for a first-order scheme (a mis-scaled step
    would not converge to the same field at all, a second-order scheme gives 4)"""
    n, t_end = 32, 0.064
    w0 = R.gaussian_random_field(np.random.default_rng(7).standard_normal((1, n, n)))
    run = lambda dt: R.solve(w0, 2, int(round(t_end / dt)), dt, 1e-3)[0, 1]
    runs = {k: run(4e-3 / k) for k in (1, 2, 4, 8)}
    e1 = np.linalg.norm(runs[1] - runs[4])
    e2 = np.linalg.norm(runs[2] - runs[8])
    assert e2 > 0 and 1.5 <= e1 / e2 <= 2.5, e1 / e2


def test_restatement_conventions():
    n = 32
    lap, lapi, mask, nyquist = R.tables(n)
    assert lap[0, 0] == 0 and lapi[0, 0] == 1 and np.array_equal(lap.ravel()[1:], lapi.ravel()[1:])
    assert mask.sum() == 21 * 11 and not mask[nyquist].any()       # |ka| <= 10: 21 rows; kb <= 10: 11 columns
    amp = R.grf_amplitude(n)
    assert amp[0, 0] == 0 and not amp[nyquist].any() and amp[1, 0] == pytest.approx(n * 2 ** 0.5 * 7 ** 1.5 * (4 * np.pi ** 2 + 49) ** -1.25)
    # frame 0 is the band-limited initial condition; the float32 form stores float32
    w0 = np.random.default_rng(1).standard_normal((2, n, n))
    out = R.solve(w0, 1, 1, 1e-3, 1e-3)
    spec = np.fft.rfft2(out[:, 0])
    assert np.abs(spec[:, nyquist]).max() <= 1e-12 * np.abs(spec).max()
    keep = ~nyquist
    assert np.allclose(spec[:, keep], np.fft.rfft2(w0)[:, keep], rtol=0, atol=1e-10)
    assert R.solve(w0, 2, 3, 1e-3, 1e-3, dtype=np.float32).dtype == np.float32
    # field standard deviation of the random initial condition (0.29 at N = 64 in expectation)
    std = R.gaussian_random_field(np.random.default_rng(2).standard_normal((64, 64, 64))).std()
    assert 0.25 < std < 0.33


def test_c_abi_declares_types_and_exports_the_entry_point():
    name = "dlwp_ns2d_rollout_f32"
    header = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    comment = header[:header.index("int32_t " + name)].rsplit("/*", 1)[1]
    assert "PARITY UNPINNED" in comment and "DESIGN.md section 38" in comment
    proto = re.search(r"int32_t\s+" + name + r"\s*\(([^()]*)\)\s*;", header).group(1)
    params = [p.strip() for p in proto.split(",")]
    assert [p.split()[-1] for p in params] == ["w0_dev", "filter_dev", "forcing_dev", "out_dev", "batch", "n", "frames", "substeps",
                                               "dt", "nu", "stream"]
    res, args = L.SIGNATURES[name]
    assert res is ctypes.c_int32 and len(args) == len(params)
    assert args[8] is ctypes.c_double and args[9] is ctypes.c_double and args[4:8] == [ctypes.c_int32] * 4
    assert hasattr(L.load(), name)


def test_ops_refuse_cpu_tensors():
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.synthetic import NavierStokes2D

    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        ops.navier_stokes_2d(torch.zeros(1, 32, 32), 2, 10, 1e-3, 1e-3)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        ops.gaussian_random_field((1, 32, 32), seed=0, device="cpu")
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        ops.gaussian_random_field(torch.zeros(1, 32, 32), seed=0)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        NavierStokes2D(n=32, device="cpu").initial(2)


def test_windows_hold_every_window_of_every_trajectory():
    from dlwp_benchmark_amd.synthetic import NavierStokes2D

    prog = torch.arange(2 * 5, dtype=torch.float32).reshape(2, 5, 1, 1, 1).expand(2, 5, 1, 4, 4)
    x, y = NavierStokes2D.windows(prog, 2, 1)
    assert x.shape == (8, 2, 1, 4, 4) and y.shape == (8, 1, 1, 4, 4)
    assert x[:, :, 0, 0, 0].tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [5, 6], [6, 7], [7, 8], [8, 9]]
    assert torch.equal(y, x[:, 1:])
    x3, y3 = NavierStokes2D.windows(prog, 4, 2)
    assert x3.shape == (4, 4, 1, 4, 4) and y3[:, :, 0, 0, 0].tolist() == [[2, 3], [3, 4], [7, 8], [8, 9]]
    with pytest.raises(ValueError):
        NavierStokes2D.windows(prog, 6, 1)
