"""The yardstick of tests/test_sht_bwd_gpu.py, pinned without a GPU: the float32 restatements of the four backward operators
(tests/sht_bwd_ref.py, written from the closed forms of DESIGN.md section 35.7) against the float64 truth, which is autograd of
the independent float64 forwards of tests/sht_ref.py.  Bound 1e-5 relative L2: fp32 tables and fp32 sums of at most a few
hundred terms leave about 1e-7, so the bound only separates "the closed form is right" from "it is not" (a wrong factor,
stride or sign is an error of order one).
"""
import os
import re

import numpy as np
import pytest

import sht_bwd_ref as B
import sht_ref as R
from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import sphere as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LG, EQ = "legendre-gauss", "equiangular"
CASES = [(LG, 8, 16, 8, 8), (LG, 12, 20, 7, 5), (EQ, 9, 16, 4, 4), (LG, 12, 16, 10, 9)]     # the last: the Nyquist column
IDS = [f"{g[:2]}-{a}x{b}-l{l}-m{m}" for g, a, b, l, m in CASES]
MIX = [(1, 3, 5, 4, 4), (2, 5, 70, 9, 6)]
NEW_SYMBOLS = ["dlwp_sht_bwd_f32", "dlwp_isht_bwd_f32", "dlwp_sph_mix_dgrad_f32", "dlwp_sph_mix_wgrad_f32"]


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax", CASES, ids=IDS)
def test_sht_backward_restatement_against_float64_autograd(grid, nlat, nlon, lmax, mmax):
    rng = np.random.default_rng(21)
    g = (rng.standard_normal((3, lmax, mmax)) + 1j * rng.standard_normal((3, lmax, mmax))).astype(np.complex64)   # l < m filled too
    p, w = R.tables(grid, nlat, lmax, mmax)
    want = B.truth_sht_bwd(g, p, w, nlat, nlon)
    wleg32, _ = S.tables_f32(grid, nlat, lmax, mmax)
    err = B.rel(B.sht_bwd_f32(g, wleg32, S.twiddles(nlon).astype(np.float32), nlon), want)
    print(f"sht_bwd_f32 {grid} {nlat}x{nlon} l{lmax} m{mmax}: {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax", CASES, ids=IDS)
def test_isht_backward_restatement_against_float64_autograd(grid, nlat, nlon, lmax, mmax):
    rng = np.random.default_rng(22)
    gy = rng.standard_normal((3, nlat, nlon)).astype(np.float32)
    p, _ = R.tables(grid, nlat, lmax, mmax)
    want = B.truth_isht_bwd(gy, p, lmax, mmax)
    _, leg32 = S.tables_f32(grid, nlat, lmax, mmax)
    got = B.isht_bwd_f32(gy, leg32, S.twiddles(nlon).astype(np.float32))
    err = B.rel(got, want)
    print(f"isht_bwd_f32 {grid} {nlat}x{nlon} l{lmax} m{mmax}: {err:.3e}")
    assert err <= 1e-5
    upper = np.triu(np.ones((lmax, mmax), dtype=bool), 1)
    assert np.all(got[..., upper] == 0) and np.all(want[..., upper] == 0)
    for m in range(mmax):                              # the columns irfft takes the real part of give no imaginary gradient
        if m == 0 or 2 * m == nlon:
            assert np.all(got[..., m].imag == 0) and np.all(want[..., m].imag == 0)


@pytest.mark.parametrize("b,ci,co,lmax,mmax", MIX, ids=[f"b{b}-i{i}-o{o}-l{l}-m{m}" for b, i, o, l, m in MIX])
def test_sph_mix_backward_restatements_against_float64_autograd(b, ci, co, lmax, mmax):
    rng = np.random.default_rng(23)
    c = B.triangular(rng, (b, ci), lmax, mmax).astype(np.complex64)
    g = (rng.standard_normal((b, co, lmax, mmax)) + 1j * rng.standard_normal((b, co, lmax, mmax))).astype(np.complex64)
    wt = ((rng.standard_normal((ci, co, lmax)) + 1j * rng.standard_normal((ci, co, lmax))) / np.sqrt(ci)).astype(np.complex64)
    want_c, want_w = B.truth_sph_mix_bwd(c, wt, g)
    ec, ew = B.rel(B.sph_mix_dgrad_f32(g, wt), want_c), B.rel(B.sph_mix_wgrad_f32(c, g), want_w)
    print(f"sph_mix backward b{b} ci{ci} co{co} l{lmax} m{mmax}: dgrad {ec:.3e}, wgrad {ew:.3e}")
    assert ec <= 1e-5 and ew <= 1e-5


def test_header_table_and_library_carry_the_backward_entries():
    src = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"include/dlwp_hip.h does not declare {name}"
        assert name in L.SIGNATURES, f"lib.SIGNATURES lacks {name}"
        assert hasattr(lib, name), f"libdlwp_hip.so does not export {name}"
        assert len(L.SIGNATURES[name][1]) == len(L.SIGNATURES[name.replace("_bwd", "").replace("_dgrad", "").replace("_wgrad", "")][1])
