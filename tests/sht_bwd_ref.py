"""References of the backwards of the spherical transforms and the Driscoll-Healy mix -- shared by tests/test_sht_bwd_cpu.py,
tests/test_sht_bwd_gpu.py and tests/test_sfno_train_hip_gpu.py.  Imports nothing from the product.

Two kinds, as tests/sht_ref.py has for the forwards:
  *_f32      float32 numpy restatements of the four backward operators from their closed forms, with
             the SAME fp32 tables and twiddles as the device and fp32 accumulation: they set the tolerance of the kernels.
  truth_*    float64, by autograd of sht_ref.sht / isht / sph_mix -- independent of the closed forms.
Gradients of complex tensors follow torch's convention g = dL/dRe + i dL/dIm.
"""
import math

import numpy as np
import torch

import sht_ref as R


def _lower(a):
    return np.where(np.tril(np.ones(a.shape[-2:], dtype=bool)), a, 0).astype(a.dtype)


# ---- float32 restatements -----------------------------------------------------------------------------------------------------
def sht_bwd_f32(g64, wleg32, tw32, nlon: int):
    """g64 complex64 [..., lmax, mmax] (l < m not read), wleg32 [mmax, lmax, nlat] (P w) -> float32 [..., nlat, nlon]"""
    mmax = wleg32.shape[0]
    g = _lower(g64)
    scale = np.float32(2.0 * math.pi / nlon)
    yr = np.einsum("mlk,...lm->...km", wleg32, np.ascontiguousarray(g.real, dtype=np.float32)) * scale
    yi = np.einsum("mlk,...lm->...km", wleg32, np.ascontiguousarray(g.imag, dtype=np.float32)) * scale
    dr, di = R._dft_f32(tw32, nlon, mmax)
    return (yr @ dr.T + yi @ di.T).astype(np.float32)


def isht_bwd_f32(gy32, leg32, tw32):
    """gy32 float32 [..., nlat, nlon], leg32 [mmax, lmax, nlat] (P, zero for l < m) -> complex64 [..., lmax, mmax]"""
    nlon, mmax = gy32.shape[-1], leg32.shape[0]
    dr, di = R._dft_f32(tw32, nlon, mmax)
    f = np.full(mmax, 2.0, dtype=np.float32)
    zr, zi = gy32 @ dr, gy32 @ di
    for m in range(mmax):
        if m == 0 or 2 * m == nlon:
            f[m] = 1.0
            zi[..., m] = 0.0
    zr, zi = zr * f, zi * f
    return (np.einsum("mlk,...km->...lm", leg32, zr) + 1j * np.einsum("mlk,...km->...lm", leg32, zi)).astype(np.complex64)


def sph_mix_dgrad_f32(g64, w64):
    """g64 complex64 [B, Co, lmax, mmax], w64 complex64 [Ci, Co, lmax] -> complex64 [B, Ci, lmax, mmax], zero above the diagonal"""
    return _lower(np.einsum("bolm,iol->bilm", _lower(g64), np.conj(w64).astype(np.complex64)).astype(np.complex64))


def sph_mix_wgrad_f32(c64, g64):
    """c64 complex64 [B, Ci, lmax, mmax], g64 complex64 [B, Co, lmax, mmax] -> complex64 [Ci, Co, lmax]"""
    return np.einsum("bilm,bolm->iol", np.conj(_lower(c64)).astype(np.complex64), _lower(g64)).astype(np.complex64)


# ---- float64 truth by autograd of sht_ref -------------------------------------------------------------------------------------
def _vjp(fn, inputs, cotangent):
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(torch.complex128 if np.iscomplexobj(a) else torch.float64)
           .requires_grad_(True) for a in inputs]
    out = fn(*ins)
    cot = torch.from_numpy(np.ascontiguousarray(cotangent)).to(out.dtype)
    return [t.numpy() for t in torch.autograd.grad(out, ins, cot)]


def truth_sht_bwd(g, p, w, nlat: int, nlon: int):
    """p [mmax, lmax, nlat], w [nlat] float64 tables -> float64 [..., nlat, nlon]"""
    zero = np.zeros(g.shape[:-2] + (nlat, nlon))
    return _vjp(lambda x: R.sht(x, p, w), [zero], g)[0]


def truth_isht_bwd(gy, p, lmax: int, mmax: int):
    zero = np.zeros(gy.shape[:-2] + (lmax, mmax), dtype=np.complex128)
    return _vjp(lambda c: R.isht(c, p, gy.shape[-1]), [zero], gy)[0]


def truth_sph_mix_bwd(c, wt, g):
    """(gc_in, gw) in complex128"""
    return _vjp(R.sph_mix, [c, wt], g)


def rel(a, b) -> float:
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def triangular(rng, lead, lmax, mmax):
    c = rng.standard_normal(lead + (lmax, mmax)) + 1j * rng.standard_normal(lead + (lmax, mmax))
    return c * np.tril(np.ones((lmax, mmax)))


def dot64(a, b) -> float:
    """Re sum a conj(b), summed in float64"""
    return float(np.sum((np.asarray(a).astype(np.complex128) * np.conj(np.asarray(b).astype(np.complex128))).real))
