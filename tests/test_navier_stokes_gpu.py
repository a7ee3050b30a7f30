"""ops.navier_stokes_2d / ops.gaussian_random_field (csrc/navier_stokes.hip) against the float64 restatement tests/ns_ref.py, the
closed-form decay of a Taylor-Green vortex, and themselves (bitwise).  The reference tree holds no solver -- PARITY UNPINNED.

Bounds: the kernel may be at most 4 times as far from float64 as the float32 restatement (numpy's single-precision transforms,
float32 storage between operations) is, both measured in the test.  The kernel's radix split and summation order differ from
pocketfft's; a missing factor or mask shows at 1e-2 or worse.  Measured on MI355X (kernel / float32 restatement, rel-L2; DESIGN.md
section 38.5):
  against float64, 100 sub-steps       N = 32: 1.96e-6 / 3.61e-6    N = 64: 2.75e-6 / 3.78e-6
  Taylor-Green against the closed form N = 32: 2.99e-6 / 4.08e-6    N = 64: 3.00e-6 / 4.09e-6
  gaussian_random_field                N = 32: 1.39e-7 / 1.12e-7    N = 64: 1.58e-7 / 1.19e-7
"""
import numpy as np
import pytest
import torch

import ns_ref as R
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd.lib import DlwpError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NU, DT = 1e-3, 1e-3


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@pytest.fixture(scope="module")
def grf():
    """per N: the kernel's own band-limited GRF initial condition, on the host (float32 values)"""
    return {n: ops.gaussian_random_field((3, n, n), seed=11, device=DEV).cpu().numpy() for n in (32, 64)}


@pytest.mark.parametrize("n", [32, 64])
def test_against_float64(n, grf):
    w0 = grf[n]
    want = R.solve(w0, 3, 50, DT, NU, dtype=np.float64)
    ref32 = R.solve(w0, 3, 50, DT, NU, dtype=np.float32)
    got = ops.navier_stokes_2d(_gpu(w0), 3, 50, DT, NU).cpu().numpy()
    assert got.shape == (3, 3, n, n)
    e_ref, e_hip = R.rel_l2(ref32[:, -1], want[:, -1]), R.rel_l2(got[:, -1], want[:, -1])
    e_mid, e_first = R.rel_l2(got[:, 1], want[:, 1]), R.rel_l2(got[:, 0], want[:, 0])
    print(f"ns2d N={n}: 100 sub-steps rel-L2 against float64: kernel {e_hip:.3e}, float32 restatement {e_ref:.3e}; "
          f"50 sub-steps {e_mid:.3e}; frame 0 {e_first:.3e}")
    assert e_hip <= 4 * e_ref
    assert e_mid <= 4 * e_ref and e_first <= 4 * e_ref        # the earlier frames are no further away than the last may be


@pytest.mark.parametrize("n", [32, 64])
def test_taylor_green_decay(n):
    m, nu, steps = 2, 1e-2, 100
    w0 = R.taylor_green(n, m)
    want = R.taylor_green_decay(m, steps, DT, nu) * w0
    ref32 = R.solve(w0[None], 2, steps, DT, nu, forcing=None, dtype=np.float32)[0, 1]
    got = ops.navier_stokes_2d(_gpu(w0[None]), 2, steps, DT, nu, forcing=None)[0, 1].cpu().numpy()
    e_ref, e_hip = R.rel_l2(ref32, want), R.rel_l2(got, want)
    print(f"ns2d N={n}: Taylor-Green m=2 after 100 sub-steps against the closed form: kernel {e_hip:.3e}, float32 restatement {e_ref:.3e}")
    assert e_hip <= 4 * e_ref


@pytest.mark.parametrize("n", [32, 64])
def test_gaussian_random_field(n):
    z = ops.philox_normal((3, n, n), seed=5, offset=64, device=DEV)
    got = ops.gaussian_random_field((3, n, n), seed=5, offset=64, device=DEV).cpu().numpy()
    zh = z.cpu().numpy()
    want = R.gaussian_random_field(zh, dtype=np.float64)
    ref32 = R.gaussian_random_field(zh, dtype=np.float32)
    e_ref, e_hip = R.rel_l2(ref32, want), R.rel_l2(got, want)
    print(f"grf N={n}: rel-L2 against float64: kernel {e_hip:.3e}, float32 restatement {e_ref:.3e}; std {got.std():.4f}")
    assert e_hip <= 4 * e_ref
    spec = np.abs(np.fft.rfft2(got.astype(np.float64)))
    assert max(spec[:, n // 2, :].max(), spec[:, :, n // 2].max()) <= 1e-6 * spec.max()
    # an explicit filter through navier_stokes_2d is the same launch
    amp = ops.grf_amplitude(n, 7.0, 2.5, DEV)
    same = ops.navier_stokes_2d(z, 1, 1, 1.0, 0.0, forcing=None, filter=amp)[:, 0]
    assert torch.equal(same.cpu(), torch.from_numpy(got))


def test_trajectory_does_not_depend_on_the_batch():
    """259 workgroups (more than the device has compute units) against trajectories run alone"""
    n, b = 32, 259
    w0 = ops.gaussian_random_field((b, n, n), seed=3, device=DEV)
    full = ops.navier_stokes_2d(w0, 2, 10, DT, NU)
    for k in (0, 100, 258):
        alone = ops.navier_stokes_2d(w0[k:k + 1].clone(), 2, 10, DT, NU)
        assert torch.equal(alone[0], full[k]), k
    assert bool(torch.isfinite(full).all()) and float(full[:, 1].std()) > 0.1


@pytest.mark.parametrize("n", [32, 64])
def test_frames_divide_one_integration(n):
    """the state never leaves spectral space: 5 frames of 20 sub-steps and 2 frames of 80 share frames 0 and 80, bit for bit;
    and a call repeated gives the same bits"""
    w0 = ops.gaussian_random_field((2, n, n), seed=9, device=DEV)
    fine = ops.navier_stokes_2d(w0, 5, 20, DT, NU)
    coarse = ops.navier_stokes_2d(w0, 2, 80, DT, NU)
    assert torch.equal(fine[:, 0], coarse[:, 0]) and torch.equal(fine[:, 4], coarse[:, 1])
    assert torch.equal(ops.navier_stokes_2d(w0, 5, 20, DT, NU), fine)
    assert not torch.equal(fine[:, 3], fine[:, 4])


def test_refusals(monkeypatch):
    from dlwp_benchmark_amd import lib as L

    w0 = torch.zeros(1, 32, 32, device=DEV)
    with pytest.raises(DlwpError, match="32 x 32 and 64 x 64") as e:
        ops.navier_stokes_2d(torch.zeros(1, 48, 48, device=DEV), 2, 10, DT, NU)
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(DlwpError, match="exceeds") as e:
        ops.navier_stokes_2d(w0, 3, ops.NS2D_MAX_STEPS // 3 + 1, DT, NU)
    assert e.value.status == L.ERR_UNSUPPORTED
    # refused before the library is reached
    def forbidden(*a, **k):
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(L, "launch", forbidden)
    with pytest.raises(DlwpError, match=r"\[B, N, N\]"):
        ops.navier_stokes_2d(torch.zeros(1, 32, 64, device=DEV), 2, 10, DT, NU)
    with pytest.raises(DlwpError, match="forcing must be"):
        ops.navier_stokes_2d(w0, 2, 10, DT, NU, forcing=torch.zeros(32, 17, device=DEV))
    with pytest.raises(DlwpError, match="no CPU fallback"):
        ops.navier_stokes_2d(w0.cpu(), 2, 10, DT, NU)
