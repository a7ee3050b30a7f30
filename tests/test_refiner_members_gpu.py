"""The member streams of csrc/refiner.hip on the GPU: ops.philox_normal_members and ops.ddpm_step(members=...).

Values are compared with tests/ensemble_ref.member_normals (philox_ref with counter word 2 = member) under the bound
tests/test_refiner_gpu.py uses for the stream against philox_ref (1e-5 absolute: the kernel's fp32 libm against float64);
everything the feature promises beyond values -- member 0 is the plain stream, a group of members is the members of any
split, the fused draw is the explicit one -- is bitwise."""
import numpy as np
import pytest
import torch

import ensemble_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM_TOL = 1e-5          # tests/test_refiner_gpu.py::test_stream_values
LAST = 2 ** 31 - 1


def _ops():
    from dlwp_benchmark_amd import ops
    return ops


def _max_err(got, seed, first, offset):
    m, n = got.shape
    got = got.cpu().numpy().astype(np.float64)
    return max(float(np.abs(got[j] - ensemble_ref.member_normals(seed, first + j, offset, n)).max()) for j in range(m))


@pytest.mark.parametrize("n", [1, 5, 4096, 4099])
def test_member_zero_is_philox_normal_bitwise(n):
    ops = _ops()
    plain = ops.philox_normal((1, n), 2024, 8, device=DEV)
    assert torch.equal(ops.philox_normal_members((1, n), 2024, 1, 0, 8, device=DEV), plain)
    # and as member 0 of a wider draw
    assert torch.equal(ops.philox_normal_members((3, n), 2024, 3, 0, 8, device=DEV)[:1], plain)


@pytest.mark.parametrize("n", [1, 5, 4096, 4099])
@pytest.mark.parametrize("first", [1, 7, LAST])
def test_member_values(n, first):
    got = _ops().philox_normal_members((1, n), 2024, 1, first, 4096, device=DEV)
    err = _max_err(got, 2024, first, 4096)
    print(f"philox_normal_members member {first} n = {n}: max abs error {err:.2e}")
    assert err <= STREAM_TOL


@pytest.mark.parametrize("n", [1, 5, 4096, 4099])
def test_several_members_in_one_call(n):
    """members 6, 7, 8 side by side: with n = 1 and 5 a thread's block of four straddles members"""
    got = _ops().philox_normal_members((3, n), 99, 3, 6, 0, device=DEV)
    err = _max_err(got, 99, 6, 0)
    print(f"philox_normal_members members 6..8 n = {n}: max abs error {err:.2e}")
    assert err <= STREAM_TOL


@pytest.mark.parametrize("n", [5, 4099])
def test_unaligned_output_view(n):
    ops = _ops()
    buf = torch.full((3 * n + 2,), 7.0, device=DEV)
    view = buf[1:3 * n + 1].view(3, n)
    assert view.data_ptr() % 16 == 4
    got = ops.philox_normal_members(view, 5, 3, 1, 0)
    assert float(buf[0]) == 7.0 and float(buf[-1]) == 7.0, "wrote outside the view"
    assert torch.equal(got, ops.philox_normal_members((3, n), 5, 3, 1, 0, device=DEV))
    assert _max_err(got, 5, 1, 0) <= STREAM_TOL


def test_above_the_grid_cap():
    """3 members whose total exceeds one sweep of the capped grid by a few workgroups: the strided loop runs, and with this
    n_per_member (4 k + 3) the blocks of four straddle members"""
    ops = _ops()
    n = (ops.refiner_grid_span() + 5 * 1024) // 3 // 4 * 4 + 3
    assert 3 * n > ops.refiner_grid_span() + 4 * 1024
    got = ops.philox_normal_members((3, n), 77, 3, 2, 4096, device=DEV)
    err = _max_err(got, 77, 2, 4096)
    print(f"philox_normal_members 3 x {n}: max abs error {err:.2e}")
    assert err <= STREAM_TOL


@pytest.mark.parametrize("n", [5, 4096, 4099])
def test_group_invariance_bitwise(n):
    ops = _ops()
    whole = ops.philox_normal_members((5, n), 31, 5, 0, 12, device=DEV)
    parts = torch.cat([ops.philox_normal_members((2, n), 31, 2, 0, 12, device=DEV),
                       ops.philox_normal_members((3, n), 31, 3, 2, 12, device=DEV)])
    assert torch.equal(whole, parts)
    # dim 0 may hold more than the members: [members * B, ...] is member-major
    assert torch.equal(ops.philox_normal_members((10, n), 31, 5, 0, 12, device=DEV).view(5, 2 * n)[:, :n],
                       ops.philox_normal_members((5, 2 * n), 31, 5, 0, 12, device=DEV)[:, :n])
    assert not torch.equal(whole[0], whole[1])


COEF = (0.8, 0.6, 0.3, 0.65, 0.25)          # sa, sb, c0, c1, sigma


@pytest.mark.parametrize("n", [5, 4096, 4099])
def test_ddpm_step_members_draws_what_philox_normal_members_draws(n):
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    sample, pred = (torch.randn(3, n, generator=g).to(DEV) for _ in range(2))
    fused = ops.ddpm_step(sample, pred, COEF, seed=17, offset=64, members=3, first_member=4)
    noise = ops.philox_normal_members((3, n), 17, 3, 4, 64, device=DEV)
    assert torch.equal(fused, ops.ddpm_step(sample, pred, COEF, noise=noise))
    assert torch.equal(fused, ops.ddpm_step(sample, pred, COEF, noise=noise, members=3, first_member=4))
    assert not torch.equal(fused, ops.ddpm_step(sample, pred, COEF, seed=17, offset=64))      # member 0 throughout
    # the members of a group are the members of the whole
    assert torch.equal(fused[1:], ops.ddpm_step(sample[1:], pred[1:], COEF, seed=17, offset=64, members=2, first_member=5))
    # in place
    work = sample.clone()
    assert ops.ddpm_step(work, pred, COEF, seed=17, offset=64, out=work, members=3, first_member=4) is work
    assert torch.equal(work, fused)


def test_ddpm_step_members_without_sigma_reads_no_noise():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    sample, pred = (torch.randn(3, 4099, generator=g).to(DEV) for _ in range(2))
    coef = COEF[:4] + (0.0,)
    garbage = torch.full((3, 4099), float("nan"), device=DEV)
    want = ops.ddpm_step(sample, pred, coef)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(ops.ddpm_step(sample, pred, coef, noise=garbage, members=3), want)
    assert torch.equal(ops.ddpm_step(sample, pred, coef, seed=5, offset=8, members=3, first_member=9), want)


def test_bad_arguments_are_refused():
    from dlwp_benchmark_amd import lib as L
    ops = _ops()
    with pytest.raises(L.DlwpError, match="divisible"):
        ops.philox_normal_members((4, 8), 0, 3, device=DEV)
    with pytest.raises(L.DlwpError, match="multiple of 4"):
        ops.philox_normal_members((3, 8), 0, 3, 0, 2, device=DEV)
    with pytest.raises(L.DlwpError, match="2\\^31"):
        ops.philox_normal_members((2, 8), 0, 2, LAST, device=DEV)
    with pytest.raises(L.DlwpError, match="2\\^31"):
        ops.philox_normal_members((2, 8), 0, 0, device=DEV)
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(L.DlwpError, match="divisible"):
        ops.ddpm_step(x, x, COEF, members=3)
    with pytest.raises(L.DlwpError) as e:
        L.launch("dlwp_philox_normal_members_f32", x.device, x, 8, 4, -1, 0, 0)
    assert e.value.status == -1      # DLWP_ERR_INVALID_ARGUMENT
