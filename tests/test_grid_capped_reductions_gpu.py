"""Kernels whose grid is capped and that loop over the rest: LayerNorm (csrc/norm.hip) and the latitude-weighted metric
sums (csrc/metrics.hip), at the sizes where the cap or the plane split actually takes effect, against float64.

  * layernorm_kernel<LPR, NV>: norm::launch caps the grid at 4 096 workgroups of 4 waves, each wave holding 64 / LPR rows,
    so the grid-stride loop runs a second time from 65 536 (LPR 16: C <= 64), 32 768 (LPR 32: C <= 128) or 16 384 rows
    (LPR 64) on.  C3 at the benchmark's batch normalises 65 536 rows of C = 96.
  * weighted_sums_kernel: weighted_sums (csrc/metrics.hip) splits each (b, k, c) plane into ceil(H*W / 8192) slices of
    ceil(H*W / chunks) cells, the last one ragged: 4 slices at 128x256, 127 at 721x1440."""
import numpy as np
import pytest
import torch

from helpers import rel_l2

DEV = "cuda:0"


def layernorm_instance(C):
    """layernorm_prebias (csrc/norm.hip): (LPR, NV) for C channels"""
    nvec = C // 4
    if nvec <= 16:
        return 16, 1
    if nvec <= 32:
        return 32, 1
    nv = (nvec + 63) // 64
    return 64, {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6}.get(nv, 8)


def stride_threshold(C):
    """rows from which norm::launch's capped grid (4 096 blocks x 4 waves x 64 / LPR rows) loops"""
    lpr, _ = layernorm_instance(C)
    return 4096 * 4 * (64 // lpr)


LN_WIDTHS = [64, 96, 192, 384, 768, 1024, 1536, 2048]


def test_layernorm_widths_cover_every_instance():
    assert {layernorm_instance(c) for c in LN_WIDTHS} == {(16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4), (64, 6), (64, 8)}
    assert [stride_threshold(c) for c in (64, 96, 192)] == [65536, 32768, 16384]


@pytest.mark.gpu
@pytest.mark.parametrize("c", LN_WIDTHS)
def test_layernorm_past_the_grid_cap(c):
    """fp32 LayerNorm with and without the pre-bias, and the bf16-output form, at 2 x the stride threshold plus a ragged
    wave (rows % (64 / LPR) != 0)"""
    from dlwp_benchmark_amd import ops

    rows = 2 * stride_threshold(c) + 37
    g = torch.Generator(device=DEV).manual_seed(c)
    x = torch.randn(rows, c, device=DEV, generator=g) * 3.0 + 1.5
    w = 1.0 + 0.3 * torch.randn(c, device=DEV, generator=g)
    b = 0.3 * torch.randn(c, device=DEV, generator=g)
    pre = 0.5 * torch.randn(c, device=DEV, generator=g)
    F = torch.nn.functional
    with torch.no_grad():
        for tag, pb in (("plain", None), ("prebias", pre)):
            got = ops.layer_norm(x, w, b, 1e-5, pre_bias=pb)
            xin = x.double() if pb is None else x.double() + pb.double()
            want = F.layer_norm(xin, (c,), w.double(), b.double(), 1e-5)
            err = rel_l2(got, want)
            row_err = (got.double() - want).abs().amax(dim=1)
            print(f"layernorm C={c} rows={rows} {tag}: rel-L2 {err:.3e}, worst row max-abs {row_err.max().item():.3e}")
            assert err < 5e-7, (tag, err)
            assert row_err.max().item() <= 1e-5 * want.abs().max().item(), tag     # no row left out or written twice
            if pb is not None:
                got16 = ops.layer_norm(x, w, b, 1e-5, pre_bias=pb, out_dtype=torch.bfloat16)
                assert got16.dtype == torch.bfloat16 and torch.equal(got16, got.bfloat16())


def metric_chunks(h, w):
    """weighted_sums (csrc/metrics.hip): slices per plane, cells per slice, cells of the last slice"""
    hw = h * w
    chunks = max(1, (hw + 8191) // 8192)
    per = (hw + chunks - 1) // chunks
    return chunks, per, hw - per * (chunks - 1)


def test_metric_grids_split_into_ragged_slices():
    assert metric_chunks(128, 256) == (4, 8192, 8192)
    chunks, per, last = metric_chunks(721, 1440)
    assert chunks == 127 and last < per


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,k,c", [(128, 256, 3, 4, 3), (721, 1440, 2, 2, 2)])
@pytest.mark.parametrize("with_clim", [False, True])
def test_rollout_metric_sums_on_multi_slice_grids(h, w, n, k, c, with_clim):
    """RolloutMetrics against oracle.restate.metrics.lat_weighted_metrics, with and without a climatology and a per-variable
    scale; the running-sum form (dlwp_weighted_error_sums_acc_f32) over two batches equals the sums of the whole set"""
    from dlwp_benchmark_amd.metrics import RolloutMetrics
    from oracle.restate.metrics import lat_weighted_metrics

    g = torch.Generator().manual_seed(h + n + int(with_clim))
    out = torch.randn(n, k, c, h, w, generator=g)
    tar = out + 0.1 * torch.randn(n, k, c, h, w, generator=g)
    clim = 0.3 * torch.randn(k, c, h, w, generator=g) if with_clim else None
    lats = torch.linspace(-90.0, 90.0, h) if h % 2 else torch.linspace(-90.0 + 90.0 / h, 90.0 - 90.0 / h, h)
    std = torch.tensor([2.0, 0.5, 10.0][:c])
    mean = torch.tensor([1.0, -3.0, 250.0][:c])
    o, t = out.to(DEV), tar.to(DEV)
    for scaled in (False, True):
        m = RolloutMetrics(lats, std=std if scaled else None, climatology=clim)
        want_rmse, want_acc = lat_weighted_metrics(out.numpy(), tar.numpy(), lats.numpy(), std.numpy() if scaled else None,
                                                   mean.numpy() if scaled else None, clim.numpy() if with_clim else None)
        got = m(o, t)
        np.testing.assert_allclose(got["rmse"].cpu().numpy(), want_rmse, rtol=2e-6)
        if with_clim:
            np.testing.assert_allclose(got["acc"].cpu().numpy(), want_acc, rtol=2e-6, atol=1e-7)
        else:
            assert got["acc"] is None
        run = torch.zeros(4, k, c, dtype=torch.float64, device=DEV)
        assert m.sums(o[:1], t[:1], into=run) is run
        m.sums(o[1:], t[1:], into=run)
        whole = m.sums(o, t)
        assert torch.allclose(run, whole, rtol=1e-12, atol=0)
        acc = m.finalize(run, float(n), h * w)
        np.testing.assert_allclose(acc["rmse"].cpu().numpy(), want_rmse, rtol=2e-6)
        print(f"metrics {h}x{w} clim={with_clim} scaled={scaled}: rmse max rel err "
              f"{np.max(np.abs(got['rmse'].cpu().numpy() / want_rmse - 1)):.3e}")
