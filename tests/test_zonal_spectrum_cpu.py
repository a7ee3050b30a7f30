"""Zonal energy spectrum / MELR without a GPU: the numpy restatement (tests/zonal_spectrum_ref.py) against identities of
its definition, the cross-rank part of ZonalSpectrumMetrics.finalize (gloo, two ranks, unequal shards) against the whole
batch, and the refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dlwp_benchmark_amd.lib import DlwpError
from dlwp_benchmark_amd.metrics import ZonalSpectrumMetrics, circumference_weights
from dlwp_benchmark_amd.sharding import shard_bounds
from zonal_spectrum_ref import circumference, melr, zonal_energy, zonal_power


@pytest.mark.parametrize("w", [32, 64, 256])
def test_parseval_with_the_doubled_nyquist_bin(w):
    f = np.random.default_rng(w).standard_normal((7, w))
    p = zonal_power(f)
    nyq = np.abs(np.fft.rfft(f, axis=-1, norm="forward")[:, -1]) ** 2
    assert np.allclose(p.sum(-1), (f ** 2).mean(-1) + nyq, rtol=1e-13, atol=0)


@pytest.mark.parametrize("w,m0,phi", [(32, 1, 0.3), (64, 5, -1.1), (256, 127, 2.0), (512, 64, 0.0)])
def test_pure_zonal_wave_fills_one_bin(w, m0, phi):
    a = 1.7
    n = np.arange(w)
    p = zonal_power(a * np.cos(2 * np.pi * m0 * n / w + phi))
    assert abs(p[m0] - a * a / 2) <= 1e-12
    others = np.delete(p, m0)
    assert np.all(np.abs(others) <= 1e-12)


def test_constant_field_is_all_in_bin_zero():
    p = zonal_power(np.full((3, 64), -2.5))
    assert abs(p[:, 0] - 6.25).max() <= 1e-12
    assert np.abs(p[:, 1:]).max() <= 1e-12


def test_identical_fields_have_zero_melr():
    x = np.random.default_rng(0).standard_normal((2, 3, 2, 8, 32))
    res = melr(x, x.copy())
    assert np.all(res["log_ratio"] == 0.0) and np.all(res["melr"] == 0.0)


def test_energy_weights_circles_of_latitude():
    # a constant field c: E = c^2 * mean_h circ_h in bin 0
    lats = np.linspace(-90, 90, 9)
    e = zonal_energy(np.full((2, 1, 1, 9, 32), 3.0), lats)
    assert np.allclose(e[0, 0, 0], 9.0 * circumference(lats).mean(), rtol=1e-13)
    assert np.allclose(circumference_weights(torch.from_numpy(lats)).numpy(), circumference(lats), rtol=1e-14, atol=1e-6)


def test_cpu_tensors_are_refused():
    m = ZonalSpectrumMetrics(torch.linspace(-90, 90, 8))
    x = torch.zeros(1, 1, 1, 8, 32)
    with pytest.raises(DlwpError, match="no CPU fallback"):
        m.sums(x, x)


# ---------------------------------------------------------------------------------------------------------------
# two ranks: ZonalSpectrumMetrics with the HIP sums kernel replaced by its definition (include/dlwp_hip.h) in float64
# torch; what is under test is the cross-rank part of finalize against the restatement on the whole batch
# ---------------------------------------------------------------------------------------------------------------
class _CpuZonal(ZonalSpectrumMetrics):
    def sums(self, out, target, into=None):
        res = torch.stack([self._power_sum(out), self._power_sum(target)])
        return res if into is None else into.add_(res)

    def _power_sum(self, x):
        fk = torch.fft.rfft(x.double(), dim=-1, norm="forward")
        p = fk.real ** 2 + fk.imag ** 2
        p[..., 1:] *= 2
        return (p * self.circ[:, None]).sum(dim=(0, 3))


def _inputs():
    g = torch.Generator().manual_seed(5)
    out = torch.randn(5, 3, 2, 8, 32, generator=g)
    tar = out + 0.3 * torch.randn(5, 3, 2, 8, 32, generator=g)
    return out, tar, torch.linspace(-90, 90, 8)


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out, tar, lats = _inputs()
        lo, hi = shard_bounds(out.shape[0], world, rank)   # 3 + 2 samples
        res = _CpuZonal(lats)(out[lo:hi], tar[lo:hi], world_size=world)
        ret[rank] = {k: v.clone() for k, v in res.items()}
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_rank_finalize_matches_whole_batch():
    world = 2
    ret = mp.Manager().dict()
    port = 35500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    out, tar, lats = _inputs()
    want = melr(out.numpy(), tar.numpy(), lats.numpy())
    single = _CpuZonal(lats)(out, tar)
    for r in range(world):
        got = ret[r]
        for key in ("energy_pred", "energy_true", "log_ratio", "melr"):
            assert got[key].dtype == torch.float64
            assert torch.allclose(got[key], single[key], rtol=1e-13, atol=1e-15), (r, key)
            assert np.allclose(got[key].numpy(), want[key], rtol=1e-10, atol=1e-12), (r, key)
