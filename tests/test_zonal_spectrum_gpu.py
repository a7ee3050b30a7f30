"""ZonalSpectrumMetrics on the device (dlwp_zonal_power_sums_f32, csrc/zonal_spectrum.hip) against the numpy restatement
of reference scripts/losses.py:16-152 (tests/zonal_spectrum_ref.py): energies per bin within rtol 1e-4, log ratio and MELR
within 1e-4, exact zeros for identical fields, bitwise-reproducible and graph-capturable sums, refusals."""
import json
import math

import numpy as np
import pytest
import torch

from dlwp_benchmark_amd.lib import DlwpError
from dlwp_benchmark_amd.metrics import ZonalSpectrumMetrics
from zonal_spectrum_ref import melr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _linspace_lats(h):
    return torch.linspace(-90, 90, h, dtype=torch.float64)


def _cell_centres(h):
    return 90 - (torch.arange(h, dtype=torch.float64) + 0.5) * (180 / h)


def _field(shape, seed):
    """A smooth red spectrum (amplitude (1 + m)^-0.75 in every bin, random phases varying slowly with latitude) plus white
    noise of std 0.02: every bin carries at least ~1e-4 of the peak power."""
    g = torch.Generator().manual_seed(seed)
    b, k, c, h, w = shape
    n = torch.arange(w, dtype=torch.float64, device=DEV)
    x = torch.zeros(shape, dtype=torch.float64, device=DEV)
    for m in range(w // 2 + 1):
        amp = (1.0 + m) ** -0.75
        phase = 2 * math.pi * torch.rand(b, k, c, 1, 1, generator=g, dtype=torch.float64).to(DEV)
        tilt = torch.linspace(0, 1, h, dtype=torch.float64)[:, None] * torch.rand(1, generator=g, dtype=torch.float64)
        x += amp * torch.cos(2 * math.pi * m * n / w + phase + tilt.to(DEV))
    x += 0.02 * torch.randn(shape, generator=g, dtype=torch.float64).to(DEV)
    return x.float().cpu()


# Shapes on which a workgroup walks SEVERAL row chunks (register prefetch of the next chunk, per-chunk weights, sums
# carried across chunks) and a segment ends on a partial chunk: the path of the C4 / C5 evaluation shapes.
MULTI_CHUNK = [(3, 20, 3, 120, 256), (16, 12, 3, 130, 64), (2, 40, 3, 100, 512)]


def _assert_multi_chunk(shape):
    """From the public workspace query ([2][K C][S][W/2 + 1] doubles): S segments share the B H rows of a plane, in chunks of
    8192 / W rows, segments starting on chunk boundaries.  More rows than S chunks -> some segment walks several chunks; rows
    not a multiple of the chunk -> a segment ends on a partial one."""
    from dlwp_benchmark_amd import lib

    b, k, c, h, w = shape
    segs = lib.load().dlwp_zonal_power_workspace_bytes(b, k, c, h, w) // (16 * k * c * (w // 2 + 1))
    rch = 8192 // w
    assert b * h > segs * rch, (shape, segs)
    assert (b * h) % rch != 0, (shape, segs)


def _check(got, out, tar, lats):
    want = melr(out.cpu().numpy(), tar.cpu().numpy(), lats.numpy())
    for key in ("energy_pred", "energy_true"):
        g = got[key].cpu().numpy()
        assert g.shape == want[key].shape
        assert np.allclose(g, want[key], rtol=1e-4, atol=0), (key, np.abs(g / want[key] - 1).max())
    for key in ("log_ratio", "melr"):
        g = got[key].cpu().numpy()
        assert np.allclose(g, want[key], rtol=0, atol=1e-4), (key, np.abs(g - want[key]).max())


@pytest.mark.parametrize("shape", [(3, 2, 3, 32, 64), (2, 3, 2, 128, 256), (1, 1, 1, 5, 32), (2, 1, 2, 16, 512)])
@pytest.mark.parametrize("lats", ["linspace", "centres"])
def test_matches_restatement(shape, lats):
    lat = (_linspace_lats if lats == "linspace" else _cell_centres)(shape[3])
    out, tar = _field(shape, 1), _field(shape, 2)
    m = ZonalSpectrumMetrics(lat)
    got = m(out.to(DEV), tar.to(DEV))
    _check(got, out, tar, lat)


@pytest.mark.parametrize("shape", MULTI_CHUNK)
@pytest.mark.parametrize("lats", ["linspace", "centres"])
def test_multi_chunk_segments_match_restatement(shape, lats):
    _assert_multi_chunk(shape)
    lat = (_linspace_lats if lats == "linspace" else _cell_centres)(shape[3])
    out, tar = _field(shape, 13), _field(shape, 14)
    got = ZonalSpectrumMetrics(lat)(out.to(DEV), tar.to(DEV))
    _check(got, out, tar, lat)


@pytest.mark.parametrize("shape", MULTI_CHUNK)
def test_multi_chunk_sums_are_bitwise_reproducible(shape):
    _assert_multi_chunk(shape)
    out, tar = _field(shape, 15).to(DEV), _field(shape, 16).to(DEV)
    m = ZonalSpectrumMetrics(_cell_centres(shape[3]))
    a = m.sums(out, tar).clone()
    assert torch.equal(a, m.sums(out, tar))


def test_workspace_is_shared_by_shapes():
    m = ZonalSpectrumMetrics(_cell_centres(32))
    big = torch.zeros(8, 4, 3, 32, 64, device=DEV)
    small = big[:2]
    m.sums(big, big)
    first = m._ws[str(big.device)][-1]
    m.sums(small, small)                 # needs less: the same buffer
    assert len(m._ws[str(big.device)]) == 1 and m._ws[str(big.device)][-1] is first


def test_non_contiguous_slice_of_a_rollout():
    big_o, big_t = _field((2, 4, 3, 32, 64), 3).to(DEV), _field((2, 4, 3, 32, 64), 4).to(DEV)
    out, tar = big_o[:, 1:3, ::2], big_t[:, 1:3, ::2]
    assert not out.is_contiguous()
    lat = _cell_centres(32)
    _check(ZonalSpectrumMetrics(lat)(out, tar), out, tar, lat)


def test_same_tensor_gives_exact_zero():
    x = _field((2, 3, 2, 32, 64), 5).to(DEV)
    got = ZonalSpectrumMetrics(_linspace_lats(32))(x, x)
    assert torch.all(got["log_ratio"] == 0.0) and torch.all(got["melr"] == 0.0)


@pytest.mark.parametrize("w,m0", [(32, 3), (64, 31), (256, 17), (512, 200)])
def test_pure_zonal_wave(w, m0):
    h = 6
    n = torch.arange(w, dtype=torch.float64)
    phase = torch.linspace(0, 2, h, dtype=torch.float64)[:, None]
    x = (1.3 * torch.cos(2 * math.pi * m0 * n / w + phase)).float().expand(2, 1, 1, h, w).contiguous()
    lat = _cell_centres(h)
    got = ZonalSpectrumMetrics(lat)(x.to(DEV), x.to(DEV))
    want = melr(x.numpy(), x.numpy(), lat.numpy())["energy_pred"][0, 0]
    e = got["energy_pred"][0, 0].cpu().numpy()
    assert abs(e[m0] / want[m0] - 1) <= 1e-6
    assert np.abs(np.delete(e, m0)).max() <= 1e-9 * e[m0]


def test_sums_are_bitwise_reproducible():
    out, tar = _field((4, 5, 3, 128, 256), 6).to(DEV), _field((4, 5, 3, 128, 256), 7).to(DEV)
    m = ZonalSpectrumMetrics(_cell_centres(128))
    a = m.sums(out, tar).clone()
    b = m.sums(out, tar)
    assert torch.equal(a, b)


@pytest.mark.parametrize("w", [48, 360, 1024])
def test_unsupported_width_is_refused(w):
    x = torch.zeros(1, 1, 1, 4, w, device=DEV)
    with pytest.raises(DlwpError, match="not supported"):
        ZonalSpectrumMetrics(_cell_centres(4)).sums(x, x)


def test_healpix_rollout_is_refused():
    x = torch.zeros(1, 2, 12, 1, 8, 8, device=DEV)
    with pytest.raises(DlwpError, match="HEALPix"):
        ZonalSpectrumMetrics(_cell_centres(8)).sums(x, x)


def test_running_sums_over_batches_equal_the_whole_set():
    out, tar = _field((5, 2, 3, 32, 64), 8).to(DEV), _field((5, 2, 3, 32, 64), 9).to(DEV)
    m = ZonalSpectrumMetrics(_cell_centres(32))
    whole = m.sums(out, tar)
    run = torch.zeros(2, 2, 3, 33, dtype=torch.float64, device=DEV)
    assert m.sums(out[:3], tar[:3], into=run) is run
    m.sums(out[3:], tar[3:], into=run)
    assert torch.allclose(run, whole, rtol=1e-12, atol=0)
    res = m.finalize(run, 5.0)
    _check(res, out, tar, _cell_centres(32))
    with pytest.raises(DlwpError, match="double"):
        m.sums(out, tar, into=torch.zeros(2, 2, 3, 33, dtype=torch.float32, device=DEV))
    with pytest.raises(DlwpError, match="double"):
        m.sums(out, tar, into=torch.zeros(2, 2, 3, 32, dtype=torch.float64, device=DEV))


def test_replayed_sums_equal_eager_bitwise():
    from dlwp_benchmark_amd.sharding import CapturedStep

    out, tar = _field((2, 4, 3, 64, 128), 10).to(DEV), _field((2, 4, 3, 64, 128), 11).to(DEV)
    m = ZonalSpectrumMetrics(_cell_centres(64))
    want = m.sums(out, tar).clone()
    cap = CapturedStep(lambda o, t: m.sums(o, t))
    for _ in range(3):
        got = cap(out, tar)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert cap.replays == 2
    out2 = _field((2, 4, 3, 64, 128), 12).to(DEV)
    want2 = m.sums(out2, tar).clone()
    out.copy_(out2)                      # the same address, new contents: the replay reads them
    got = cap(out, tar)
    torch.cuda.synchronize()
    assert torch.equal(got, want2)


def test_backbone_rollout_scored_on_device():
    """A real Swin rollout (the golden C3 configuration of test_backbones_gpu.py) scored against its reference
    trajectory on the device equals the restatement of the same trajectories on the host."""
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec
    from helpers import load_golden
    from oracle.make_golden import MODEL_CASES, model_inputs

    tag = "swin_c3_full"
    family, cfg, (batch, frames), gain = MODEL_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, _ = fill_by_spec(json.loads(str(g["param_spec"])), gain=gain)
    model = M.SwinTransformer(**cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(DEV).eval()
    constants, prescribed, prognostic = model_inputs(tag, cfg, batch, frames)
    dev = lambda t: t.to(DEV) if t is not None else None
    with torch.no_grad():
        got = model(constants=dev(constants), prescribed=dev(prescribed), prognostic=dev(prognostic))
    target = torch.from_numpy(g["y"]).to(DEV)
    lat = _cell_centres(got.shape[-2])
    res = ZonalSpectrumMetrics(lat)(got, target)
    _check(res, got, target, lat)
