"""The year-long soundness evaluation on the device: dlwp_climate_sums_acc_f32 against numpy float64 and across chunkings,
`metrics.SoundnessMetrics` end to end, the fixed-memory driver `rollout.rollout_chunks` against the one-shot forward, and
`ops.insolation` against fixtures of the real reference function (tools/make_golden_insolation.py)."""
import numpy as np
import pytest
import torch

from helpers import fno_std_fn, load_golden, per_step_rel_l2
from test_soundness_cpu import INSOLATION_CASES, LATS, insolation_from_tables, soundness_numpy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _launch(out, tar, zonal, window, wb, we, accept=()):
    from dlwp_benchmark_amd import lib

    b, k, c, h, w = out.shape
    return lib.launch("dlwp_climate_sums_acc_f32", DEV, out, tar, zonal, window, b, k, c, h, w, wb, we, accept=accept)


def _offset_fields(shape, seed):
    """1e4 + N(0, 1): with a common offset 2^13 times the spread an fp32 partial anywhere loses what the bound allows"""
    g = torch.Generator().manual_seed(seed)
    out = (1e4 + torch.randn(shape, generator=g)).float()
    tar = (1e4 + torch.randn(shape, generator=g)).float()
    return out, tar


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("shape", [
    (1, 1, 1, 1, 1),
    (2, 3, 3, 5, 20),
    (1, 4, 1, 7, 37),        # odd W: 4-byte loads
    (2, 2, 2, 33, 64),
    (1, 2, 1, 3, 260),       # 65 load units: a row longer than a wave's first sweep
    (1, 3, 1, 2, 130),       # 4-byte loads past the units whose window sums ride in registers
    (1, 2, 1, 2, 520),       # 16-byte loads past them
    (2, 2, 3, 11000, 4),     # B C H = 66000 rows > 65535, one lane per row
])
def test_climate_sums_match_numpy_float64(shape):
    """every sum within 2^-52 n sum|x_i| of numpy's float64 sum of the same float32 inputs: the textbook bound
    (n - 1) u sum|x_i|, u = 2^-53, of n sequential fp64 adds, doubled"""
    b, k, c, h, w = shape
    out, tar = _offset_fields(shape, 7)
    wb, we = (k // 2, k) if k > 1 else (0, 1)
    x = torch.stack([out, tar]).double().numpy()                       # [2, B, K, C, H, W]
    zonal = torch.zeros(2, b, c, h, dtype=torch.float64, device=DEV)
    window = torch.zeros(2, b, c, h, w, dtype=torch.float64, device=DEV)
    assert _launch(out.to(DEV), tar.to(DEV), zonal, window, wb, we) == 0
    torch.cuda.synchronize()
    want_z, abs_z = x.sum(axis=(2, 5)), np.abs(x).sum(axis=(2, 5))
    err = np.abs(zonal.cpu().numpy() - want_z)
    bound = 2.0 ** -52 * (k * w) * abs_z
    print(f"{shape}: zonal max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    want_w, abs_w = x[:, :, wb:we].sum(axis=2), np.abs(x[:, :, wb:we]).sum(axis=2)
    err = np.abs(window.cpu().numpy() - want_w)
    assert (err <= 2.0 ** -52 * (we - wb) * abs_w).all()
    # the sums are RUNNING sums: a second call adds onto the first
    assert _launch(out.to(DEV), tar.to(DEV), zonal, None, 0, 0) == 0
    err = np.abs(zonal.cpu().numpy() - 2 * want_z)
    assert (err <= 2.0 ** -52 * (2 * k * w) * 2 * abs_z).all()


@pytest.mark.parametrize("shape", [(2, 11, 2, 5, 20), (1, 11, 1, 3, 37), (1, 11, 1, 2, 130), (1, 11, 1, 2, 520), (3, 11, 1, 70, 4)])
def test_climate_sums_do_not_depend_on_the_chunking(shape):
    """a K = 11 trajectory whole, step by step and as 4 + 7, the window on steps 3 ... 8: the same bits; twice: the same bits;
    and from a view 4 bytes off a 16-byte boundary: the same bits"""
    b, k, c, h, w = shape
    out, tar = _offset_fields(shape, 11)
    out, tar = out.to(DEV), tar.to(DEV)
    lo, hi = 3, 9

    def run(cuts, o=out, t=tar):
        zonal = torch.zeros(2, b, c, h, dtype=torch.float64, device=DEV)
        window = torch.zeros(2, b, c, h, w, dtype=torch.float64, device=DEV)
        for s0, s1 in zip(cuts[:-1], cuts[1:]):
            wb, we = min(max(lo - s0, 0), s1 - s0), min(max(hi - s0, 0), s1 - s0)
            assert _launch(o[:, s0:s1].contiguous(), t[:, s0:s1].contiguous(), zonal, window if we > wb else None, wb, max(we, wb)) == 0
        torch.cuda.synchronize()
        return zonal, window

    whole = run([0, 11])
    for cuts in ([0, 11], list(range(12)), [0, 4, 11]):
        z, wn = run(cuts)
        assert torch.equal(z, whole[0]) and torch.equal(wn, whole[1]), cuts
    # an unaligned view of the same values (the 4-byte loads of the 16-byte path's elements)
    shifted = [torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape).copy_(x) for x in (out, tar)]
    assert shifted[0].data_ptr() % 16 == 4
    z, wn = run([0, 11], *shifted)
    assert torch.equal(z, whole[0]) and torch.equal(wn, whole[1])
    want = torch.stack([out, tar]).double()
    assert torch.allclose(whole[1], want[:, :, lo:hi].sum(dim=2), rtol=1e-14, atol=0)


def test_climate_sums_window_edge_cases_and_bad_arguments():
    from dlwp_benchmark_amd.lib import DlwpError

    shape = (1, 3, 2, 4, 8)
    out, tar = (x.to(DEV) for x in _offset_fields(shape, 3))
    zonal = torch.zeros(2, 1, 2, 4, dtype=torch.float64, device=DEV)
    window = torch.full((2, 1, 2, 4, 8), 5.0, dtype=torch.float64, device=DEV)
    for wb, we in ((0, 0), (2, 2), (3, 3)):                                 # empty windows leave `window` untouched
        assert _launch(out, tar, zonal, window, wb, we) == 0
    torch.cuda.synchronize()
    assert torch.equal(window, torch.full_like(window, 5.0))
    assert _launch(out, tar, zonal, None, 1, 3) == 0                        # a null window is accepted, whatever the range
    torch.cuda.synchronize()
    assert torch.allclose(zonal, 4 * torch.stack([out, tar]).double().sum(dim=(2, 5)), rtol=1e-14, atol=0)
    before = zonal.clone()
    for wb, we in ((-1, 2), (2, 1), (0, 4), (4, 4)):
        assert _launch(out, tar, zonal, window, wb, we, accept=(-1,)) == -1
    from dlwp_benchmark_amd import lib

    for args in ((None, tar, zonal), (out, None, zonal), (out, tar, None)):
        assert lib.launch("dlwp_climate_sums_acc_f32", DEV, *args, None, 1, 3, 2, 4, 8, 0, 0, accept=(-1,)) == -1
    for dims in ((0, 3, 2, 4, 8), (1, 0, 2, 4, 8), (1, 3, -2, 4, 8), (1, 3, 2, 0, 8), (1, 3, 2, 4, 0)):
        assert lib.launch("dlwp_climate_sums_acc_f32", DEV, out, tar, zonal, None, *dims, 0, 0, accept=(-1,)) == -1
    with pytest.raises(DlwpError, match="window"):
        _launch(out, tar, zonal, window, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(zonal, before)                                       # a refused call launches nothing


# ------------------------------------------------------------------ SoundnessMetrics
def _rollout_pair(b, k, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    tar = torch.randn(b, k, c, h, w, generator=g)
    out = tar + 0.3 * torch.randn(b, k, c, h, w, generator=g) + 0.1 * torch.linspace(-1, 1, h).view(1, 1, 1, h, 1)
    return out.float(), tar.float()


def test_soundness_metrics_end_to_end():
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.metrics import DEFAULT_BANDS, SoundnessMetrics

    out, tar = _rollout_pair(2, 12, 3, 36, 8, 5)
    std = torch.tensor([2.0, 0.5, 30.0])
    want, want_window = soundness_numpy(out.numpy(), tar.numpy(), LATS, 1.0, std.numpy(), None, (5, 9))
    results = []
    for cuts in ([0, 12], [0, 5, 12], list(range(13))):
        m = SoundnessMetrics(LATS, 1.0, std=std, window_days=(5, 9))
        for s0, s1 in zip(cuts[:-1], cuts[1:]):
            m.update(out[:, s0:s1].to(DEV), tar[:, s0:s1].to(DEV), s0)
        assert m.steps == 12 and m.n_window_steps == 5
        res = m.finalize()
        assert res["zonal_mean_pred"].is_cuda and res["zonal_mean_pred"].dtype == torch.float64
        assert tuple(res["zonal_mean_true"].shape) == (2, 3, 36) and tuple(res["window_mean_pred"].shape) == (2, 3, 36, 8)
        for name in DEFAULT_BANDS:
            np.testing.assert_allclose(res["rmse"][name].cpu().numpy(), want[name], rtol=1e-12, atol=0)
        np.testing.assert_allclose(res["rmse_window"].cpu().numpy(), want_window, rtol=1e-12, atol=0)
        results.append(res)
    for res in results[1:]:                                                 # the chunking does not show in any bit
        for key in ("zonal_mean_pred", "zonal_mean_true", "window_mean_pred", "window_mean_true", "rmse_window"):
            assert torch.equal(res[key], results[0][key]), key
    # a changed geometry, a gap and a CPU tensor are refused; reset() starts over
    with pytest.raises(DlwpError, match="after chunks with"):
        m.update(out[:1, :2].to(DEV), tar[:1, :2].to(DEV), 12)
    with pytest.raises(DlwpError, match="in order"):
        m.update(out[:, :2].to(DEV), tar[:, :2].to(DEV), 13)
    with pytest.raises(DlwpError, match="MI355X"):
        m.update(out[:, :2], tar[:, :2], 12)
    m.reset()
    m.update(out[:, :4].to(DEV), tar[:, :4].to(DEV), 0)
    assert m.finalize()["rmse_window"] is None                              # four daily steps never reach day 5


@pytest.mark.parametrize("batch, workspace_samples", [(1, 1), (3, 2)])
def test_soundness_metrics_remap_healpix_chunks(batch, workspace_samples):
    """a HEALPix chunk equals the lat-lon path on ops.healpix_to_latlon of the same tensors, bit for bit -- also when the
    workspace holds fewer samples than the batch and the sums go through per-sample slices"""
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.metrics import SoundnessMetrics

    lons = np.arange(8) * 45.0
    g = torch.Generator().manual_seed(9)
    out = torch.randn(batch, 6, 2, 12, 4, 4, generator=g).to(DEV)
    tar = torch.randn(batch, 6, 2, 12, 4, 4, generator=g).to(DEV)
    per_sample = 8 * 6 * 2 * 36 * 8
    hpx = SoundnessMetrics(LATS, 1.0, window_days=(2, 5), lons_deg=lons, max_workspace_bytes=workspace_samples * per_sample)
    ll = SoundnessMetrics(LATS, 1.0, window_days=(2, 5))
    for s0, s1 in ((0, 4), (4, 6)):
        hpx.update(out[:, s0:s1], tar[:, s0:s1], s0)
        ll.update(ops.healpix_to_latlon(out[:, s0:s1], LATS, lons), ops.healpix_to_latlon(tar[:, s0:s1], LATS, lons), s0)
    a, b = hpx.finalize(), ll.finalize()
    for key in ("zonal_mean_pred", "zonal_mean_true", "window_mean_pred", "window_mean_true", "rmse_window"):
        assert torch.equal(a[key], b[key]), key
    for name in a["rmse"]:
        assert torch.equal(a["rmse"][name], b["rmse"][name])
    with pytest.raises(DlwpError, match="lons_deg"):
        ll.update(out[:, :1], tar[:, :1], 6)


# ------------------------------------------------------------------ rollout_chunks
UNET_KW = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], n_convolutions=2,
               context_size=2)
FNO_KW = dict(n_modes=[12, 12], constant_channels=0, prescribed_channels=0, prognostic_channels=1, hidden_channels=32,
              lifting_channels=256, projection_channels=256, n_layers=4, context_size=1)
STEPS = 7


@pytest.fixture(scope="module")
def unet_case():
    """(model, constants, prescribed, prognostic, the one-shot forward): computed once, left unchanged"""
    from dlwp_benchmark_amd import models as M
    from dlwp_benchmark_amd.synthetic import weatherbench
    from dlwp_benchmark_amd.weights import fill_state_dict

    model = M.UNet(**UNET_KW)
    fill_state_dict(model, gain=1.0)
    model = model.to(DEV).eval()
    cons, presc, prog = (t.to(DEV) for t in weatherbench(2, 2 + STEPS, 16, 32, prognostic_channels=2, constant_channels=2))
    want = model(constants=cons, prescribed=presc, prognostic=prog)
    torch.cuda.synchronize()
    return model, cons, presc, prog, want


def _collect(gen):
    """the chunks of a rollout_chunks generator, cloned (a chunk is valid until the next one) and concatenated"""
    parts, begins = [], []
    for s0, chunk in gen:
        begins.append(s0)
        parts.append(chunk.clone())
    return begins, torch.cat(parts, dim=1)


@pytest.mark.parametrize("chunk_steps", [1, 3, 7])
def test_rollout_chunks_unet_equals_the_one_shot_forward(unet_case, chunk_steps):
    from dlwp_benchmark_amd.rollout import rollout_chunks

    model, cons, presc, prog, want = unet_case
    begins, got = _collect(rollout_chunks(model, cons, presc, prog[:, :2], STEPS, chunk_steps))
    assert begins == list(range(0, STEPS, chunk_steps))
    assert torch.equal(got, want)
    calls = []

    def forcing(f0, f1):                                  # the callable form: the same frames on demand
        calls.append((f0, f1))
        return presc[:, f0:f1]

    _, got = _collect(rollout_chunks(model, cons, forcing, prog[:, :2], STEPS, chunk_steps))
    assert torch.equal(got, want)
    assert calls == [(s0, s0 + 2 + min(chunk_steps, STEPS - s0)) for s0 in begins]


def test_rollout_chunks_fno_equals_the_one_shot_forward():
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.rollout import rollout_chunks
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    ref = FNO2DModuleRef(**FNO_KW).eval()
    fill_state_dict(ref, std_fn=fno_std_fn(0.85), gain=0.85)
    hip = FNO2DModule(**FNO_KW)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(DEV).eval()
    prog = navier_stokes(2, 1 + STEPS)[2].to(DEV)
    want = hip(prognostic=prog)
    for chunk_steps in (1, 3, 7):
        begins, got = _collect(rollout_chunks(hip, None, None, prog[:, :1], STEPS, chunk_steps))
        assert begins == list(range(0, STEPS, chunk_steps))
        errs = per_step_rel_l2(got, want)
        print(f"FNO chunk_steps = {chunk_steps}: bit-equal {torch.equal(got, want)}, per-step rel L2 max {max(errs):.2e}")
        assert torch.equal(got, want), chunk_steps


def test_rollout_chunks_healpix_backbone_goes_through_forward():
    """a HEALPix class folds the faces itself, so its chunks are whole forwards: the same bits as the one-shot forward"""
    from dlwp_benchmark_amd import models as M
    from dlwp_benchmark_amd.rollout import rollout_chunks
    from dlwp_benchmark_amd.weights import fill_state_dict

    model = M.UNetHPX(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], context_size=2)
    fill_state_dict(model, gain=1.0)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    cons = torch.randn(1, 1, 1, 12, 8, 8, generator=g).to(DEV)
    presc = torch.randn(1, 2 + 5, 1, 12, 8, 8, generator=g).to(DEV)
    prog = torch.randn(1, 2 + 5, 2, 12, 8, 8, generator=g).to(DEV)
    want = model(constants=cons, prescribed=presc, prognostic=prog)
    for chunk_steps in (1, 2, 5):
        begins, got = _collect(rollout_chunks(model, cons, presc, prog[:, :2], 5, chunk_steps))
        assert begins == list(range(0, 5, chunk_steps)) and torch.equal(got, want), chunk_steps


def test_rollout_chunks_refusals():
    from dlwp_benchmark_amd import models as M
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.rollout import rollout_chunks

    clstm = M.ConvLSTM(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_sizes=[4, 4], height=8, width=16)
    x = torch.zeros(1, 1, 2, 8, 16, device=DEV)
    with pytest.raises(DlwpError, match="recurrent"):
        rollout_chunks(clstm.to(DEV), None, None, x, 4, 2)
    diff = M.DiffModernUNet(constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_channels=[8, 16],
                            context_size=1, norm=False, use_scale_shift_norm=False)
    with pytest.raises(DlwpError, match="scheduler"):
        rollout_chunks(diff, None, None, x, 4, 2)
    unet = M.UNet(**UNET_KW)
    with pytest.raises(DlwpError, match="initial frames"):
        rollout_chunks(unet, None, None, torch.zeros(1, 3, 2, 8, 16, device=DEV), 4, 2)      # three frames for context_size 2
    with pytest.raises(DlwpError, match="positive"):
        rollout_chunks(unet, None, None, torch.zeros(1, 2, 2, 8, 16, device=DEV), 0, 2)


def test_rollout_chunks_memory_does_not_grow_with_the_horizon(unet_case):
    """the peak of a 64-step run may exceed the peak of a 16-step run (both in chunks of 4) by one chunk buffer at most"""
    from dlwp_benchmark_amd.rollout import rollout_chunks

    model, cons, presc, prog, _ = unet_case
    forcing = lambda f0, f1: presc[:, :f1 - f0]          # any horizon from the frames at hand

    def peak(n_steps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        for _ in rollout_chunks(model, cons, forcing, prog[:, :2], n_steps, 4):
            pass
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(DEV) - base

    peak(8)                                              # warm-up: plans, packed weights, workspaces
    short, long = peak(16), peak(64)
    chunk_buffer = 4 * prog[:, :4].numel()
    print(f"peak above the inputs: 16 steps {short} B, 64 steps {long} B, one chunk buffer {chunk_buffer} B")
    assert long <= short + chunk_buffer


# ------------------------------------------------------------------ insolation
@pytest.mark.parametrize("tag", INSOLATION_CASES)
def test_insolation_matches_the_reference_fixture(tag):
    from dlwp_benchmark_amd import ops

    fx = load_golden(f"insolation_{tag}")
    dates = [str(d) for d in fx["dates"]]
    got = ops.insolation(dates, fx["lat"], fx["lon"], device=DEV)
    assert got.dtype == torch.float32 and tuple(got.shape) == fx["sol"].shape and got.is_cuda
    err = float((got.cpu().double() - torch.from_numpy(fx["sol"]).double()).abs().max())
    print(f"{tag}: max abs difference {err:.3e} (bound 1.2e-7)")
    assert err <= 1.2e-7                                                   # one float32 ulp at 1.0; values in [0, 1.04]
    if "sol_daily" in fx:
        daily = ops.insolation(dates, fx["lat"], fx["lon"], daily=True, device=DEV)
        assert float((daily.cpu().double() - torch.from_numpy(fx["sol_daily"]).double()).abs().max()) <= 1.2e-7


def test_insolation_options():
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.lib import DlwpError

    fx = load_golden("insolation_mesh8x20_yearend")
    dates = [str(d) for d in fx["dates"]]
    lat, lon = fx["lat"], fx["lon"]
    plain = ops.insolation(dates, lat, lon, device=DEV)
    # the 1-D mesh and the per-cell form of the same points
    lon2, lat2 = np.meshgrid(lon, lat)
    assert torch.equal(ops.insolation(dates, lat2, lon2, device=DEV), plain)
    # normalisation in the same pass: (x - mean) / std on the rounded value, in float32
    mean, std = 0.25, 0.31
    norm = ops.insolation(dates, lat, lon, mean=mean, std=std, device=DEV)
    want = (plain.cpu().numpy() - np.float32(mean)) / np.float32(std)
    assert (np.abs(norm.cpu().numpy() - want) <= np.spacing(np.abs(want))).all()
    # out= is written in place and returned
    buf = torch.full((3,) + tuple(plain.shape), -7.0, device=DEV)
    ret = ops.insolation(dates, lat, lon, out=buf[1])
    assert ret.data_ptr() == buf[1].data_ptr() and torch.equal(buf[1], plain)
    assert bool((buf[0] == -7.0).all()) and bool((buf[2] == -7.0).all())
    # S scales, clip_zero=False keeps the night side negative
    date_tab, point_tab, grid = ops.insolation_tables(dates, lat, lon)
    scaled = ops.insolation(dates, lat, lon, S=1361.0, clip_zero=False, device=DEV).cpu().numpy()
    host = insolation_from_tables(date_tab, point_tab, S=1361.0, clip_zero=False).reshape(scaled.shape)
    assert scaled.min() < -100.0 and (np.abs(scaled - host) <= np.spacing(np.abs(host))).all()
    with pytest.raises(DlwpError, match="both mean and std"):
        ops.insolation(dates, lat, lon, mean=0.0, device=DEV)
    with pytest.raises(DlwpError, match="out must be"):
        ops.insolation(dates, lat, lon, out=buf)


def test_insolation_forcing_feeds_rollout_chunks(unet_case):
    """the callable built by insolation_forcing gives what the tensor of the same fields gives"""
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.rollout import insolation_forcing, rollout_chunks

    model, cons, _, prog, _ = unet_case
    lat, lon = np.linspace(-84.375, 84.375, 16), np.arange(32) * 11.25
    dates = np.datetime64("2019-12-29T00:00:00") + np.arange(2 + STEPS) * np.timedelta64(6, "h")
    field = ops.insolation(dates, lat, lon, mean=0.3, std=0.4, device=DEV)                       # [T, H, W]
    presc = field.view(1, 2 + STEPS, 1, 16, 32).expand(2, -1, -1, -1, -1).contiguous()
    _, want = _collect(rollout_chunks(model, cons, presc, prog[:, :2], STEPS, 3))
    forcing = insolation_forcing(dates, lat, lon, batch=2, mean=0.3, std=0.4, device=DEV)
    assert torch.equal(forcing(1, 4), presc[:, 1:4])
    _, got = _collect(rollout_chunks(model, cons, forcing, prog[:, :2], STEPS, 3))
    assert torch.equal(got, want)
